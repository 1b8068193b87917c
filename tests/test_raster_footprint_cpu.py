"""The rasteriser's culling footprints are conservative (no GPU): csrc/raster.hpp compiled for the host (raster_hostcheck.py).

raster_k ray-tests a moving primitive only inside prim_span's footprint and raster_tiles_k only in the tiles prim_screen_rect's
rectangle overlaps, so a footprint that under-covers by one pixel silently loses that pixel.  Per sample (primitive, camera, size):
  P   pixels where the kernel's own exact test (hit_prim; hit_capsule_k for capsules) hits,
  F   pixels the object-order walk visits (band loop, span_band_chunks, span_locate: every chunk, wavefront offset and lane),
  Ft  pixels of the 8x8 tiles whose mask holds the primitive.
Properties, no tolerance: P within F and Ft; F inside the image and inside its band, no pixel twice; the lane arithmetic of
span_locate; hit_capsule_k == hit_capsule bit for bit at every pixel.  The samples are drawn so that every branch of the footprint
code is reached by primitives that are actually visible — the class counts at the end are asserted, not only printed."""
import numpy as np
import pytest

import raster_hostcheck as rh

SIZES = [(64, 64), (224, 224), (50, 38), (16, 1024), (300, 12), (8, 8)]
# samples per (camera, size): the cost of a sample is its pixel count
N_SAMPLES = {(64, 64): 700, (224, 224): 160, (50, 38): 800, (16, 1024): 320, (300, 12): 800, (8, 8): 500}
FPV_AT = [(2.0, 2.0), (0.45, 0.4), (3.6, 3.55), (0.4, 3.2)]      # robot positions of the fpv camera: mid-arena and near three corners
CAMERAS = [("kuka0", rh.KUKA_CAM0, 0, 0), ("kuka1", rh.KUKA_CAM1, 0, 0), ("top", rh.MOBILE_TOP, 0, 0)] + \
          [("fpv{}".format(i), rh.MOBILE_FPV, x, y) for i, (x, y) in enumerate(FPV_AT)]
DEPTH = {"kuka0": (0.15, 3.0), "kuka1": (0.15, 3.0), "top": (0.3, 5.0)}      # fpv*: (0.1, 4.0)

CLASSES = ["slab active", "slab refused: slope", "slab refused: hw >= w/2", "near-plane fallback", "P at top border", "P at bottom border",
           "P at left border", "P at right border", "cch > 1", "rpc > 1", "span crosses a band"]


def world(cam, x, y, z):
    """camera-space tangent position (x, y) at depth z -> world (float64)"""
    e, f, r, u = (cam[3 * i:3 * i + 3].astype(np.float64) for i in range(4))
    x, y, z = (np.asarray(v, np.float64)[..., None] for v in (x, y, z))
    return e + z * (f + x * r + y * u)


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def make_prims(types, a, b, rad, yaw):
    n = len(types)
    out = np.zeros((n, 13), np.float32)
    out[:, 0] = types
    out[:, 1:4] = 0.5
    out[:, 4:7], out[:, 7:10], out[:, 10] = a, b, rad
    out[:, 11], out[:, 12] = np.cos(yaw), np.sin(yaw)
    return out


def sample_prims(rng, cam, zlo, zhi, n):
    """n primitives for one camera: a general draw from the view frustum with a 30 % margin on every side, plus the deliberate
    poses — near / behind the camera plane, capsule axes through the eye, axes swept through horizontal, long near capsules,
    zero-length capsules, large near boxes and cylinders."""
    tan = float(cam[12])
    parts = []

    def general(m, near=False):
        types = rng.randint(1, 4, m)
        size = log_uniform(rng, 0.005, 0.3, (3, m))
        z = rng.uniform(-0.25, 0.4, m) if near else log_uniform(rng, zlo, zhi, m)
        c = world(cam, rng.uniform(-1.3, 1.3, m) * tan, rng.uniform(-1.3, 1.3, m) * tan, z)
        a, b, rad, yaw = c.copy(), size.T.copy(), np.zeros(m), rng.uniform(-np.pi, np.pi, m)
        cyl = types == rh.CYL
        b[cyl, 1] = 0.0
        cap = types == rh.CAPSULE
        d = rng.normal(size=(m, 3))
        d *= (log_uniform(rng, 0.01, 1.0, m) / np.linalg.norm(d, axis=1))[:, None]
        a[cap], b[cap], rad[cap] = (c - d)[cap], (c + d)[cap], size[0][cap]
        return make_prims(types, a, b, rad, yaw)

    parts.append(general(int(0.36 * n)))
    parts.append(general(int(0.12 * n), near=True))                    # endpoints / corners closer than 0.05 + size to the camera plane, and behind it
    # capsule axis within a radius of an eye ray: a' ~ b'
    m = int(0.08 * n)
    x, y, rad = rng.uniform(-1.1, 1.1, m) * tan, rng.uniform(-1.1, 1.1, m) * tan, log_uniform(rng, 0.005, 0.3, m)
    z1 = log_uniform(rng, zlo, zhi, m)
    z2 = z1 + log_uniform(rng, 0.01, 1.0, m)
    off = rng.normal(size=(m, 3))
    off *= (rng.uniform(0.0, 1.0, m) * rad / np.linalg.norm(off, axis=1))[:, None]
    parts.append(make_prims(np.full(m, rh.CAPSULE), world(cam, x, y, z1) + off, world(cam, x, y, z2) + off, rad, np.zeros(m)))
    # projected axis swept through horizontal: dy / len in fine steps around the 1e-4 threshold and coarser up to 0.1 (hw around w / 2)
    m = int(0.24 * n)
    xa, xb = rng.uniform(-1.2, 0.2, m) * tan, rng.uniform(-0.2, 1.2, m) * tan
    ya = rng.uniform(-1.05, 1.05, m) * tan
    steps = np.concatenate([np.linspace(-4e-4, 4e-4, m - m // 2), np.linspace(-0.1, 0.1, m // 2)])
    yb = ya + steps * np.abs(xb - xa)
    za, zb = log_uniform(rng, zlo + 0.3, zhi, m), log_uniform(rng, zlo + 0.3, zhi, m)
    flip = rng.rand(m) < 0.5
    A, Bp = world(cam, xa, ya, za), world(cam, xb, yb, zb)
    parts.append(make_prims(np.full(m, rh.CAPSULE), np.where(flip[:, None], Bp, A), np.where(flip[:, None], A, Bp),
                            log_uniform(rng, 0.005, 0.3, m) * np.minimum(1.0, np.minimum(za, zb)), np.zeros(m)))
    # long, thick and near: hw >= w / 2
    m = int(0.08 * n)
    rad = rng.uniform(0.1, 0.3, m)
    zn = 0.06 + rad + log_uniform(rng, 0.005, 0.4, m)
    A = world(cam, rng.uniform(-1, 1, m) * tan, rng.uniform(-1, 1, m) * tan, zn)
    Bp = world(cam, rng.uniform(-1, 1, m) * tan, rng.uniform(-1, 1, m) * tan, zn + rng.uniform(0.0, 2.0, m))
    parts.append(make_prims(np.full(m, rh.CAPSULE), A, Bp, rad, np.zeros(m)))
    # zero-length capsules
    m = max(2, int(0.02 * n))
    A = world(cam, rng.uniform(-1, 1, m) * tan, rng.uniform(-1, 1, m) * tan, log_uniform(rng, zlo, zhi, m))
    parts.append(make_prims(np.full(m, rh.CAPSULE), A, A, log_uniform(rng, 0.005, 0.3, m), np.zeros(m)))
    # large near boxes and cylinders: wide footprints (cch > 1), every border
    m = n - sum(len(p) for p in parts)
    types = rng.randint(1, 3, m)
    z = log_uniform(rng, max(zlo, 0.4), 0.5 * (zlo + zhi), m)
    c = world(cam, rng.uniform(-1.2, 1.2, m) * tan, rng.uniform(-1.2, 1.2, m) * tan, z)
    b = rng.uniform(0.1, 0.3, (m, 3))
    b[types == rh.CYL, 1] = 0.0
    parts.append(make_prims(types, c, b, np.zeros(m), rng.uniform(-np.pi, np.pi, m)))
    return np.concatenate(parts)


def describe(p):
    return "type {} a ({:.9g}, {:.9g}, {:.9g}) b ({:.9g}, {:.9g}, {:.9g}) rad {:.9g} cs {:.9g} sn {:.9g}".format(int(p[0]), *p[4:13])


def check_batch(prims, cam, h, w, label):
    """the properties on one batch; returns (samples, samples with non-empty P, class counts among those)"""
    o = rh.footprints(prims, cam, h, w, capsule_t=True)
    P, F, Ft = o["P"], o["F"], o["Ft"]
    B = len(prims)
    lostF, lostT = (P & (F == 0)).reshape(B, -1).sum(1), (P & ~Ft).reshape(B, -1).sum(1)
    for lost, what in ((lostF, "the span walk (prim_span / span_locate)"), (lostT, "the tile masks (prim_screen_rect)")):
        if lost.any():
            i = int(np.argmax(lost))
            pytest.fail("{} {}x{}: {} of {} samples lose pixels in {}; worst: {} of {} hit pixels, {}".format(
                label, h, w, int((lost > 0).sum()), B, what, int(lost[i]), int(P[i].sum()), describe(prims[i])))
    for key in ("outside_image", "outside_band", "bad_lane", "tile_mask_overflow"):
        assert not o[key].any(), "{} {}x{}: {} at {}".format(label, h, w, key, describe(prims[int(np.argmax(o[key]))]))
    assert F.max(initial=0) <= 1, "{} {}x{}: a pixel is visited twice: {}".format(label, h, w, describe(prims[int(np.argmax(F.reshape(B, -1).max(1)))]))
    assert np.array_equal(o["visits"], F.reshape(B, -1).sum(1, dtype=np.int64))
    # lane -> (row span, column) arithmetic of span_locate at the W the spans really have
    Wc, lanes = np.maximum(o["W"], 1).astype(np.int64), np.arange(64)
    small = Wc <= 64
    rr = (lanes[None, :] * o["inv_w"][small, None].astype(np.int64)) >> 16
    assert np.array_equal(rr, lanes[None, :] // Wc[small, None])
    i = lanes[None, :] - rr * Wc[small, None]
    assert (i >= 0).all() and (i < Wc[small, None]).all()
    assert np.array_equal(o["rpc"][small], np.maximum(1, 64 // Wc[small])) and (o["rpc"][~small] == 1).all()
    assert ((rr < o["rpc"][small, None]).sum(1) == o["rpc"][small] * Wc[small]).all()       # the lanes in use: rpc full row spans
    assert np.array_equal(o["cch"], (Wc + 63) // 64)
    # hit_capsule_k == hit_capsule, bits of t and code, every pixel
    cap = prims[:, 0] == rh.CAPSULE
    assert np.array_equal(o["ta"][cap].view(np.uint32), o["tk"][cap].view(np.uint32)), label
    assert np.array_equal(o["ca"][cap], o["ck"][cap]), label
    assert np.array_equal(o["tk"][cap] > 0, P[cap])
    # classes
    seen = P.reshape(B, -1).any(1)
    slab_on = cap & (o["hw"] < 1e30)
    assigned = (o["xc0"] != 0) | (o["kx"] != 0)
    fallback = o["x0"] < -1e38
    # (a capsule with the slab never started: its rectangle is the 8-corner one alone; told from the slope refusal by the rectangle test below)
    ax, bx = prims[:, 4:7].astype(np.float64) - cam[0:3], prims[:, 7:10].astype(np.float64) - cam[0:3]
    zmin = np.minimum(ax @ cam[3:6].astype(np.float64), bx @ cam[3:6].astype(np.float64)) - prims[:, 10]
    nonempty = (o["W"] > 0) & (o["r1"] >= o["r0"])
    cls = {
        "slab active": slab_on,
        "slab refused: slope": cap & ~slab_on & ~assigned & (zmin > 0.06) & nonempty & (np.abs(prims[:, 4:7] - prims[:, 7:10]).max(1) > 0),
        "slab refused: hw >= w/2": cap & ~slab_on & assigned,
        "near-plane fallback": fallback,
        "P at top border": P[:, 0, :].any(1), "P at bottom border": P[:, -1, :].any(1),
        "P at left border": P[:, :, 0].any(1), "P at right border": P[:, :, -1].any(1),
        "cch > 1": o["cch"] > 1, "rpc > 1": o["rpc"] > 1, "span crosses a band": o["bands"] > 1,
    }
    return B, int(seen.sum()), {k: int((v & seen).sum()) for k, v in cls.items()}


_counts = {}


def run_camera(name):
    """the properties on every size for one camera, once per session: (samples, samples with non-empty P, class counts)"""
    if name not in _counts:
        index = [c[0] for c in CAMERAS].index(name)
        _, which, x, y = CAMERAS[index]
        cam = rh.camera(which, x, y)
        zlo, zhi = DEPTH.get(name, (0.1, 4.0))
        total, seen, classes = 0, 0, dict.fromkeys(CLASSES, 0)
        for si, (h, w) in enumerate(SIZES):
            rng = np.random.RandomState(1000 * (1 + index) + si)
            n, s, c = check_batch(sample_prims(rng, cam, zlo, zhi, N_SAMPLES[(h, w)]), cam, h, w, name)
            total, seen = total + n, seen + s
            for k in CLASSES:
                classes[k] += c[k]
        _counts[name] = (total, seen, classes)
    return _counts[name]


@pytest.mark.parametrize("name", [c[0] for c in CAMERAS])
def test_footprints_cover_every_hit_pixel(name):
    total, seen, classes = run_camera(name)
    print("{}: {} samples, {} with non-empty P; {}".format(name, total, seen, classes))


def test_sampler_reaches_every_class():
    """Conditions, not measurements: the properties above were checked on visible primitives of every branch."""
    runs = [run_camera(c[0]) for c in CAMERAS]
    total, seen = sum(v[0] for v in runs), sum(v[1] for v in runs)
    classes = {k: sum(v[2][k] for v in runs) for k in CLASSES}
    print("samples {}, with non-empty P {} ({:.1f} %)".format(total, seen, 100.0 * seen / total))
    for k in CLASSES:
        print("  {:28s} {}".format(k, classes[k]))
    assert seen >= 0.30 * total
    for k in CLASSES:
        assert classes[k] >= 200, k


def test_tile_mask_table_holds_every_band():
    """raster_tiles_k keeps one mask per 8x8 tile of a band in kTilePixels / 64 words: true at every width, also those that are no
    multiple of 8 (the tiles of the last column are padded)."""
    cam = rh.camera(rh.MOBILE_FPV, 2.0, 2.0)
    p = rh.prim(rh.BOX, (2.0, 2.0, 0.075), (0.325, 0.1, 0.075))[None]
    for h, w in [(224, 38), (300, 12), (224, 224), (16, 1024), (1024, 9), (700, 1017)]:
        o = rh.footprints(p, cam, h, w)
        assert o["tile_mask_overflow"][0] == 0, (h, w)
        assert not (o["P"] & ~o["Ft"]).any()


def random_scene(rng, cam, zlo, zhi, nmov, ties):
    """plane + table-like static box + nmov moving primitives; with ties: exact duplicates (the lower index must win) and boxes whose
    top face lies in the static box's top face (the static one must win)"""
    tan = float(cam[12])
    centre = world(cam, 0.0, 0.0, 0.5 * (zlo + zhi))
    static = [rh.prim(rh.PLANE, (0, 0, centre[2] - 0.6), (0, 0, 0)),
              rh.prim(rh.BOX, (centre[0], centre[1], centre[2] - 0.3), (0.6, 0.5, 0.025))]
    mov = list(sample_prims(rng, cam, zlo, zhi, 60)[rng.permutation(60)[:nmov]])
    if ties:
        for i in range(0, nmov - 1, 4):
            mov[i + 1] = mov[i].copy()
        top = float(static[1][6]) + 0.025
        for i in range(2, nmov, 6):
            hz = rng.uniform(0.01, 0.05)
            mov[i] = rh.prim(rh.BOX, (centre[0] + rng.uniform(-0.5, 0.5), centre[1] + rng.uniform(-0.4, 0.4), np.float32(top) - np.float32(hz)),
                             (rng.uniform(0.02, 0.2), rng.uniform(0.02, 0.2), hz))
    return np.stack(static + mov), 2


@pytest.mark.parametrize("hw", [(64, 64), (50, 38), (16, 1024), (300, 12), (8, 8)])
def test_scene_winner_is_the_same_in_object_order_and_per_pixel(hw):
    """Multi-primitive scenes of up to kMaxPrims primitives: the span walk with its min on (t, primitive, code) from the static
    depth, and the tile path, pick the primitive and face the full per-pixel z-test picks — ties go to the lower index, static
    scenery wins against an equal t."""
    kmax = rh.constants()["max_prims"]
    assert kmax == 28
    rng = np.random.RandomState(7 + hw[0])
    moving_won = tie_pixels = 0
    for name, which, x, y in CAMERAS[:4]:
        cam = rh.camera(which, x, y)
        zlo, zhi = DEPTH.get(name, (0.1, 4.0))
        for rep in range(3):
            nmov = kmax - 2 if rep == 0 else int(rng.randint(1, kmax - 1))
            prims, nstatic = random_scene(rng, cam, zlo, zhi, nmov, ties=rep != 1)
            full, walk, tiles = rh.scene(prims, nstatic, cam, hw[0], hw[1])
            assert (full >= -1).all()
            bad = full != walk
            assert not bad.any(), "{} {}: object order differs at {} pixels, first {} (full {}, walk {})".format(
                name, hw, int(bad.sum()), np.argwhere(bad)[0], full[bad][0], walk[bad][0])
            assert np.array_equal(full, tiles), "{} {}: tile path differs".format(name, hw)
            moving_won += int(((full >> 3) >= nstatic).sum())
            # pixels whose winner has an exact duplicate right behind it in the list: the tie was really played
            k = full >> 3
            dup = np.array([i + 1 < len(prims) and np.array_equal(prims[i], prims[i + 1]) for i in range(len(prims))])
            tie_pixels += int((dup[np.maximum(k, 0)] & (k >= nstatic)).sum())
    assert moving_won > 0 and tie_pixels > 0
