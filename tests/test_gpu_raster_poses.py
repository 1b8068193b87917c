"""GPU parity of the rasteriser against oracle/raster_oracle.c in poses no rollout reaches: the state is WRITTEN (set_state), not
stepped to, so that the culling footprints of raster.hip meet joint limits, stretched and folded arms, primitives across every image
border, near and behind the cameras, and the robot against the arena walls.  The oracle ray-tests every primitive at every pixel; a
footprint that under-covers shows as differing bytes.  (tests/test_raster_footprint_cpu.py holds the footprints themselves to the
exact test, primitive by primitive, on the host.)"""
import numpy as np
import pytest

import raster_hostcheck as rh
from oracle import raster_clib
from srlhip import _lib
from test_gpu_raster import assert_images_equal, gq, kuka_state, mobile_state

pytestmark = pytest.mark.gpu

N = 64
BUTTON_X, BUTTON_Y = (0.35, 0.65), (-0.3, 0.3)          # drawn range of the button (random_target): 0.5 +- 0.15, 0 +- 0.3
BUTTON2_X, BUTTON2_Y = (0.35, 0.65), (-0.3, -0.125)     # second button of Kuka2ButtonGymEnv: 0.5 +- 0.15, -0.125 - 0.175 * [0, 1]
TABLE_TOP = -0.195


def joint_limits():
    """lower / upper of the 12 DoFs of the baked full model (srlhip_kuka_tree_model: 33 doubles per joint after nd; lower > upper = none)"""
    t = _lib.kuka_tree_default_model()
    j = t[1:1 + 33 * 12].reshape(12, 33)
    return j[:, 16].copy(), j[:, 17].copy()


def camera_azimuth(cam):
    """the angle about z of the horizontal direction from the robot base towards the camera's eye"""
    return float(np.arctan2(cam[1] - 0.0, cam[0] - 0.0))


def kuka_poses(h, rng):
    """q [7][N], gripper q [5][N]: the listed poses first, uniform inside the limits after them"""
    lo, hi = joint_limits()
    assert (lo[:7] < hi[:7]).all()
    rest = h.get_state(_lib.F_KUKA_Q)[:, 0]
    q = rng.uniform(lo[:7, None], hi[:7, None], (7, N))
    g = h.get_state(_lib.F_KUKA_GRIPPER_Q).copy()
    glo = np.where(lo[7:] < hi[7:], lo[7:], -0.4)
    ghi = np.where(lo[7:] < hi[7:], hi[7:], 0.4)
    e = 0
    for i in range(7):                                    # every arm joint at its lower and at its upper limit, the others at rest
        for lim in (lo[i], hi[i]):
            q[:, e] = rest
            q[i, e] = lim
            e += 1
    for which in (rh.KUKA_CAM0, rh.KUKA_CAM1):            # stretched towards and away from each camera, horizontal and raised
        az = camera_azimuth(rh.camera(which))
        for turn, lift in ((0.0, np.pi / 2), (np.pi, np.pi / 2), (0.0, 1.0), (0.0, -np.pi / 2)):
            q[:, e] = 0.0
            q[0, e] = np.clip((az + turn + np.pi) % (2 * np.pi) - np.pi, lo[0], hi[0])
            q[1, e] = np.clip(lift, lo[1], hi[1])
            e += 1
    q[:, e] = 0.0                                          # straight up
    e += 1
    for sgn in (1.0, -1.0):                                # folded onto the table
        q[:, e] = 0.0
        q[1, e], q[3, e], q[5, e] = sgn * hi[1], sgn * lo[3], sgn * hi[5]
        e += 1
    g[:, e] = glo                                          # fingers at one end of their ranges, then the other, then mixed
    g[:, e + 1] = ghi
    g[:, e + 2] = np.where(np.arange(5) % 2 == 0, glo, ghi)
    g[:, e + 3] = np.where(np.arange(5) % 2 == 0, ghi, glo)
    e += 4
    assert e <= N - 8
    g[:, e:] = rng.uniform(glo[:, None], ghi[:, None], (5, N - e))
    return q, g


def corners_then_uniform(rng, xr, yr):
    x, y = rng.uniform(*xr, N), rng.uniform(*yr, N)
    for e, (cx, cy) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)] * 2):
        x[e], y[e] = xr[cx], yr[cy]
    return x, y


def write_button(h, x, y):
    """the button is drawn at BUTTON_XY; BUTTON_POS (what the reward and the oracle call's state read) moves with it"""
    h.set_state(_lib.F_KUKA_BUTTON_XY, np.stack([x, y]))
    bp = h.get_state(_lib.F_KUKA_BUTTON_POS)
    bp[0], bp[1] = x, y
    h.set_state(_lib.F_KUKA_BUTTON_POS, bp)


def kuka_handle(kind, hw, multi_view, seed0):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.seed0, cfg.random_target, cfg.multi_view = N, seed0, 1, multi_view
    cfg.obs_mode, cfg.img_h, cfg.img_w = _lib.OBS_RAW_PIXELS, hw[0], hw[1]
    return _lib.Handle(cfg)


def assert_drawn(img, reset_img):
    assert (img != reset_img).reshape(N, -1).any(1).sum() >= 1, "the written state was not drawn"


@pytest.mark.parametrize("hw", [(64, 64), (50, 38), (16, 1024), (300, 12)])
def test_kuka_written_poses_match_oracle(hw):
    h = kuka_handle(_lib.ENV_KUKA_BUTTON, hw, 1, 11)
    obs0 = h.reset()
    rng = np.random.RandomState(hw[0])
    q, g = kuka_poses(h, rng)
    h.set_state(_lib.F_KUKA_Q, q)
    h.set_state(_lib.F_KUKA_GRIPPER_Q, g)
    write_button(h, *corners_then_uniform(rng, BUTTON_X, BUTTON_Y))
    img = h.render()
    st = kuka_state(h)
    assert np.array_equal(st[:, :7], q.T) and np.array_equal(gq(h), g.T)
    assert_drawn(img, obs0)
    assert_images_equal(img, raster_clib.render(4, st, hw[0], hw[1], 1, gripper_q=gq(h)))
    h.close()


def test_two_button_written_poses_match_oracle():
    h = kuka_handle(_lib.ENV_KUKA_2BUTTON, (64, 64), 1, 12)
    obs0 = h.reset()
    rng = np.random.RandomState(5)
    q, g = kuka_poses(h, rng)
    h.set_state(_lib.F_KUKA_Q, q)
    h.set_state(_lib.F_KUKA_GRIPPER_Q, g)
    x2, y2 = corners_then_uniform(rng, BUTTON2_X, BUTTON2_Y)
    h.set_state(_lib.F_KUKA_BUTTON2_XY, np.stack([x2, y2]))
    write_button(h, *corners_then_uniform(rng, BUTTON_X, (0.0, 0.3)))
    img = h.render()
    st = np.concatenate([kuka_state(h), h.get_state(_lib.F_KUKA_BUTTON2_Q)[0][:, None], h.get_state(_lib.F_KUKA_BUTTON2_XY).T], axis=1)
    assert np.array_equal(st[:, 11], x2) and np.array_equal(st[:, 12], y2)
    assert_drawn(img, obs0)
    assert_images_equal(img, raster_clib.render(6, st, 64, 64, 1, gripper_q=gq(h)))
    h.close()


def body_poses(h, rng):
    """positions [11][3][N] of the ten distractors and the ball (index 10), by env % 8: table edges, touching each other, under the
    gripper, far off-screen, close in front of camera 0 / camera 1, the ball behind camera 0, spread over the table"""
    cams = [rh.camera(rh.KUKA_CAM0).astype(np.float64), rh.camera(rh.KUKA_CAM1).astype(np.float64)]
    grip = h.get_state(_lib.F_KUKA_GRIPPER)
    pos = np.zeros((11, 3, N))
    for e in range(N):
        spread = np.stack([rng.uniform(-0.25, 1.25, 11), rng.uniform(-0.5, 0.5, 11), np.full(11, TABLE_TOP + 0.03)], 1)
        kind = e % 8
        if kind == 0:
            t = (np.arange(11) + rng.rand()) / 11.0 * 4.0
            side, u = t.astype(int), t % 1.0
            x = np.select([side == 0, side == 1, side == 2, side == 3], [-0.25 + 1.5 * u, 1.25, 1.25 - 1.5 * u, -0.25])
            y = np.select([side == 0, side == 1, side == 2, side == 3], [-0.5, -0.5 + u, 0.5, 0.5 - u])
            p = np.stack([x, y, np.full(11, TABLE_TOP + 0.03)], 1)
        elif kind == 1:
            p = np.stack([0.3 + 0.05 * (np.arange(11) % 4), -0.1 + 0.05 * (np.arange(11) // 4), np.full(11, TABLE_TOP + 0.025)], 1)
        elif kind == 2:
            p = np.stack([grip[0, e] + rng.uniform(-0.03, 0.03, 11), grip[1, e] + rng.uniform(-0.03, 0.03, 11), np.full(11, TABLE_TOP + 0.03)], 1)
        elif kind == 3:
            p = np.stack([30.0 + np.arange(11), -40.0 - np.arange(11), 5.0 + np.arange(11)], 1)
        elif kind in (4, 5):
            c = cams[kind - 4]
            d = 0.1 + 0.03 * (10 - np.arange(11))                      # the ball (always present) nearest
            p = c[0:3] + d[:, None] * c[3:6] + rng.uniform(-0.5, 0.5, (11, 1)) * d[:, None] * c[6:9] + rng.uniform(-0.5, 0.5, (11, 1)) * d[:, None] * c[9:12]
        elif kind == 6:
            p = spread
            p[10] = cams[0][0:3] - 0.3 * cams[0][3:6]
        else:
            p = spread
        pos[:, :, e] = p
    return pos


def test_rand_button_written_bodies_match_oracle():
    h = kuka_handle(_lib.ENV_KUKA_RAND, (64, 64), 1, 13)
    obs0 = h.reset()
    rng = np.random.RandomState(6)
    q, g = kuka_poses(h, rng)
    h.set_state(_lib.F_KUKA_Q, q)
    h.set_state(_lib.F_KUKA_GRIPPER_Q, g)
    bodies = h.get_state(_lib.F_KUKA_BODIES).reshape(11, 6, N)
    pos = body_poses(h, rng)
    bodies[:, :3, :] = pos
    h.set_state(_lib.F_KUKA_BODIES, bodies.reshape(66, N))
    img = h.render()
    st = np.concatenate([kuka_state(h), h.get_state(_lib.F_KUKA_OBJECTS).T, h.get_state(_lib.F_KUKA_BODIES).T], axis=1)
    assert np.array_equal(st[:, 40:].reshape(N, 11, 6)[:, :, :3], pos.transpose(2, 0, 1))
    assert_drawn(img, obs0)
    assert_images_equal(img, raster_clib.render(8, st, 64, 64, 1, gripper_q=gq(h)))
    # the ball of the envs that hold it close to a camera fills a good part of that camera's image: it really is large there
    plain = raster_clib.render(4, st[:, :10], 64, 64, 1, gripper_q=gq(h))
    changed = (img != plain).any(-1).reshape(N, -1).mean(1)
    assert changed[4::8].min() > 0.02 and changed[5::8].min() > 0.02
    h.close()


def mobile_poses(kind, rng):
    """x y tx ty t2x t2y [6][N]: robot in the arena corners, against each wall and pushed into it, on top of the target, targets in
    the corners; uniform over (and a little beyond) the arena after them"""
    y_lo, y_hi = (0.0, 0.0) if kind == 1 else (0.0, 4.0)
    s = np.stack([rng.uniform(-0.2, 4.2, N), rng.uniform(y_lo - 0.2, y_hi + 0.2, N), rng.uniform(0.0, 4.0, N), rng.uniform(y_lo, y_hi, N),
                  rng.uniform(0.0, 4.0, N), rng.uniform(y_lo, y_hi, N)])
    listed = [(0.375, 0.15), (0.375, 3.85), (3.625, 0.15), (3.625, 3.85),              # corners (robot half extents 0.325 x 0.1, walls 0.05)
              (0.375, 2.0), (3.625, 2.0), (2.0, 0.15), (2.0, 3.85),                      # against each wall
              (0.1, 2.0), (3.95, 1.0), (1.0, 0.0), (3.0, 4.0), (0.02, 0.02)]            # pushed into the walls: the fpv eye within 0.05 of a wall face
    e = 0
    for x, y in listed:
        s[0, e], s[1, e] = x, min(max(y, y_lo), y_hi) if kind == 1 else y
        e += 1
    for k in range(4):                                                                   # robot on top of the target / of the second target
        s[0, e], s[1, e] = s[2 + 2 * (k % 2), e], s[3 + 2 * (k % 2), e]
        e += 1
    for cx, cy in [(0.0, y_lo), (0.0, y_hi), (4.0, y_lo), (4.0, y_hi)]:                  # targets in the arena corners
        s[2, e], s[3, e], s[4, e], s[5, e] = cx, cy, 4.0 - cx, cy
        e += 1
    return s


MOBILE_FIELDS = ("F_POS_X", "F_POS_Y", "F_TARGET_X", "F_TARGET_Y", "F_TARGET2_X", "F_TARGET2_Y")


def mobile_case(kind, fpv, hw):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.seed0, cfg.random_target, cfg.multi_view = N, 14, 1, fpv
    cfg.obs_mode, cfg.img_h, cfg.img_w = _lib.OBS_RAW_PIXELS, hw[0], hw[1]
    h = _lib.Handle(cfg)
    obs0 = h.reset()
    s = mobile_poses(kind, np.random.RandomState(10 * kind + fpv))
    for name, plane in zip(MOBILE_FIELDS, s):
        h.set_state(getattr(_lib, name), plane)
    img = h.render()
    st = mobile_state(h)
    assert np.array_equal(st, s.T)
    assert_drawn(img, obs0)
    assert_images_equal(img, raster_clib.render(kind, st, hw[0], hw[1], multi_view=bool(fpv)))
    h.close()


@pytest.mark.parametrize("hw", [(64, 64), (50, 38)])
@pytest.mark.parametrize("fpv", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_mobile_written_poses_match_oracle(kind, fpv, hw):
    mobile_case(kind, fpv, hw)


def test_mobile_fpv_tall_frame_of_odd_width_matches_oracle():
    """(224, 38): 28 tile rows of 5 tiles — more 8x8 tiles than a band of the tile path may hold when the band's rows are counted
    from the width instead of from whole tiles (tests/test_raster_footprint_cpu.py::test_tile_mask_table_holds_every_band)"""
    mobile_case(0, 1, (224, 38))
