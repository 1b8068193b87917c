"""GPU: srlhip_jpeg_encode / srlhip_render_jpeg / dataset_generator --device-jpeg.  The kernels of csrc/jpeg.hip are held byte for
byte, offsets included, to tests/jpeg_ref.py (the numpy restatement of the contract in include/srlhip.h); every shape is the smallest
that still reaches its code path."""
import filecmp
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref
from srlhip import _lib
from test_jpeg_cpu import MARGIN_DB, NOISE_SEED

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(kind, h, w, seed, q):
    key = (kind, h, w, seed, q)
    if key not in _REF:
        _REF[key] = jpeg_ref.encode(jpeg_ref.frame(kind, h, w, seed=seed), q)
    return _REF[key]


def _encode(frames, q, cap, sentinel=0xA5, tail=64):
    """srlhip_jpeg_encode on uint8 [n][h][w][c] -> (rc, blob with `tail` extra sentinel bytes, offsets, overflow) as host arrays"""
    n, h, w, c = frames.shape
    ns = n * c // 3
    img = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    blob = torch.full((ns * cap + tail,), sentinel, dtype=torch.uint8, device="cuda")
    offsets = torch.full((ns + 1,), -7, dtype=torch.int64, device="cuda")
    overflow = torch.full((ns,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.jpeg_encode(img.data_ptr(), n, h, w, c, q, blob.data_ptr(), cap, offsets.data_ptr(), overflow.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, blob.cpu().numpy(), offsets.cpu().numpy(), overflow.cpu().numpy()


# (h, w, c, n): smaller than one MCU; whole MCUs; padding on both sides, 2 x 3 MCUs; one stream more than a round number of workgroups
# and waves; 196 MCUs per stream (lanes stride over MCUs, a multi-wave scan) and two views per frame
@pytest.mark.parametrize("h,w,c,n", [(8, 8, 3, 1), (16, 16, 3, 3), (24, 40, 3, 2), (64, 64, 3, 65), (224, 224, 6, 2)])
def test_encode_equals_the_reference_byte_for_byte(h, w, c, n):
    views = c // 3
    ns = n * views
    # stream s shows content s mod 4 (two seeds in turn), so that every call mixes the four kinds; n = 1 takes them one call each
    rounds = range(4) if ns < 4 else (0,)
    for r in rounds:
        spec = [(jpeg_ref.KINDS[(s + r) % 4], NOISE_SEED + (s // 4) % 2) for s in range(ns)]
        streams = [jpeg_ref.frame(kind, h, w, seed=seed) for kind, seed in spec]
        frames = np.stack([np.concatenate(streams[views * i:views * (i + 1)], axis=2) for i in range(n)])
        for q in jpeg_ref.QUALITIES:
            want = [_ref(kind, h, w, seed, q) for kind, seed in spec]
            cap = 1024 + h * w * 3
            rc, blob, offsets, overflow = _encode(frames, q, cap)
            assert rc == 0 and not overflow.any()
            assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist(), (q, r)
            for s in range(ns):
                assert blob[offsets[s]:offsets[s + 1]].tobytes() == want[s], (q, r, s, spec[s])
            assert (blob[offsets[ns]:] == 0xA5).all()                 # nothing behind the packed streams, up to and past the blob's end


def test_streams_that_do_not_fit_are_flagged_and_write_nothing():
    h = w = 64
    frames = np.stack([jpeg_ref.frame("noise", h, w, seed=NOISE_SEED + i) for i in range(5)])
    cap = _lib.jpeg_header_bytes() + 64
    rc, blob, offsets, overflow = _encode(frames, 95, cap)
    assert rc == 0
    assert overflow.tolist() == [1] * 5 and offsets.tolist() == [0] * 6
    assert (blob == 0xA5).all()                                       # every slot, the bytes after each slot and after the blob


def test_mixed_call_where_only_the_flat_frames_fit():
    h = w = 64
    kinds = ["flat", "noise", "noise", "flat", "noise", "flat"]
    frames = np.stack([jpeg_ref.frame(k, h, w, seed=NOISE_SEED + i) for i, k in enumerate(kinds)])
    want = [jpeg_ref.encode(f, 95) for f in frames]
    cap = max(len(x) for x, k in zip(want, kinds) if k == "flat")
    assert cap < min(len(x) for x, k in zip(want, kinds) if k == "noise")
    rc, blob, offsets, overflow = _encode(frames, 95, cap)
    assert rc == 0 and overflow.tolist() == [int(k == "noise") for k in kinds]
    at = 0
    for s, k in enumerate(kinds):
        assert offsets[s] == at
        if k == "flat":
            assert blob[at:at + len(want[s])].tobytes() == want[s]
            at += len(want[s])
    assert offsets[-1] == at and (blob[at:] == 0xA5).all()


def test_encode_refuses_bad_arguments():
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    off, ovf = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    call = lambda h, w, c, q: _lib.jpeg_encode(buf.data_ptr(), 1, h, w, c, q, buf.data_ptr() + 32768, 8192, off.data_ptr(), ovf.data_ptr())   # noqa: E731
    for bad in ((16, 16, 3, 0), (16, 16, 3, 101), (16, 16, 4, 95), (7, 16, 3, 95), (16, 1025, 3, 95)):
        assert call(*bad) == -22, bad
    assert call(16, 16, 3, 95) == 0
    torch.cuda.synchronize()


def _handle(kind, multi_view=0, rng=_lib.RNG_MT19937):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.seed0, cfg.rng_mode, cfg.auto_reset = 8, 5, rng, 1
    cfg.img_h = cfg.img_w = 64
    cfg.multi_view = multi_view
    return _lib.Handle(cfg)


def _check_render_jpeg(h):
    frames = h.render()
    views = frames.shape[3] // 3
    got = h.render_jpeg(quality=95)
    assert len(got) == h.num_envs * views
    for i in range(h.num_envs):
        for v in range(views):
            assert got[views * i + v] == jpeg_ref.encode(frames[i, :, :, 3 * v:3 * v + 3], 95), (i, v)


@pytest.mark.parametrize("kind,multi_view", [(_lib.ENV_KUKA_BUTTON, 0), (_lib.ENV_KUKA_BUTTON, 1), (_lib.ENV_MOBILE, 0)])
def test_render_jpeg_equals_the_reference_encode_of_render(kind, multi_view):
    h = _handle(kind, multi_view)
    h.reset()
    _check_render_jpeg(h)
    acts = np.random.RandomState(0).randint(h.num_actions, size=(3, h.num_envs)).astype(np.int32)
    for t in range(3):
        h.step(acts[t])
    _check_render_jpeg(h)
    # a slot too small for any stream: every one comes back as None
    assert h.render_jpeg(quality=95, cap_per_stream=_lib.jpeg_header_bytes() + 8) == [None] * (h.num_envs * (2 if multi_view else 1))
    with pytest.raises(_lib.SrlHipError):
        h.render_jpeg(quality=0)
    h.step_async(acts[0])
    with pytest.raises(_lib.SrlHipError):                                 # EINVAL while a step is pending
        h.render_jpeg()
    h.step_wait()
    _check_render_jpeg(h)
    h.close()


def test_render_jpeg_parks_a_resident_kernel_which_steps_on_afterwards():
    a, b = _handle(_lib.ENV_MOBILE, rng=_lib.RNG_PHILOX), _handle(_lib.ENV_MOBILE, rng=_lib.RNG_PHILOX)
    a.set_persistent(True)
    a.reset(); b.reset()
    acts = np.random.RandomState(1).randint(4, size=(6, 8)).astype(np.int32)
    for t in range(6):
        x, y = a.step(acts[t]), b.step(acts[t])
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), t
        if t == 2:
            assert a.render_jpeg() == b.render_jpeg()
            _check_render_jpeg(a)
    a.close(); b.close()


def _psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_dataset_generator_with_device_jpeg_writes_the_same_dataset(tmp_path):
    from environments import dataset_generator as dg
    root = str(tmp_path) + "/"
    common = ["--env", "MobileRobotGymEnv-v0", "--num-cpu", "4", "--num-episode", "4", "--img-size", "64", "--save-path", root, "--seed", "1"]
    dg.main(common + ["--name", "host"])
    dg.main(common + ["--name", "dev", "--device-jpeg"])

    def tree(name):
        return sorted(os.path.relpath(os.path.join(d, f), root + name) for d, _, fs in os.walk(root + name) for f in fs)
    assert tree("host") == tree("dev") and sum(p.endswith(".jpg") for p in tree("dev")) > 8
    for fname in ("preprocessed_data.npz", "ground_truth.npz"):
        with np.load(root + "host/" + fname) as x, np.load(root + "dev/" + fname) as y:
            assert x.files == y.files
            for k in x.files:
                u, v = x[k], y[k]
                if k == "images_path":
                    v = np.array([p.replace("dev/", "host/", 1) for p in v])
                assert np.array_equal(u, v), (fname, k)
    for cfg_file in ("dataset_config.json", "env_globals.json"):
        assert filecmp.cmp(root + "host/" + cfg_file, root + "dev/" + cfg_file, shallow=False)
    # every frame of the device run decodes to its Pillow twin: against the twin's decode, two lossy encodes of one frame differ by
    # about their own distance to the frame (> 40 dB at quality 95 on these frames), and the device stream's distance to the FRAME may
    # exceed Pillow's by the CPU test's margin at most — the frame itself is not on disk, so the decodes are compared with each other
    worst = 99.0
    for p in tree("dev"):
        if p.endswith(".jpg"):
            x, y = Image.open(root + "host/" + p), Image.open(root + "dev/" + p)
            x.load(); y.load()
            assert x.size == y.size == (64, 64) and y.mode == "RGB"
            worst = min(worst, _psnr(x, y))
    print("worst PSNR between the device stream's decode and its Pillow twin's: {:.2f} dB".format(worst))
    assert worst >= 40.0 - MARGIN_DB, worst
