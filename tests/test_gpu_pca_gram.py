"""GPU: srlhip_pca_gram (csrc/pca_gram.hip) against the exact integer reference (tests/pca_gram_ref.py) at the tile edges, the unaligned
strides and the int32 flush; split and stream behaviour; refusals; and fit_pca on the device against fit_pca on the host twin, bit for bit,
up to the fitted model inside PixelStateVecEnv."""
import ctypes

import numpy as np
import pytest
import torch

import pca_gram_ref as ref
import pca_ref
from srlhip import _lib
from state_representation import pca_fit
from state_representation.models import SRLPCA, loadSRLModel

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF


def _gram(x, split=0, stream=None, n=None, n_features=None):
    """x: uint8 device tensor [N][F] -> (gram, rowsum) numpy, planes prefilled with a sentinel"""
    N, F = x.shape
    gram = torch.full((N, N), SENTINEL, dtype=torch.int64, device="cuda")
    rowsum = torch.full((N,), SENTINEL, dtype=torch.int64, device="cuda")
    _lib.pca_gram(0, x.data_ptr(), N if n is None else n, F if n_features is None else n_features, gram.data_ptr(), rowsum.data_ptr(),
                  split=split, stream=stream or torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gram.cpu().numpy(), rowsum.cpu().numpy()


def _check(x_host, splits=(0, 1, 7)):
    want, want_rows = ref.gram_ref(x_host)
    x = torch.from_numpy(x_host).cuda()
    for split in splits:
        got, rows = _gram(x, split)
        assert np.array_equal(rows, want_rows), (x_host.shape, split)
        assert np.array_equal(got, want), (x_host.shape, split)          # (which makes it symmetric, and the three splits identical)
        assert np.array_equal(got, got.T)


@pytest.mark.parametrize("F", ref.FS)
def test_gram_equals_the_integer_reference(F):
    for N in ref.NS:
        for content in ref.CONTENTS:
            _check(ref.frames(content, N, F))


def test_gram_at_the_reference_frame_size():
    """224 x 224 x 3 = 150528 features: three int32 chunks in one slice (split = 1), and slices that end inside a chunk (7)"""
    N, F = ref.BIG
    for content in ref.CONTENTS:
        _check(ref.frames(content, N, F))


def test_unaligned_base_pointer():
    """frames that start at an odd address: F is a multiple of 16, the base is not — the guarded byte path"""
    N, F = 33, 48
    buf = torch.from_numpy(ref.frames("random", 1, N * F + 3).reshape(-1)).cuda()
    x = buf[3:3 + N * F].view(N, F)
    assert x.data_ptr() % 16 == 3 or x.data_ptr() % 2 == 1
    want, want_rows = ref.gram_ref(x.cpu().numpy())
    got, rows = _gram(x)
    assert np.array_equal(got, want) and np.array_equal(rows, want_rows)


def test_orientation_of_the_tile():
    """frame i is i + 1 in one feature of its own and 0 elsewhere, plus a shared feature holding i + 1: gram[i][j] = (i + 1)(j + 1) off the
    diagonal and 2 (i + 1)^2 on it — asymmetric in the tile's row and column within every row of tiles"""
    N = 70
    x = np.zeros((N, N + 1), np.uint8)
    x[np.arange(N), np.arange(N)] = np.arange(N) + 1
    x[:, N] = np.arange(N) + 1
    _check(x)


def test_results_land_on_the_callers_stream():
    """The call inside a stream capture (an env handle's own stream and srlhip_graph_begin / _end, as PixelStateVecEnv captures its step): a
    synchronisation inside the call would fail the capture, and nothing runs until the graph is launched.  Replayed after the frames
    changed, the graph gives the new frames' planes — zeroes, row sums and tiles are all kernels on the captured stream."""
    from srlhip.pixel_env import RawPixelVecEnv
    N, F = 65, 12288
    first, second = ref.frames("random", N, F, seed=1), ref.frames("random", N, F, seed=2)
    env = RawPixelVecEnv("MobileRobotGymEnv-v0", 8, seed=1)
    env.reset()
    x = torch.from_numpy(first).cuda()
    gram = torch.full((N, N), SENTINEL, dtype=torch.int64, device="cuda")
    rowsum = torch.full((N,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    env.h.graph_begin()
    _lib.pca_gram(0, x.data_ptr(), N, F, gram.data_ptr(), rowsum.data_ptr(), split=0, stream=env._stream_ptr)
    g = env.h.graph_end()
    torch.cuda.synchronize()
    assert (gram == SENTINEL).all() and (rowsum == SENTINEL).all()      # captured, not run
    for frames in (first, second):
        x.copy_(torch.from_numpy(frames))
        torch.cuda.synchronize()
        env.h.graph_launch(g)
        env.h.sync()                                                     # the handle's stream alone
        want, want_rows = ref.gram_ref(frames)
        assert np.array_equal(gram.cpu().numpy(), want) and np.array_equal(rowsum.cpu().numpy(), want_rows)
    env.h.graph_destroy(g)
    env.close()


def test_refusals_leave_the_planes_untouched():
    lib = _lib.load()
    x = torch.from_numpy(ref.frames("random", 4, 16)).cuda()
    gram = torch.full((4, 4), SENTINEL, dtype=torch.int64, device="cuda")
    rowsum = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.srlhip_pca_gram(0, p(x), 0, 16, 0, p(gram), p(rowsum), None) == -95
    assert lib.srlhip_pca_gram(0, p(x), 8193, 16, 0, p(gram), p(rowsum), None) == -95
    assert b"1..8192" in lib.srlhip_pca_gram_last_error()
    assert lib.srlhip_pca_gram(0, p(x), 4, 0, 0, p(gram), p(rowsum), None) == -95
    assert lib.srlhip_pca_gram(0, None, 4, 16, 0, p(gram), p(rowsum), None) == -22
    assert lib.srlhip_pca_gram(0, p(x), 4, 16, 0, None, p(rowsum), None) == -22
    assert lib.srlhip_pca_gram(0, p(x), 4, 16, 0, p(gram), None, None) == -22
    assert lib.srlhip_pca_gram(0, p(x), 4, 16, -1, p(gram), p(rowsum), None) == -22
    with pytest.raises(_lib.SrlHipError):
        _lib.pca_gram(0, x.data_ptr(), 8193, 16, gram.data_ptr(), rowsum.data_ptr())
    torch.cuda.synchronize()
    assert (gram == SENTINEL).all() and (rowsum == SENTINEL).all()
    assert lib.srlhip_pca_gram(0, p(x), 4, 16, 0, p(gram), p(rowsum), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(gram.cpu().numpy(), ref.gram_ref(x.cpu().numpy())[0])


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    """256 frames of 64 x 64 x 3 from a RawPixelVecEnv (64 envs x 4 steps) on the device, and the two fits"""
    from srlhip.pixel_env import RawPixelVecEnv
    env = RawPixelVecEnv("KukaButtonGymEnv-v0", 64, seed=5)
    frames = pca_fit.collect_frames(env, 4, seed=1)
    env.close()
    assert frames.is_cuda and tuple(frames.shape) == (256, 64, 64, 3) and frames.dtype == torch.uint8
    hip = pca_fit.fit_pca(frames, 5, backend="hip")
    host = pca_fit.fit_pca(frames.cpu().numpy(), 5, backend="host")
    return frames, hip, host


def test_fit_on_the_device_equals_the_fit_on_the_host_bit_for_bit(recorded):
    frames, hip, host = recorded
    assert hip.backend == "hip" and host.backend == "host"
    for name in ("mean_", "components_", "explained_variance_", "singular_values_"):
        a, b = getattr(hip, name), getattr(host, name)
        assert a.dtype == np.float64 and pca_ref.same_bits(a, b), name
    assert hip.components_.shape == (5, 64 * 64 * 3) and (np.diff(hip.explained_variance_) <= 0).all()
    assert pca_fit.fit_pca(frames, 5).backend == "hip"                   # auto on device frames


def test_the_saved_model_drives_a_pixel_state_env(recorded, tmp_path):
    from srlhip.pixel_env import PixelStateVecEnv
    _, hip, _ = recorded
    path = hip.save(str(tmp_path))
    model = loadSRLModel(path, cuda=True, img_shape=(64, 64))
    assert isinstance(model, SRLPCA) and model.backend == "hip" and model.state_dim == 5
    env = PixelStateVecEnv("KukaButtonGymEnv-v0", 64, model, seed=9)
    env.reset()
    states = env.step()[0]
    torch.cuda.synchronize()
    w, b = model._w.cpu().numpy(), model._b.cpu().numpy()
    assert pca_ref.same_bits(states.cpu().numpy(), _lib.pca_project_host(w, b, env.images.cpu().numpy(), states_f32=True))
    env.close()


def test_fit_pca_from_env():
    from srlhip.pixel_env import RawPixelVecEnv
    env = RawPixelVecEnv("MobileRobotGymEnv-v0", 32, seed=2)
    model = pca_fit.fit_pca_from_env(env, 3, 4)
    env.close()
    assert model.components_.shape == (4, 64 * 64 * 3) and model.mean_.shape == (64 * 64 * 3,) and model.n_components_ == 4
    assert model.explained_variance_.shape == (4,) and (np.diff(model.explained_variance_) <= 0).all() and (model.explained_variance_ >= 0).all()
    assert model.n_samples_ == 96 and model.whiten is False
