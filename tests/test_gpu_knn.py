"""srlhip_knn on the device against tests/knn_ref.py (the contract restated in numpy with libm's fma): the neighbours equal, the distances
and the error terms equal as bit patterns, for every split of the candidates; and state_representation.evaluate on top of it."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "robotics-rl-srl_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import knn_ref as ref  # noqa: E402
from srlhip import _lib  # noqa: E402

SPLITS = (0, 1, 7)
IDX_SENTINEL, DIST_SENTINEL = -77, -12345.5


def run_device(x, k, queries=None, gt=None, split=0, stream=None, view_offset=False):
    """-> (idx, dist, err or None) as numpy, the planes prefilled with sentinels"""
    N, S = x.shape
    xt = torch.from_numpy(np.array(x))                         # (a copy: the shared cases are read-only)
    if view_offset:                                             # a float32 base pointer that is 4-byte but not 8- or 16-byte aligned
        buf = torch.empty(N * S + 1, dtype=xt.dtype, device="cuda")
        buf[1:].copy_(xt.reshape(-1).cuda())
        xd = buf[1:].view(N, S)
        assert xd.data_ptr() % 8 == 4
    else:
        xd = xt.cuda()
    qd = None if queries is None else torch.from_numpy(np.array(queries, dtype=np.int32)).cuda()
    Q = N if queries is None else len(queries)
    gd = None if gt is None else torch.from_numpy(np.array(gt)).cuda()
    idx = torch.full((Q, k), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    dist = torch.full((Q, k), DIST_SENTINEL, dtype=torch.float64, device="cuda")
    err = None if gt is None else torch.full((Q,), DIST_SENTINEL, dtype=torch.float64, device="cuda")
    work = torch.zeros((_lib.knn_workspace_bytes(N, S, k, Q, split) + 7) // 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib.knn(0, xd.data_ptr(), x.dtype == np.float32, N, S, None if qd is None else qd.data_ptr(), Q, k, None if gd is None else gd.data_ptr(),
             0 if gt is None else gt.shape[1], idx.data_ptr(), dist.data_ptr(), None if err is None else err.data_ptr(), work.data_ptr(),
             split=split, stream=stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), None if err is None else err.cpu().numpy()


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert ref.same_bits(got[1], want[1])
    if len(want) > 2 and want[2] is not None:
        assert ref.same_bits(got[2], want[2])


@pytest.mark.parametrize("content", ref.CONTENTS)
def test_device_equals_the_reference(content):
    """every shape of knn_ref.shapes() x the three query lists x splits 0, 1, 7: idx equal, dist and err bit-equal (so the three splits
    equal each other)"""
    for N, S, k, G in ref.shapes():
        for which in range(3):
            x, gt, queries, want = ref.case(content, N, S, k, G, which)
            for split in SPLITS:
                assert_same(run_device(x, k, queries, gt, split), want)


@pytest.fixture(scope="module")
def larger():
    """N = 1000, S = 32, k = 5, Q = 300: 16 candidate tiles of 64 (several inside one slice), a ragged last tile of 40 rows, two query
    workgroups of 256 with a ragged last wavefront (300 = 4 x 64 + 44)"""
    N, S, k, G = 1000, 32, 5, 3
    queries = np.sort(np.random.RandomState(5).choice(N, 300, replace=False)).astype(np.int32)
    gt = ref.make_ground_truth(N, G)
    cases = {}
    for content in ("grid", "random"):
        x = ref.make_states(content, N, S)
        cases[content] = (x, ref.neighbours(x, k, queries, gt, exact=content == "grid", fast=content == "random"))
    return k, queries, gt, cases


@pytest.mark.parametrize("content", ("grid", "random"))
@pytest.mark.parametrize("split", SPLITS)
def test_larger_case_crosses_tiles_and_wavefronts(larger, content, split):
    k, queries, gt, cases = larger
    x, want = cases[content]
    assert_same(run_device(x, k, queries, gt, split), want)


def test_a_query_does_not_depend_on_its_batch():
    N, S, k = 130, 33, 5
    x, gt = ref.make_states("random", N, S), ref.make_ground_truth(N, 3)
    a, b = 71, 5
    full = run_device(x, k, None, gt)
    for queries in ([a], [a, b], [b, a, a]):
        got = run_device(x, k, np.array(queries, np.int32), gt)
        at = queries.index(a)
        assert np.array_equal(got[0][at], full[0][a]) and ref.same_bits(got[1][at], full[1][a]) and ref.same_bits(got[2][at:at + 1], full[2][a:a + 1])


def test_results_land_on_the_callers_stream():
    """The call inside a stream capture (an env handle's own stream and srlhip_graph_begin / _end): nothing runs until the graph is
    launched, and a replay after the states changed gives the new states' planes — lists start in kernels, nothing is preset by the host."""
    from srlhip.pixel_env import RawPixelVecEnv
    N, S, k, G = 300, 8, 5, 3
    first, second = ref.make_states("random", N, S, seed=1), ref.make_states("random", N, S, seed=2)
    gt = ref.make_ground_truth(N, G)
    env = RawPixelVecEnv("MobileRobotGymEnv-v0", 8, seed=1)
    env.reset()
    x, gd = torch.from_numpy(first).cuda(), torch.from_numpy(gt).cuda()
    idx = torch.full((N, k), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    dist = torch.full((N, k), DIST_SENTINEL, dtype=torch.float64, device="cuda")
    err = torch.full((N,), DIST_SENTINEL, dtype=torch.float64, device="cuda")
    work = torch.zeros(_lib.knn_workspace_bytes(N, S, k, N, 3) // 8 + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    env.h.graph_begin()
    _lib.knn(0, x.data_ptr(), False, N, S, None, N, k, gd.data_ptr(), G, idx.data_ptr(), dist.data_ptr(), err.data_ptr(), work.data_ptr(),
             split=3, stream=env._stream_ptr)
    g = env.h.graph_end()
    torch.cuda.synchronize()
    assert (idx == IDX_SENTINEL).all() and (dist == DIST_SENTINEL).all() and (err == DIST_SENTINEL).all()      # captured, not run
    for states in (first, second):
        x.copy_(torch.from_numpy(states))
        torch.cuda.synchronize()
        env.h.graph_launch(g)
        env.h.sync()
        assert_same((idx.cpu().numpy(), dist.cpu().numpy(), err.cpu().numpy()), ref.neighbours(states, k, None, gt))
    env.h.graph_destroy(g)
    env.close()


def test_unaligned_float32_states():
    N, S, k = 65, 33, 5
    x, gt = ref.make_states("f32", N, S), ref.make_ground_truth(N, 3)
    want = ref.neighbours(x, k, None, gt)
    for split in SPLITS:
        assert_same(run_device(x, k, None, gt, split, view_offset=True), want)


def test_out_of_range_query_on_the_device():
    N, S, k = 130, 3, 5
    x, gt = ref.make_states("random", N, S), ref.make_ground_truth(N, 3)
    queries = np.array([4, N, 9, -1, 2 ** 31 - 1, 129], np.int32)
    good = np.array([0, 2, 5])
    want = ref.neighbours(x, k, queries[good], gt)
    for split in SPLITS:
        idx, dist, err = run_device(x, k, queries, gt, split)
        assert_same((idx[good], dist[good], err[good]), want)
        for bad in (1, 3, 4):
            assert (idx[bad] == -1).all() and np.isposinf(dist[bad]).all() and err[bad] == 0.0


def test_refusals_leave_outputs_and_workspace_untouched():
    lib = _lib.load()
    N, S, k, G = 20, 4, 3, 2
    x = torch.from_numpy(ref.make_states("random", N, S)).cuda()
    gt = torch.from_numpy(ref.make_ground_truth(N, G)).cuda()
    idx = torch.full((N, 33), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    dist = torch.full((N, 33), DIST_SENTINEL, dtype=torch.float64, device="cuda")
    err = torch.full((N,), DIST_SENTINEL, dtype=torch.float64, device="cuda")
    work = torch.full((4096,), 0x5a5a, dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(n=N, s=S, kk=k, g=G, split=0, states=x, gtp=gt, errp=err, idxp=idx, distp=dist, workp=work):
        return lib.srlhip_knn(0, p(states), 0, n, s, None, n, kk, p(gtp), g, split, p(idxp), p(distp), p(errp), p(workp), None)

    cases = [(dict(s=65), -95, "64"), (dict(kk=33), -95, "32"), (dict(kk=N), -95, "n - 1"),
             (dict(n=1), -95, "2..2^20"), (dict(g=33), -95, "32"), (dict(gtp=None), -22, "both"), (dict(errp=None), -22, "both"),
             (dict(split=-1), -22, "split"), (dict(states=None), -22, "null"), (dict(idxp=None), -22, "null"), (dict(workp=None), -22, "workspace")]
    for kwargs, code, word in cases:
        assert call(**kwargs) == code, kwargs
        assert word in lib.srlhip_knn_last_error().decode(), (kwargs, lib.srlhip_knn_last_error())
    torch.cuda.synchronize()
    assert (idx == IDX_SENTINEL).all() and (dist == DIST_SENTINEL).all() and (err == DIST_SENTINEL).all() and (work == 0x5a5a).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (idx.view(-1)[:N * k] != IDX_SENTINEL).all()


class _Recording(object):
    """a RawPixelVecEnv that notes the robot's position after every reset and step: the ground truth of the frames collect_frames takes"""

    def __init__(self, env):
        self._env, self.positions = env, []

    def __getattr__(self, name):
        return getattr(self._env, name)

    def _note(self):
        self.positions.append(np.stack([self._env.h.get_state(_lib.F_POS_X), self._env.h.get_state(_lib.F_POS_Y)], axis=1).astype(np.float64))

    def reset(self):
        out = self._env.reset()
        self._note()
        return out

    def step(self, actions):
        out = self._env.step(actions)
        self._note()
        return out


def test_evaluate_model_end_to_end_on_the_device(tmp_path):
    from srlhip.pixel_env import RawPixelVecEnv
    from state_representation import evaluate, pca_fit
    env = _Recording(RawPixelVecEnv("MobileRobotGymEnv-v0", 16, seed=3, img_shape=(64, 64)))
    frames = pca_fit.collect_frames(env, 12, seed=0)
    gt = np.concatenate(env.positions).reshape(len(frames), -1)
    env.close()
    model = pca_fit.fit_pca(frames, 4, backend="hip")
    path = model.save(str(tmp_path))
    states = torch.from_numpy(model.transform(frames.cpu().numpy())).cuda()
    on_device = evaluate.knn_mse(states, gt, k=5, backend="hip")
    on_host = evaluate.knn_mse(states, gt, k=5, backend="host")
    assert np.array_equal(on_device["idx"], on_host["idx"]) and ref.same_bits(on_device["err"], on_host["err"])
    assert ref.same_bits([on_device["knn_mse"]], [on_host["knn_mse"]])
    floor = evaluate.knn_mse(gt, gt, k=5, backend="hip")
    assert floor["knn_mse"] <= on_device["knn_mse"]
    # the whole tool on the same frames: the files, their keys, and the floor below the model's score
    data = tmp_path / "data"
    data.mkdir()
    names = np.array(["data/record_{:03d}/frame{:06d}".format(n // 16, n % 16) for n in range(len(frames))])
    np.savez(str(data / "ground_truth.npz"), ground_truth_states=gt, images_path=names)
    out = evaluate.evaluate_model(str(data), path, k=5, knn_samples=100, backend="hip", log_folder=str(tmp_path / "out"), frames=frames,
                                  indices=np.arange(len(frames)))
    assert out["backend"] == "hip" and out["n_queries"] == 100 and out["n_frames"] == len(frames)
    assert out["knn_mse_ground_truth"] <= out["knn_mse"] and len(out["gtc"]) == gt.shape[1]
    saved = np.load(str(tmp_path / "out" / "nearest_neighbours.npz"))
    assert saved["idx"].shape == (100, 5) and np.array_equal(saved["queries"], evaluate.sample_queries(len(frames), 100, 1))
