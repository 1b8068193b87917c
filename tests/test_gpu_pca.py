"""GPU: srlhip_pca_forward (csrc/pca_project.hip) against the library's host twin BIT FOR BIT — the same header functions, so the kernel
holds tests/test_pca_cpu.py's derived bound transitively — batch invariance, determinism, orientation, and the PCA model inside
PixelStateVecEnv (eager, graph, policy rollout) and HipVecEnv (two shards)."""
import numpy as np
import pytest
import torch

import pca_ref as ref
from srlhip import _lib
from state_representation.models import SRLPCA

pytestmark = pytest.mark.gpu


def _forward(proj, frames, f32=False, n=None):
    n = len(frames) if n is None else n
    x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = torch.full((n, proj.state_dim), float("nan"), dtype=torch.float32 if f32 else torch.float64, device="cuda")
    proj.forward(x.data_ptr(), n, out.data_ptr(), states_f32=f32, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _model(F, S, seed, whiten=True):
    rng = np.random.RandomState(seed)
    w, b = ref.fold(ref.make_model(rng, F, S, whiten))
    return rng, w, b


# F: 192 below one chunk, 720 ragged, 2500 several chunks and a ragged tail at a frame stride that is no multiple of 16 (the byte path),
# 12288 = 64 x 64 x 3, 24576 = 6 channels
@pytest.mark.parametrize("F", [192, 720, 2500, 12288, 24576])
@pytest.mark.parametrize("S", [1, 5, 32, 64])
def test_kernel_equals_the_host_twin_bit_for_bit(F, S):
    rng, w, b = _model(F, S, 100 * S + F % 97)
    proj = _lib.PcaProjector(0, w, b)
    frames = ref.make_frames(rng, 130, F)
    frames[64], frames[65] = 255, 0                       # (also inside the batch, across the tile seam of 64-column states)
    want = _lib.pca_project_host(w, b, frames)
    want32 = want.astype(np.float32)
    for n in (1, 3, 65, 130):
        sub = frames[130 - n:]                             # every n ends with the all-0 and all-255 frames
        assert ref.same_bits(_forward(proj, sub), want[130 - n:]), n
        assert ref.same_bits(_forward(proj, sub, f32=True), want32[130 - n:]), n
    proj.close()


def test_kernel_equals_the_host_twin_at_the_reference_frame_size():
    """F = 224 x 224 x 3: 294 chunks joined through the partial buffer"""
    F, S = 150528, 5
    rng, w, b = _model(F, S, 5)
    proj = _lib.PcaProjector(0, w, b)
    frames = ref.make_frames(rng, 2, F)
    frames[1] = 255
    want = _lib.pca_project_host(w, b, frames)
    assert ref.same_bits(_forward(proj, frames), want)
    assert ref.same_bits(_forward(proj, frames, f32=True), want.astype(np.float32))
    proj.close()


def test_zero_frames_and_refusals():
    _, w, b = _model(192, 5, 1)
    proj = _lib.PcaProjector(0, w, b)
    proj.forward(None, 0, None)                            # n = 0: a successful call that launches nothing
    with pytest.raises(_lib.SrlHipError):
        proj.forward(None, 3, None)
    with pytest.raises(_lib.SrlHipError):
        _lib.PcaProjector(0, np.zeros((4, 65)), np.zeros(65))
    proj.close()


@pytest.mark.parametrize("F,S", [(720, 5), (12288, 32), (2500, 64)])
def test_batch_invariance_and_determinism(F, S):
    rng, w, b = _model(F, S, 9)
    frames = ref.make_frames(rng, 130, F)
    proj = _lib.PcaProjector(0, w, b)
    alone = _forward(proj, frames[:1])                     # before any larger batch has grown the scratch
    first = np.concatenate([frames[:1], frames[1:]])
    at0 = _forward(proj, first)
    last = np.concatenate([frames[1:], frames[:1]])
    at129 = _forward(proj, last)
    assert ref.same_bits(alone[0], at0[0]) and ref.same_bits(alone[0], at129[129])
    assert ref.same_bits(at0[1:], at129[:129])
    assert ref.same_bits(_forward(proj, first), at0)       # two launches on the same input
    assert ref.same_bits(_forward(proj, frames[:1]), alone)  # after forwards of another batch size have grown the scratch
    fresh = _lib.PcaProjector(0, w, b)
    small = _forward(fresh, frames[:3])
    _forward(fresh, frames)
    assert ref.same_bits(_forward(fresh, frames[:3]), small) and ref.same_bits(small, at0[:3])
    proj.close(); fresh.close()


def _device_frames(n, F, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n, F), dtype=torch.uint8, device="cuda", generator=g)


def _enqueue(proj, x, out, stream):
    proj.forward(x.data_ptr(), len(x), out.data_ptr(), states_f32=out.dtype == torch.float32, stream=stream.cuda_stream)


def test_a_batch_of_several_launches():
    """F = 24576, S = 64: 48 chunks x 128 frames x 64 columns of float64 chunk sums per frame tile, so 512 MiB hold 170 tiles = 21760
    frames and 21900 frames go as two launches through the same scratch.  Bitwise the two halves' forwards (one launch each), and the
    host twin's on the rows either side of the seam."""
    F, S, n, seam = 24576, 64, 21900, 21760
    rng, w, b = _model(F, S, 31)
    x = _device_frames(n, F, 32)
    x[seam - 1], x[seam] = 0, 255
    proj = _lib.PcaProjector(0, w, b)
    cur = torch.cuda.current_stream()
    for dtype in (torch.float64, torch.float32):
        whole = torch.full((n, S), float("nan"), dtype=dtype, device="cuda")
        halves = torch.full((n, S), float("nan"), dtype=dtype, device="cuda")
        _enqueue(proj, x, whole, cur)
        _enqueue(proj, x[:n // 2], halves[:n // 2], cur)
        _enqueue(proj, x[n // 2:], halves[n // 2:], cur)
        torch.cuda.synchronize()
        assert ref.same_bits(whole.cpu().numpy(), halves.cpu().numpy())
        rows = [0, seam - 1, seam, n - 1]
        want = _lib.pca_project_host(w, b, x[rows].cpu().numpy(), states_f32=dtype == torch.float32)
        assert ref.same_bits(whole[rows].cpu().numpy(), want)
    proj.close()


def test_one_handle_on_two_streams_at_once():
    """Two batches through ONE handle on two unordered streams, back to back with no synchronisation between them: 2048 frames of
    64 x 64 x 3 are 192 workgroups a launch, fewer than the device has compute units, so the two streams' launches run side by side.
    Each stream's states are bitwise what the batch gives alone: the chunk sums and the tickets are the stream's, not the handle's."""
    F, S, n, rounds = 12288, 32, 2048, 8
    rng, w, b = _model(F, S, 41)
    proj = _lib.PcaProjector(0, w, b)
    xs = [_device_frames(n, F, 42), _device_frames(n, F, 43)]
    alone = []
    for x in xs:
        out = torch.full((n, S), float("nan"), dtype=torch.float64, device="cuda")
        _enqueue(proj, x, out, torch.cuda.current_stream())
        torch.cuda.synchronize()
        alone.append(out.cpu().numpy())
    rows = [0, n - 1]
    for x, got in zip(xs, alone):
        assert ref.same_bits(got[rows], _lib.pca_project_host(w, b, x[rows].cpu().numpy()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((rounds, n, S), float("nan"), dtype=torch.float64, device="cuda") for _ in xs]
    torch.cuda.synchronize()
    for r in range(rounds):
        for x, out, st in zip(xs, outs, streams):
            _enqueue(proj, x, out[r], st)
    torch.cuda.synchronize()
    for out, want in zip(outs, alone):
        got = out.cpu().numpy()
        for r in range(rounds):
            assert ref.same_bits(got[r], want), r
    proj.close()


def test_orientation():
    """W with a single 1 at [f0][s0] and asymmetric values elsewhere, b distinct per column, distinct bytes: a transposed tile or a
    swapped row and column shows"""
    F, S, f0, s0 = 720, 5, 533, 3
    w = np.zeros((F, S))
    w[f0, s0] = 1.0
    b = np.array([0.5, -1.25, 2.0, 1000.0, -7.0])
    frames = (np.arange(4 * F).reshape(4, F) * 7 % 251).astype(np.uint8)
    proj = _lib.PcaProjector(0, w, b)
    got = _forward(proj, frames)
    want = np.tile(b, (4, 1))
    want[:, s0] += frames[:, f0]
    assert np.array_equal(got, want) and len(set(frames[:, f0])) == 4
    w2 = w + 2.0 ** -10 * (np.arange(F)[:, None] * 3 + np.arange(S)[None, :] * 5 + 1) % 17      # every product and sum exact
    proj2 = _lib.PcaProjector(0, w2, b)
    got2 = _forward(proj2, frames)
    assert np.array_equal(got2, frames.astype(np.float64) @ w2 + b) and ref.same_bits(got2, _lib.pca_project_host(w2, b, frames))
    proj.close(); proj2.close()


# ---- the model inside the envs ---------------------------------------------------------------------------------------------------------
def _srlpca(S, F, seed, backend="auto"):
    m = SRLPCA(S, cuda=True, backend=backend)
    m.set_model(ref.make_model(np.random.RandomState(seed), F, S, True))
    return m


def _twin32(m, images):
    w, b = m._w.cpu().numpy(), m._b.cpu().numpy()
    return _lib.pca_project_host(w, b, images.cpu().numpy(), states_f32=True)


def test_pixel_state_vec_env_with_a_pca_model():
    from srlhip.pixel_env import PixelStateVecEnv
    n, S = 64, 5
    m = _srlpca(S, 64 * 64 * 3, 21)
    assert m.hip is not None and m.backend == "hip" and m.replicate("cuda:0").backend == "hip"
    assert _srlpca(S, 64 * 64 * 3, 21, backend="torch").hip is None
    env = PixelStateVecEnv("KukaButtonGymEnv-v0", n, m, seed=3)
    acts = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    for states in (env.reset(), env.step(acts)[0], env.step()[0]):
        torch.cuda.synchronize()
        assert states is env.states and states.dtype == torch.float32
        assert ref.same_bits(states.cpu().numpy(), _twin32(m, env.images))
    env.close()
    # the step replayed from a graph: bitwise the eager one's
    envs = [PixelStateVecEnv("KukaButtonGymEnv-v0", n, m, seed=4, use_graph=flag) for flag in (False, True)]
    for e in envs:
        e.reset()
    for t in range(5):
        outs = []
        for e in envs:
            s, r, d = e.step()
            torch.cuda.synchronize()
            outs.append((s.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy()))
        for a, b in zip(*outs):
            assert ref.same_bits(a, b), t
    assert envs[1]._graphs and not envs[0]._graphs
    for e in envs:
        e.close()


def test_pixel_state_policy_rollout_with_a_pca_model():
    """rollout_policy on the PCA states: row t of the obs plane is written by the kernel.  Against the same env driven through the torch
    formulation: an env-step is vouched for while, at every step so far, the margin between the two best scores of the state the action
    was taken from exceeded what the two formulations' difference can move a score by — |state - state'| <= the derived bound (two
    summations of the same terms) plus a float32 ulp, carried through |W|.  Those env-steps must agree, and be at least 95 % of all."""
    from srlhip.pixel_env import PixelStateVecEnv
    n, S, T, A, F = 64, 5, 4, 6, 64 * 64 * 3
    hip, tor = _srlpca(S, F, 22), _srlpca(S, F, 22, backend="torch")
    W = torch.from_numpy(np.random.RandomState(8).standard_normal((S, A))).cuda()
    outs, envs, start = [], [], []
    for m in (hip, tor):
        env = PixelStateVecEnv("KukaButtonGymEnv-v0", n, m, seed=6)
        start.append(env.reset().to(torch.float32).cpu().numpy().copy())
        out = env.rollout_policy(T, W, per_env=False)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
        envs.append(env)
    assert outs[0]["obs"].dtype == np.float32 and ref.same_bits(outs[0]["obs"][T - 1], _twin32(hip, envs[0].images))
    w, b, Wn = hip._w.cpu().numpy(), hip._b.cpu().numpy(), np.abs(W.cpu().numpy())
    cap = 255.0 * np.abs(w).sum(axis=0) + np.abs(b)                   # >= sum_f x_f |w_fs| + |b_s| for every frame
    valid, vouched = np.ones(n, bool), 0
    for t in range(T):
        st = (start[0] if t == 0 else outs[0]["obs"][t - 1]).astype(np.float64)      # the states step t's actions were taken from
        move = ((ref.bound(F, cap)[None, :] + 2.0 ** -23 * np.abs(st)) @ Wn).max(axis=1)
        sc = np.sort(st @ W.cpu().numpy(), axis=1)
        valid &= (sc[:, -1] - sc[:, -2]) > 2.0 * move
        vouched += int(valid.sum())
        for k in ("actions", "reward", "done"):
            assert np.array_equal(outs[0][k][t][valid], outs[1][k][t][valid]), (k, t)
    print("env-steps vouched for: %d of %d" % (vouched, n * T))
    assert vouched >= 0.95 * n * T
    for e in envs:
        e.close()


def test_hip_vec_env_with_a_pca_model_on_two_shards():
    from srlhip.vec_env import HipVecEnv
    n, S, F = 32, 10, 64 * 64 * 3
    hip, tor = _srlpca(S, F, 23), _srlpca(S, F, 23, backend="torch")
    kw = {"img_shape": (64, 64), "srl_model": "pca"}
    env = HipVecEnv("MobileRobotGymEnv-v0", n, seed=5, env_kwargs=kw, encoder=hip, device_ids=[0, 0])
    twin = HipVecEnv("MobileRobotGymEnv-v0", n, seed=5, env_kwargs=kw, encoder=tor, device_ids=[0, 0])
    w, b = hip._w.cpu().numpy(), hip._b.cpu().numpy()
    rs = np.random.RandomState(2)
    obs, obs_t = env.reset(), twin.reset()
    for t in range(4):
        frames = np.concatenate([sh.t["images"].cpu().numpy() for sh in env._shards])
        assert obs.dtype == np.float64 and obs.shape == (n, S)
        assert ref.same_bits(obs, _lib.pca_project_host(w, b, frames)), t
        x = frames.reshape(n, -1).astype(np.float64)
        assert (np.abs(obs - obs_t) <= ref.bound(F, x @ np.abs(w) + np.abs(b)[None, :])).all(), t
        a = rs.randint(4, size=n)
        obs, r, d, _ = env.step(a)
        obs_t, r2, d2, _ = twin.step(a)
        assert np.array_equal(r, r2) and np.array_equal(d, d2)
    env.close(); twin.close()


def test_hip_vec_env_shards_of_one_gpu_overlap_on_one_model():
    """Two 2048-env shards on one GPU, one SRLPCA model between them: each shard enqueues its forward on its own stream and nothing
    orders the two, so the launches (about 0.2 ms each) overlap.  The observations are still the host twin of each shard's frames."""
    from srlhip.vec_env import HipVecEnv
    n, S, F = 4096, 5, 64 * 64 * 3
    hip = _srlpca(S, F, 24)
    env = HipVecEnv("MobileRobotGymEnv-v0", n, seed=7, env_kwargs={"img_shape": (64, 64), "srl_model": "pca"}, encoder=hip, device_ids=[0, 0])
    assert [sh.n for sh in env._shards] == [2048, 2048] and all(sh.enc is hip for sh in env._shards)
    w, b = hip._w.cpu().numpy(), hip._b.cpu().numpy()
    obs = env.reset()
    for t in range(2):
        frames = np.concatenate([sh.t["images"].cpu().numpy() for sh in env._shards])
        assert obs.dtype == np.float64 and ref.same_bits(obs, _lib.pca_project_host(w, b, frames)), t
        obs = env.step(np.full(n, t % 4))[0]
    env.close()


def test_srlpca_device_and_stream_arguments():
    """a bare "cuda" is torch's current device for the tensors and the projector alike; with a stream of the caller's, frames that
    would need a temporary copy (numpy, another device, not contiguous) are refused — torch's allocator does not know that stream"""
    m = _srlpca(5, 192, 25)
    assert m.device == torch.device("cuda", torch.cuda.current_device()) and m._w.device == m.device
    frames = ref.make_frames(np.random.RandomState(3), 6, 192)
    x = torch.from_numpy(frames).cuda()
    want = _lib.pca_project_host(m._w.cpu().numpy(), m._b.cpu().numpy(), frames)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = m.getStates(x, stream=st.cuda_stream)
    st.synchronize()
    assert ref.same_bits(got.cpu().numpy(), want)
    got = m.getStates(frames.reshape(6, 8, 8, 3))                  # numpy on torch's own stream: copied, as before
    torch.cuda.synchronize()
    assert ref.same_bits(got.cpu().numpy(), want)
    for bad in (frames, x.cpu(), torch.cat([x, x], dim=1)[:, :192]):
        with pytest.raises(ValueError):
            m.getStates(bad, stream=st.cuda_stream)
