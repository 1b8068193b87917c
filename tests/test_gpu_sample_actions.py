"""GPU checks of srlhip_sample_actions — the sampled selection on a score plane — and of the loops built on it: the kernel against
tests/policy_sample_ref.py with the scores given (E = 0: only 2^-48 remains), its bookkeeping (frozen envs, counters, batch invariance,
refusals), the equivalence T x (srlhip_policy_act for the scores, srlhip_sample_actions, srlhip_step) = one srlhip_rollout_policy_sampled,
and the sampled rollouts from pixels and on learned states."""
import numpy as np
import pytest

import pixel_policy_ref as ppr
import policy_sample_ref as psr
from test_policy_sample_cpu import plane

pytestmark = pytest.mark.gpu

KINDS = {2: "ENV_MOBILE_1D", 4: "ENV_MOBILE", 6: "ENV_KUKA_BUTTON"}
SEED = 11


def make_handle(A, n, io_device=1, discrete=1, obs_mode=None, rng="PHILOX", seed=SEED, kind=None):
    from srlhip import _lib
    cfg = _lib.default_config(getattr(_lib, kind or KINDS[A]))
    cfg.num_envs, cfg.seed0, cfg.is_discrete = n, seed, discrete
    cfg.rng_mode, cfg.auto_reset, cfg.io_device = getattr(_lib, "RNG_" + rng), 1, io_device
    if obs_mode is not None:
        cfg.obs_mode, cfg.img_h, cfg.img_w = obs_mode, 16, 16
    return _lib.Handle(cfg)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sample(h, score, frozen=None):
    import torch
    s, act = dev(score), torch.full((h.num_envs,), -7, dtype=torch.int32, device="cuda")
    f = None if frozen is None else dev(frozen.astype(np.uint8))
    h.sample_actions(s.data_ptr(), act.data_ptr(), frozen=None if f is None else f.data_ptr())
    h.sync()
    return act.cpu().numpy()


RESULTS = {}                                          # (A, rng, n) -> the actions of the two calls (computed once, shared)


def two_calls(A, rng, n):
    """a fresh handle: one call with every third env frozen, one with nobody frozen -> (score, frozen, first, second)"""
    if (A, rng, n) not in RESULTS:
        h = make_handle(A, n, rng=rng)
        try:
            score, frozen = plane(A, n), (np.arange(n) % 3 == 1)
            RESULTS[(A, rng, n)] = (score, frozen, sample(h, score, frozen), sample(h, score))
        finally:
            h.close()
    return RESULTS[(A, rng, n)]


@pytest.mark.parametrize("rng", ["PHILOX", "MT19937"])
@pytest.mark.parametrize("A", [2, 4, 6])
@pytest.mark.parametrize("n", [5, 67])
def test_kernel_against_the_reference_frozen_envs_counters_and_batch_invariance(n, A, rng):
    """equal rows, a dominant score (ahead by 800: the other weights underflow to 0), -0.0 entries, plain rows (test_policy_sample_cpu.plane)"""
    score, frozen, first, second = two_calls(A, rng, n)
    seeds = SEED + np.arange(n)
    ok, differs, banded = psr.sample_check(score, None, 0, psr.draws(seeds, 0, 1)[0], first, frozen)
    print("n = {}, A = {}: {} decided differently by numpy at rho = 0, {} inside the band".format(n, A, int(differs.sum()), int(banded.sum())))
    assert ok.all() and not banded.any()
    assert np.all(first[frozen] == -1) and np.all(first[~frozen] >= 0)
    dom = (np.arange(n) % 4 == 1) & ~frozen
    assert np.array_equal(first[dom], (np.arange(n)[dom] // 4) % A)
    # every counter is c + 1, frozen or not: the second call, with nobody frozen, draws at block 1 for every env
    ok, _, _ = psr.sample_check(score, None, 0, psr.draws(seeds, 1, 1)[0], second)
    assert ok.all()
    if n == 67:
        stale, _, _ = psr.sample_check(score, None, 0, psr.draws(seeds, 0, 1)[0], second)
        assert not stale[frozen].all() and not stale[~frozen].all(), "the check must tell block 0 from block 1, for frozen envs too"
    # env e's result does not depend on the batch: n = 5 equals the first five rows of n = 67
    small, big = two_calls(A, rng, 5), two_calls(A, rng, 67)
    assert np.array_equal(small[2], big[2][:5]) and np.array_equal(small[3], big[3][:5])


def test_any_env_kind_model_and_observation_mode_and_a_graph_replays_afresh():
    """a lumped-model KukaRandButton handle in raw_pixels mode: the call reads the action space and the counters only"""
    import torch
    from srlhip import _lib
    cfg = _lib.default_config(_lib.ENV_KUKA_RAND)
    cfg.num_envs, cfg.seed0, cfg.rng_mode, cfg.io_device, cfg.kuka_model = 9, SEED, _lib.RNG_PHILOX, 1, _lib.KUKA_MODEL_LUMPED
    cfg.obs_mode, cfg.img_h, cfg.img_w = _lib.OBS_RAW_PIXELS, 16, 16
    h = _lib.Handle(cfg)
    score = plane(6, 9)
    s, act = dev(score), torch.zeros((9,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h.graph_begin()
    h.sample_actions(s.data_ptr(), act.data_ptr())
    g = h.graph_end()
    seeds = SEED + np.arange(9)
    for rep in range(3):
        h.graph_launch(g)
        h.sync()
        ok, _, _ = psr.sample_check(score, None, 0, psr.draws(seeds, rep, 1)[0], act.cpu().numpy())
        assert ok.all(), rep
    h.graph_destroy(g)
    h.close()


def test_refusals_by_message():
    import torch
    from srlhip import _lib
    s, act = torch.zeros((5, 7), dtype=torch.float64, device="cuda"), torch.zeros((5, 7), dtype=torch.int32, device="cuda")

    def call(h, scores, out):
        return h._lib.srlhip_sample_actions(h._h, scores, None, out)

    h = make_handle(4, 5)
    assert call(h, None, act.data_ptr()) == -22 and h.last_error() == "sample_actions: null scores or act_out"
    assert call(h, s.data_ptr(), None) == -22 and h.last_error() == "sample_actions: null scores or act_out"
    assert call(h, s.data_ptr(), act.data_ptr()) == 0
    h.close()
    for kind in ("ENV_MOBILE", "ENV_KUKA_BUTTON"):
        h = make_handle(4, 5, discrete=0, kind=kind)
        assert call(h, s.data_ptr(), act.data_ptr()) == -95
        assert h.last_error().startswith("sample_actions:") and "discrete" in h.last_error()
        h.close()
    h = make_handle(4, 5, io_device=0)
    host_s, host_a = np.zeros((5, 4)), np.zeros(5, np.int32)
    assert call(h, host_s.ctypes.data, host_a.ctypes.data) == -95
    assert h.last_error() == "sample_actions: device-pointer handles only (io_device = 1)"
    h.reset()
    h.step_async(np.zeros(5, np.int32))
    assert call(h, host_s.ctypes.data, host_a.ctypes.data) == -22 and "pending" in h.last_error()
    h.step_wait()
    h.close()


@pytest.mark.parametrize("kind,rng,normalize,freeze", [("MobileRobotGymEnv-v0", "philox", 0, 1), ("MobileRobot2TargetGymEnv-v0", "mt19937", 1, 0)])
def test_the_loop_of_launches_equals_the_fused_sampled_rollout(kind, rng, normalize, freeze):
    """MobileRobot, n = 32, T = 40 (step counters set to 230: every env passes its 251-step limit inside the call): T x (srlhip_policy_act
    linear for score_out, srlhip_sample_actions, srlhip_step) equals one srlhip_rollout_policy_sampled bit for bit — actions and every plane"""
    import torch
    from srlhip import _lib
    from srlhip.device_env import DeviceVecEnv
    n, T, seed = 32, 40, 6
    envs = [DeviceVecEnv(kind, n, seed=seed, rng_mode=rng) for _ in range(2)]
    D, A = envs[0].h.obs_dim, envs[0].h.num_actions
    W = torch.from_numpy(np.random.RandomState(1).uniform(-2, 2, size=(n, D, A))).cuda()
    mean = torch.tensor([0.2, -0.3][:D], dtype=torch.float64, device="cuda") if normalize else None
    std = torch.tensor([0.9, 1.3][:D], dtype=torch.float64, device="cuda") if normalize else None
    obs0 = []
    for e in envs:
        e.reset()
        torch.cuda.synchronize()
        e.h.set_state(_lib.F_STEP_COUNT, np.full(n, 230, np.int32))
        obs0.append(e.obs.clone())
    fused = envs[0].rollout_policy(T, W, freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=1.5, sample=True)
    torch.cuda.synchronize()
    env, h = envs[1], envs[1].h
    frozen = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    score = torch.zeros((n, A), dtype=torch.float64, device="cuda")
    out = {"obs": torch.zeros((T, n, D), dtype=torch.float32, device="cuda"), "reward": torch.zeros((T, n), dtype=torch.float32, device="cuda"),
           "done": torch.zeros((T, n), dtype=torch.uint8, device="cuda"), "actions": torch.zeros((T, n), dtype=torch.int32, device="cuda")}
    prev = obs0[1].contiguous()
    for t in range(T):
        h.policy_act(prev.data_ptr(), D, out["actions"][t].data_ptr(), weights=W.data_ptr(), freeze_after_done=bool(freeze),
                     obs_mean=None if mean is None else mean.data_ptr(), obs_std=None if std is None else std.data_ptr(), clip_obs=1.5,
                     done_prev=out["done"][t - 1].data_ptr() if t else None, frozen=frozen.data_ptr(), score_out=score.data_ptr())
        h.sample_actions(score.data_ptr(), out["actions"][t].data_ptr(), frozen=frozen.data_ptr() if freeze else None)
        h.step(out["actions"][t].data_ptr(), out=(out["obs"][t].data_ptr(), out["reward"][t].data_ptr(), out["done"][t].data_ptr()))
        prev = out["obs"][t]
    h.sync()
    assert (fused["done"].cpu().numpy() & 1).any(0).all()
    if freeze:
        assert (fused["actions"].cpu().numpy() == -1).any()
    for k in ("actions", "obs", "reward", "done"):
        assert np.array_equal(fused[k].cpu().numpy().view(np.uint8), out[k].cpu().numpy().view(np.uint8)), k
    # ... and both handles' action streams stand at the same counter
    a, b = (torch.zeros((4, n), dtype=torch.int32, device="cuda") for _ in range(2))
    envs[0].h.rollout(4, out=(None, None, None, a.data_ptr()))
    envs[1].h.rollout(4, out=(None, None, None, b.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    for e in envs:
        e.close()


@pytest.mark.parametrize("freeze", [False, True])
def test_raw_pixel_rollout_samples_from_the_frames_scores(freeze):
    """RawPixelVecEnv.rollout_pixel_policy(sample=True) at 16 x 16, n = 8, T = 12: two runs from one seed give equal bits; a twin stepped
    with the recorded actions supplies the frames, and every action is accepted against tests/pixel_policy_ref.py's scores (which the
    device's scores equal bit for bit: E = 0)"""
    import torch
    from srlhip.pixel_env import RawPixelVecEnv
    n, T, seed, IMG = 8, 12, 5, (16, 16)
    envs = [RawPixelVecEnv("MobileRobotGymEnv-v0", n, seed=seed, img_shape=IMG) for _ in range(3)]
    try:
        A, D = envs[0].h.num_actions, IMG[0] * IMG[1] * 3
        rng = np.random.RandomState(3)
        M = torch.from_numpy(rng.uniform(-1, 1, size=(D, A)) * 2e-4).cuda()
        delta = torch.from_numpy(rng.normal(size=(n // 2, D, A))).cuda()
        noise = 1e-4
        for e in envs:
            e.reset()
        if freeze:                                       # every env reports done at step 2 of the call
            for e in envs:
                torch.cuda.synchronize()
                from srlhip import _lib
                e.h.set_state(_lib.F_STEP_COUNT, np.full(n, 249, np.int32))
        runs = []
        for e in envs[:2]:
            o = e.rollout_pixel_policy(T, M, delta, noise, freeze_after_done=freeze, sample=True)
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy() for k, v in o.items()})
        for k in runs[0]:
            assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k
        got = runs[0]
        twin = envs[2]
        u = psr.draws(seed + np.arange(n), 0, T)
        seen = np.zeros(n, bool)
        off = 0
        for t in range(T):
            torch.cuda.synchronize()
            frames = twin.images.cpu().numpy().copy()
            score = ppr.scores(frames, M.cpu().numpy(), delta.cpu().numpy(), noise)
            fz = seen if freeze else np.zeros(n, bool)
            ok, _, banded = psr.sample_check(score, None, 0, u[t], got["actions"][t], fz)
            assert ok.all() and not banded.any(), t
            off += int((got["actions"][t] != score.argmax(1))[~fz].sum())
            _, r, d = twin.step(torch.from_numpy(got["actions"][t]).cuda())
            torch.cuda.synchronize()
            assert np.array_equal(r.cpu().numpy().view(np.uint32), got["reward"][t].view(np.uint32)) and np.array_equal(d.cpu().numpy(), got["done"][t])
            seen = seen | ((got["done"][t] & 1) != 0)
        assert off > 0, "the scores must leave room to sample"
        if freeze:
            assert seen.all() and (got["actions"][-1] == -1).all()
    finally:
        for e in envs:
            e.close()


def test_learned_state_rollout_samples_the_linear_policy():
    """PixelStateVecEnv.rollout_policy(sample=True) on 64 x 64 frames (the smallest the encoder tests use), n = 6, T = 10: every action
    is accepted given the state plane the call returned (the previous row; the states the env held before the call for row 0), and two
    envs from one seed give equal bits"""
    import torch
    from srlhip.pixel_env import PixelStateVecEnv
    from state_representation.models import SRLNeuralNetwork
    n, T, seed, D = 6, 10, 3, 3
    torch.manual_seed(0)
    enc = SRLNeuralNetwork(D, cuda=True, img_shape=(64, 64))
    envs = [PixelStateVecEnv("MobileRobotGymEnv-v0", n, enc, seed=seed, img_shape=(64, 64), env_kwargs={"is_discrete": True}) for _ in range(2)]
    try:
        A = envs[0].h.num_actions
        Wn = np.random.RandomState(5).uniform(-2, 2, size=(n, D, A))
        W = torch.from_numpy(Wn).cuda()
        runs, first = [], []
        for e in envs:
            s0 = e.reset()
            torch.cuda.synchronize()
            first.append(s0.to(torch.float32).cpu().numpy().copy())
            o = e.rollout_policy(T, W, sample=True)
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy() for k, v in o.items()})
        for k in runs[0]:
            assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k
        got = runs[0]
        prev = np.concatenate([first[0][None], got["obs"][:-1]], 0)
        u = psr.draws(seed + np.arange(n), 0, T)
        for t in range(T):
            score, S = psr.scores(prev[t], Wn)
            ok, _, banded = psr.sample_check(score, S, D, u[t], got["actions"][t])
            assert ok.all() and not banded.any(), t
        det = envs[1]
        det.reset()
        assert not np.array_equal(det.rollout_policy(T, W)["actions"].cpu().numpy(), got["actions"])      # it does sample
    finally:
        for e in envs:
            e.close()
