"""GPU checks of the fused linear-policy rollout (srlhip_rollout_policy): the MobileRobot family and the full-model Kuka envs
(KukaButton, KukaMovingButton, Kuka2Button).

Every case checks three things on the same run:
  1. policy    the recorded action of every (t, env) is the float64 numpy policy applied to the recorded previous observation
               (at t = 0 the one reset() returned); frozen envs take the `None` action from the step after their first done;
  2. dynamics  a second handle with the same seed, run through srlhip_rollout with the recorded actions as the GIVEN plane, is
               bit-identical: planes, episode statistics, final state, Monitor's record planes;
  3. oracle    MobileRobot: oracle.clib.mobile_rollout with the recorded actions is bit-identical, all four env kinds.  KukaButton:
               oracle.kuka_clib.rollout, reward / done bit for bit and |obs - oracle| <= 1e-4 before the IK conditioning flag.
Shapes: n = 7 (a tail group / a partial wavefront), n = 260 (more than one 256-lane MobileRobot workgroup, 65 Kuka workgroups on the
padded grid); MobileRobot T = 300 (crosses the 251-step reset); Kuka T = 64, and n = 16 x T = 1100 across the 1001-step limit.
Then the surfaces (DeviceVecEnv, sharded HipVecEnv, graph replay, refusals, persistent park / resume) and ARS."""
import numpy as np
import pytest

from oracle import clib
from srlhip import _lib

pytestmark = pytest.mark.gpu

T = 300
N_ACT = {0: 4, 1: 2, 2: 4, 3: 4}
STATE_FIELDS = ("F_POS_X", "F_POS_Y", "F_TARGET_X", "F_TARGET_Y", "F_TARGET2_X", "F_TARGET2_Y", "F_STEP_COUNT", "F_CUR_TARGET",
                "F_EP_RETURN", "F_EP_LENGTH", "F_LAST_REWARD", "F_LAST_RETURN", "F_LAST_LENGTH", "F_N_FINISHED")


def make(kind, n, rng_mode, seed0=0, **kw):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.rng_mode, cfg.auto_reset, cfg.seed0 = n, rng_mode, 1, seed0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return _lib.Handle(cfg)


def weights_for(h, per_env, seed):
    return np.random.RandomState(seed).standard_normal(h.policy_shape(per_env))


def numpy_policy(prev_obs, W, per_env, mean=None, std=None, clip=10.0):
    """float64 scores [T][N][A] and the error scale sum_d |x_d W[d][a]| of the same shape"""
    x = prev_obs
    if mean is not None:
        x = np.clip((prev_obs.astype(np.float64) - mean) / std, -clip, clip).astype(np.float32)
    x = x.astype(np.float64)
    Wn = W if per_env else W[None]
    terms = x[:, :, :, None] * Wn[None]                # [T][N][D][A]
    score = terms[:, :, 0]
    for d in range(1, terms.shape[2]):                 # d ascending
        score = score + terms[:, :, d]
    return score, np.abs(terms).sum(2)


POLICY_TOL = 2.0 ** -50      # at most 3 products and 2 additions in float64: gamma_3 <= 3 * 2^-53; twice that (two scores are compared) < 2^-50


def check_policy(h, obs0, out, W, per_env, freeze, mean=None, std=None, clip=10.0):
    """tol_a = 2^-50 sum_d |x_d W[d][a]|.  A discrete action a has score[a] >= max(score) - tol_a, and no lower index k has
    score[k] >= score[a] + tol_a; a continuous one lies in [f32(score - tol), f32(score + tol)] — for almost every entry one float."""
    n = h.num_envs
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    score, scale = numpy_policy(prev, W, per_env, mean, std, clip)
    done = (out["done"] & 1) != 0                     # (bit 1: info_bits)
    seen_before = np.concatenate([np.zeros((1, n), bool), np.cumsum(done, 0)[:-1] > 0], 0)       # done at an EARLIER step
    frozen = seen_before if freeze else np.zeros_like(seen_before)
    if freeze:
        assert frozen.any(), "the case must freeze somebody"
    act = out["actions"]
    tol = POLICY_TOL * scale                          # [T][N][A]
    if h.cfg.is_discrete:
        A = score.shape[2]
        assert np.all(act[frozen] == -1), "frozen envs take -1"
        live = ~frozen
        assert np.all((act[live] >= 0) & (act[live] < A)), "nobody is frozen early"
        a = np.where(live, act, 0)
        sa = np.take_along_axis(score, a[..., None], 2)[..., 0]
        ta = np.take_along_axis(tol, a[..., None], 2)[..., 0]             # tol_a of the recorded action
        print("policy check: {} of {} live env-steps off numpy's argmax".format(int((a != score.argmax(2))[live].sum()), int(live.sum())))
        assert np.all((sa >= score.max(2) - ta)[live]), "score[a] >= max(score) - tol"
        lower = np.arange(A)[None, None, :] < a[..., None]
        assert np.all((~lower | (score < (sa + ta)[..., None]))[live]), "no lower index reaches score[a] + tol"
    else:
        if h.cfg.env_kind >= _lib.ENV_KUKA_BUTTON:
            assert np.isnan(act[frozen]).all(), "frozen Kuka envs take a row of NaNs"
        else:
            assert np.all(act[frozen] == 0.0), "frozen MobileRobot envs take a zero row"
        lo, hi = (score - tol).astype(np.float32), (score + tol).astype(np.float32)
        live = ~frozen
        print("policy check: {} of {} live entries have more than one float32 in their interval".format(int((lo != hi)[live].sum()), int(live.sum()) * act.shape[2]))
        assert np.all((lo <= act)[live] & (act <= hi)[live]), "f32(score - tol) <= a <= f32(score + tol)"
    return frozen


def state_of(h):
    return {f: h.get_state(getattr(_lib, f)) for f in STATE_FIELDS}


CASES = [
    # kind, discrete, rng, n, per_env, normalize, freeze
    (0, 1, "MT19937", 260, 1, 0, 0),
    (0, 1, "PHILOX", 7, 1, 0, 1),
    (1, 1, "PHILOX", 260, 1, 0, 0),
    (1, 1, "MT19937", 7, 1, 1, 1),
    (2, 1, "MT19937", 260, 1, 0, 1),
    (2, 1, "PHILOX", 7, 0, 0, 0),
    (3, 1, "PHILOX", 260, 1, 1, 1),
    (3, 1, "MT19937", 7, 1, 0, 0),
    (0, 0, "PHILOX", 260, 1, 0, 1),
    (0, 0, "MT19937", 7, 1, 1, 0),
    (3, 0, "MT19937", 260, 0, 0, 0),
    (3, 0, "PHILOX", 7, 1, 0, 1),
]


@pytest.mark.parametrize("kind,discrete,rng,n,per_env,normalize,freeze", CASES)
def test_policy_rollout_policy_dynamics_oracle(kind, discrete, rng, n, per_env, normalize, freeze):
    rng_mode, seed0 = getattr(_lib, "RNG_" + rng), 17
    kw = dict(is_discrete=discrete, random_target=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = weights_for(h, per_env, 1000 + kind)
    mean = std = None
    if normalize:
        mean, std = np.array([-0.3, 0.45])[:h.obs_dim], np.array([0.7, 1.9])[:h.obs_dim]
    obs0 = h.reset()
    out = h.rollout_policy(T, W, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=1.5)
    assert out["done"].sum() == n                      # every env crosses exactly one 251-step reset
    # 1. policy
    check_policy(h, obs0, out, W, per_env, freeze, mean, std, 1.5)
    # 2. dynamics against the existing GIVEN path (host-pointer handles: Monitor's record planes too)
    g = make(kind, n, rng_mode, seed0=seed0, **kw)
    assert np.array_equal(g.reset(), obs0)
    ref = g.rollout(T, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(ref[k], out[k]), k
    sa, sb = state_of(h), state_of(g)
    for f in STATE_FIELDS:
        assert np.array_equal(sa[f], sb[f]), f
    for a, b in zip(h.episode_stats(), g.episode_stats()):
        assert np.array_equal(a, b)
    for a, b in zip(h.episode_records(), g.episode_records()):
        assert np.array_equal(a, b)
    # the streams continue identically
    assert np.array_equal(h.rollout(40)["obs"], g.rollout(40)["obs"])
    # 3. dynamics against the CPU oracle with the recorded actions
    ora = clib.mobile_rollout(kind, seed0 + np.arange(n), T, actions=out["actions"], is_discrete=bool(discrete), random_target=True,
                              rng_mode=getattr(clib, "RNG_" + rng))
    assert np.array_equal(ora["obs0"], obs0)
    for k in ("obs", "reward", "done"):
        assert np.array_equal(ora[k], out[k]), "oracle " + k
    h.close(); g.close()


def test_null_outputs_and_chunked_calls_continue():
    """Any output plane may be missing, and two calls of T1 + T2 steps equal one of T1 + T2 (the kernel recomputes the first
    observation from the state it loads)."""
    n = 70
    hs = [make(0, n, _lib.RNG_PHILOX, seed0=3, random_target=1) for _ in range(2)]
    W = weights_for(hs[0], True, 5)
    for h in hs:
        h.reset()
    whole = hs[0].rollout_policy(T, W)
    a = hs[1].rollout_policy(130, W, want=("done",))
    assert a["obs"] is None and a["reward"] is None and a["actions"] is None
    b = hs[1].rollout_policy(T - 130, W)
    assert np.array_equal(a["done"], whole["done"][:130])
    for k in ("obs", "reward", "done", "actions"):
        assert np.array_equal(b[k], whole[k][130:]), k
    for h in hs:
        h.close()


def _single(kind, n, rng_mode, seed, W, discrete=1, **pol):
    h = make(kind, n, rng_mode, seed0=seed, is_discrete=discrete)
    obs0 = h.reset()
    out = h.rollout_policy(T, W, **pol)
    h.close()
    return obs0, out


def test_device_vec_env_equals_single_handle_and_graph_replays():
    """Every call on the tensor surface is mirrored on a host-pointer handle with the same seed (the streams continue across
    resets, so the mirror makes the same sequence of calls)."""
    import torch
    from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize
    n, seed = 260, 9
    env = DeviceVecEnv("MobileRobotGymEnv-v0", n, seed=seed, rng_mode="philox")
    W = weights_for(env.h, True, 77)
    mirror = make(0, n, _lib.RNG_PHILOX, seed0=seed)
    Wd = torch.as_tensor(W, device=env.device)
    keys = ("obs", "reward", "done", "actions")

    def same(out, ref, tag):
        for k in keys:
            assert np.array_equal(out[k].cpu().numpy(), ref[k]), tag + " " + k

    with torch.cuda.stream(env.torch_stream):
        o0 = env.reset().clone()
        out = env.rollout_policy(T, Wd, freeze_after_done=True)
    env.torch_stream.synchronize()
    assert np.array_equal(o0.cpu().numpy(), mirror.reset())
    same(out, mirror.rollout_policy(T, W, freeze_after_done=True), "on stream")
    # off the env's stream: the call synchronises by itself
    env.reset(); mirror.reset()
    same(env.rollout_policy(T, Wd, freeze_after_done=True), mirror.rollout_policy(T, W, freeze_after_done=True), "off stream")
    # graph capture of one call: the replay starts from the state the capture found and fills the same planes
    bufs = (torch.zeros((T, n, 2), dtype=torch.float32, device=env.device), torch.zeros((T, n), dtype=torch.float32, device=env.device),
            torch.zeros((T, n), dtype=torch.uint8, device=env.device), torch.zeros((T, n), dtype=torch.int32, device=env.device))
    env.reset(); mirror.reset()
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_policy(T, Wd.data_ptr(), True, True, out=tuple(b.data_ptr() for b in bufs))
    g = h.graph_end()
    h.graph_launch(g)
    h.sync()
    same(dict(zip(keys, bufs)), mirror.rollout_policy(T, W, freeze_after_done=True), "graph")
    h.graph_destroy(g)
    # wrappers: the trivial frame stack passes through, a real one refuses; frozen normalisation statistics reach the kernel
    same(DeviceVecFrameStack(env, 1).rollout_policy(4, Wd), mirror.rollout_policy(4, W), "stack of 1")
    with pytest.raises(NotImplementedError):
        DeviceVecFrameStack(env, 4).rollout_policy(4, Wd)
    norm = DeviceVecNormalize(env, training=False, norm_reward=False, clip_obs=1.5)
    norm.obs_rms.mean = torch.tensor([-0.3, 0.45], dtype=torch.float64, device=env.device)
    norm.obs_rms.var = torch.tensor([0.49, 3.61], dtype=torch.float64, device=env.device)
    std = np.sqrt(np.array([0.49, 3.61]) + norm.epsilon)
    env.reset(); mirror.reset()
    same(norm.rollout_policy(T, Wd, freeze_after_done=True),
         mirror.rollout_policy(T, W, freeze_after_done=True, obs_mean=np.array([-0.3, 0.45]), obs_std=std, clip_obs=1.5), "normalised")
    count0 = norm.obs_rms.count
    norm.training = True
    env.reset()
    norm.rollout_policy(T, Wd, freeze_after_done=True)
    assert norm.obs_rms.count == count0 + 251 * n          # rows up to and including each env's first done (step 250)
    env.close(); mirror.close()


KUKA_FIELDS = ("F_KUKA_Q", "F_KUKA_QD", "F_KUKA_GRIPPER_Q", "F_KUKA_COUNTERS", "F_EP_RETURN", "F_EP_LENGTH", "F_LAST_RETURN",
               "F_LAST_LENGTH", "F_N_FINISHED", "F_LAST_REWARD")
KUKA_WEIGHT_SEED = {(1, 0): 2001, (0, 0): 2000, (0, 1): 2002}          # (discrete, joints): see the test's docstring
KUKA_CASES = [
    # env kind, discrete, joints, rng, n, T, per_env, normalize, freeze, oracle
    ("KUKA_BUTTON", 1, 0, "PHILOX", 7, 64, 1, 0, 0, 1),
    ("KUKA_BUTTON", 1, 0, "MT19937", 260, 64, 1, 0, 0, 1),
    ("KUKA_BUTTON", 0, 0, "PHILOX", 260, 64, 1, 1, 0, 1),
    ("KUKA_BUTTON", 0, 1, "MT19937", 7, 64, 1, 0, 0, 1),
    ("KUKA_MOVING", 1, 0, "PHILOX", 7, 64, 0, 0, 0, 0),
    ("KUKA_2BUTTON", 1, 0, "MT19937", 7, 64, 1, 0, 0, 0),
    ("KUKA_BUTTON", 1, 0, "PHILOX", 16, 1100, 1, 0, 1, 1),
    ("KUKA_BUTTON", 0, 0, "MT19937", 7, 1100, 1, 0, 1, 0),          # continuous freeze: the all-NaN `None` rows
    ("KUKA_2BUTTON", 1, 0, "PHILOX", 5, 3, 1, 0, 0, 0),             # the linear policy's two-button kernel on the Philox streams: no other case launches it
]


@pytest.mark.parametrize("env,discrete,joints,rng,n,T_,per_env,normalize,freeze,oracle", KUKA_CASES)
def test_kuka_policy_rollout_policy_dynamics_oracle(env, discrete, joints, rng, n, T_, per_env, normalize, freeze, oracle):
    """Full-model Kuka envs: the three checks of the MobileRobot cases.  The oracle comparison (KukaButton; reward and done bit for
    bit, |obs - oracle| <= 1e-4) covers every env-step before the env's first IK conditioning flag (bit 1 of the done bytes,
    info_bits = 1; everything after it is masked, later episodes included) and has to cover at least half of all env-steps.  The
    n = 16, T = 1100 case crosses the 1001-step limit and an auto-reset with freeze_after_done.
    Env seed 23 and the weight seeds (KUKA_WEIGHT_SEED) were fixed from the CPU oracle run closed-loop under the numpy policy
    (tests/kuka_policy_closed_loop.py, no GPU): share of env-steps before the first flag for the oracle alone — discrete n = 7 and
    n = 260, T = 64, seed 2001: 1.0000; continuous Cartesian normalised n = 260, seed 2000: 1.0000; joints n = 7, seed 2002: 1.0000
    (64 steps are too few for a held action to reach the badly conditioned region); discrete n = 16, T = 1100, freeze, seed 2001:
    0.8657 (seeds 2002 / 2003: 0.8997 / 0.9055)."""
    from oracle import kuka_clib
    kind, rng_mode, seed0 = getattr(_lib, "ENV_" + env), getattr(_lib, "RNG_" + rng), 23
    kw = dict(is_discrete=discrete, action_joints=joints, info_bits=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = weights_for(h, per_env, KUKA_WEIGHT_SEED[(discrete, joints)])
    mean = std = None
    if normalize:
        mean, std = np.array([-0.1, 0.05, 0.2]), np.array([0.3, 0.25, 0.15])
    obs0 = h.reset()
    out = h.rollout_policy(T_, W, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=2.0)
    if freeze:
        assert (out["done"] & 1).any(0).all()          # every env reaches its episode's end (the 1001-step limit at the latest)
    check_policy(h, obs0, out, W, per_env, freeze, mean, std, 2.0)
    g = make(kind, n, rng_mode, seed0=seed0, **kw)
    assert np.array_equal(g.reset(), obs0)
    ref = g.rollout(T_, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(ref[k], out[k]), k
    for f in KUKA_FIELDS:
        assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    for a, b in zip(h.episode_records(), g.episode_records()):
        assert np.array_equal(a, b)
    h.close(); g.close()
    if not oracle:
        return
    ora = kuka_clib.rollout(seed0 + np.arange(n), T_, actions=out["actions"], is_discrete=bool(discrete), action_joints=bool(joints),
                            rng_mode=getattr(kuka_clib, "RNG_" + rng), trace=False)
    flagged = np.cumsum((out["done"] >> 1) & 1, 0) > 0            # at or after the env's first flagged step
    share = 1.0 - flagged.mean()
    err = np.abs(out["obs"] - ora["obs"]).max(-1)
    print("oracle check: share compared {:.3f}, max |obs - oracle| there {:.3g}".format(share, float(err[~flagged].max())))
    assert share >= 0.5
    assert np.array_equal(ora["obs0"], obs0)
    assert np.array_equal(ora["reward"][~flagged], out["reward"][~flagged])
    assert np.array_equal(ora["done"][~flagged], (out["done"] & 1)[~flagged])
    assert err[~flagged].max() <= 1e-4


def test_kuka_chunked_calls_continue_and_graph_replays():
    """Two calls of T1 + T2 steps equal one of T1 + T2 on a Kuka handle (the kernel recomputes the first observation from the state
    it loads), and a captured call — header kernel and rollout kernel — replays to the same planes on a device-pointer handle."""
    import torch
    from srlhip.device_env import DeviceVecEnv
    n, T_, seed = 9, 48, 31
    hs = [make(_lib.ENV_KUKA_BUTTON, n, _lib.RNG_PHILOX, seed0=seed) for _ in range(2)]
    W = weights_for(hs[0], True, 41)
    mean, std = np.array([-0.1, 0.05, 0.2]), np.array([0.3, 0.25, 0.15])
    for h in hs:
        h.reset()
    whole = hs[0].rollout_policy(T_, W, obs_mean=mean, obs_std=std, clip_obs=2.0)
    a = hs[1].rollout_policy(20, W, obs_mean=mean, obs_std=std, clip_obs=2.0)
    b = hs[1].rollout_policy(T_ - 20, W, obs_mean=mean, obs_std=std, clip_obs=2.0)
    for k in ("obs", "reward", "done", "actions"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    for h in hs:
        h.close()
    env = DeviceVecEnv("KukaButtonGymEnv-v0", n, seed=seed, rng_mode="philox")
    dev = env.device
    Wd, md, sd = (torch.as_tensor(x, device=dev) for x in (W, mean, std))
    bufs = (torch.zeros((T_, n, 3), dtype=torch.float32, device=dev), torch.zeros((T_, n), dtype=torch.float32, device=dev),
            torch.zeros((T_, n), dtype=torch.uint8, device=dev), torch.zeros((T_, n), dtype=torch.int32, device=dev))
    env.reset()
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_policy(T_, Wd.data_ptr(), True, False, md.data_ptr(), sd.data_ptr(), 2.0, out=tuple(x.data_ptr() for x in bufs))
    g = h.graph_end()
    h.graph_launch(g)
    h.sync()
    for x, k in zip(bufs, ("obs", "reward", "done", "actions")):
        assert np.array_equal(x.cpu().numpy(), whole[k]), "graph " + k
    h.graph_destroy(g)
    env.close()


def test_ars_fused_rollout_on_kuka_completes_with_finite_policy():
    import argparse
    from rl_baselines.evolution_strategies.ars import ARSModel
    P = 4
    a = argparse.Namespace(env="KukaButtonGymEnv-v0", num_population=P, top_population=2, step_size=0.02, exploration_noise=0.02,
                           algo_type="v1", max_step_amplitude=10, deterministic=True, continuous_actions=False, fused_rollout=True,
                           num_timesteps=4, seed=1, srl_model="ground_truth", num_stack=1, num_cpu=2 * P, log_dir=None)
    m = ARSModel().train(a)
    assert len(m.history) == 1 and m.M.shape == (3, 6) and np.isfinite(m.M).all()


def test_sharded_host_vec_env_equals_single_handle():
    from srlhip.vec_env import HipVecEnv
    n, seed = 261, 4
    env = HipVecEnv("MobileRobotGymEnv-v0", n, seed=seed, env_kwargs={"srl_model": "ground_truth"}, device_ids=[0, 0], rng_mode="mt19937")
    W = np.random.RandomState(8).standard_normal((n, 2, 4))
    obs0, ref = _single(0, n, _lib.RNG_MT19937, seed, W, freeze_after_done=True)
    assert np.array_equal(env.reset(), obs0)
    out = env.rollout_policy(T, W, freeze_after_done=True)
    for k in ("obs", "reward", "done", "actions"):
        assert np.array_equal(out[k], ref[k]), k
    env.close()


def _call(h, T_, pol):
    return h._lib.srlhip_rollout_policy(h._h, T_, pol, None, None, None, None)


def _pol(W, **kw):
    import ctypes
    p = _lib.LinearPolicy()
    p.struct_size, p.per_env, p.weights, p.clip_obs = ctypes.sizeof(_lib.LinearPolicy), 1, W.ctypes.data, 10.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_host_pointer_validation_returns_einval_and_leaves_the_handle_usable():
    n = 7
    h = make(0, n, _lib.RNG_PHILOX, seed0=1)
    h.reset()
    W = weights_for(h, True, 2)
    ok = np.array([0.1, 0.2]), np.array([1.0, 2.0])
    assert _call(h, 4, _pol(W, struct_size=8)) == -22 and "struct_size" in h.last_error()
    assert _call(h, 0, _pol(W)) == -22
    assert _call(h, 4, _pol(W, weights=None)) == -22 and "weights" in h.last_error()
    assert _call(h, 4, _pol(W, normalize=1, obs_mean=ok[0].ctypes.data)) == -22
    assert _call(h, 4, _pol(W, normalize=1, obs_std=ok[1].ctypes.data)) == -22
    for bad in (np.array([1.0, 0.0]), np.array([-1.0, 1.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])):
        assert _call(h, 4, _pol(W, normalize=1, obs_mean=ok[0].ctypes.data, obs_std=bad.ctypes.data)) == -22, bad
        assert "obs_std" in h.last_error()
    for v in (np.nan, np.inf):
        Wb = W.copy(); Wb[3, 1, 2] = v
        assert _call(h, 4, _pol(Wb)) == -22 and "weights" in h.last_error()
    # a pending step
    h.step_async(np.zeros(n, np.int32))
    assert _call(h, 4, _pol(W)) == -22 and "pending" in h.last_error()
    h.step_wait()
    # ... and the handle still equals one that saw none of this
    g = make(0, n, _lib.RNG_PHILOX, seed0=1)
    g.reset(); g.step(np.zeros(n, np.int32))
    a, b = h.rollout_policy(T, W), g.rollout_policy(T, W)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    h.close(); g.close()


REFUSALS = [
    ("joints", _lib.ENV_KUKA_BUTTON, dict(obs_mode=_lib.OBS_JOINTS), "joints"),
    ("joints_position", _lib.ENV_KUKA_BUTTON, dict(obs_mode=_lib.OBS_JOINTS_POSITION), "joints_position"),
    ("raw_pixels", _lib.ENV_MOBILE, dict(obs_mode=_lib.OBS_RAW_PIXELS, img_h=16, img_w=16), "raw_pixels"),
    ("rand_button", _lib.ENV_KUKA_RAND, dict(), "KukaRandButton"),
    ("lumped", _lib.ENV_KUKA_BUTTON, dict(kuka_model=_lib.KUKA_MODEL_LUMPED), "lumped"),
    ("rng_host", _lib.ENV_MOBILE, dict(rng_mode=_lib.RNG_HOST, auto_reset=0), "RNG_HOST"),
    ("no_auto_reset", _lib.ENV_MOBILE, dict(auto_reset=0), "auto_reset"),
]


@pytest.mark.parametrize("name,kind,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_what_they_refuse_and_leave_the_handle_usable(name, kind, kw, word):
    n = 5
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.rng_mode, cfg.seed0 = n, _lib.RNG_PHILOX, 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = _lib.Handle(cfg)
    host_rand = np.full((n, h.reset_rand_count), 0.5) if cfg.rng_mode == _lib.RNG_HOST else None
    before = h.reset(host_rand=host_rand)
    W = np.zeros((n, 32, 8))                          # larger than any policy shape: never read
    assert _call(h, 4, _pol(W)) == -95
    assert word in h.last_error(), h.last_error()
    assert h.last_error().startswith("rollout_policy:"), h.last_error()
    again = h.reset(host_rand=host_rand)              # the refusal left the handle usable
    assert again.shape == before.shape
    if cfg.rng_mode != _lib.RNG_HOST:
        o, r, d = h.step(np.zeros(n, np.int32))
        assert d.shape == (n,) and np.isfinite(r).all()
    h.close()


def test_persistent_handle_parks_and_resumes_around_the_call():
    n = 64
    hs = [make(0, n, _lib.RNG_PHILOX, seed0=6, random_target=1) for _ in range(2)]
    W = weights_for(hs[0], True, 11)
    acts = np.random.RandomState(3).randint(4, size=(6, n)).astype(np.int32)
    hs[0].set_persistent(True)
    res = []
    for h in hs:
        r = [h.reset()]
        for t in range(3):
            r += [x.copy() for x in h.step(acts[t])]
        pol = h.rollout_policy(T, W)
        r += [pol[k] for k in ("obs", "reward", "done", "actions")]
        for t in range(3, 6):
            r += [x.copy() for x in h.step(acts[t])]
        res.append(r)
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for h in hs:
        h.close()


def test_ars_fused_rollout_equals_per_step_path():
    """ARSModel.train on MobileRobotGymEnv-v0, --deterministic --algo-type v1, P = 8, three updates: the fused path yields the
    per-step path's M to 1e-12.  Both draw the same deltas from the same generator; the rewards are 0 / +-1, so the returns are
    exact in either summation order, and the only thing that could differ is a near-tie argmax — the seed is one for which the
    per-step path's recorded scores have none (asserted)."""
    import argparse
    import torch
    from rl_baselines.evolution_strategies.ars import ARSModel
    P = 8

    def args(fused):
        return argparse.Namespace(env="MobileRobotGymEnv-v0", num_population=P, top_population=2, step_size=0.02, exploration_noise=0.02,
                                  algo_type="v1", max_step_amplitude=10, deterministic=True, continuous_actions=False, fused_rollout=fused,
                                  num_timesteps=20000, seed=5, srl_model="ground_truth", num_stack=1, num_cpu=2 * P, log_dir=None)

    class PerStep(ARSModel):
        gaps = []

        @staticmethod
        def batched_actions(obs, M, delta, noise, active, *a, **k):
            sign = torch.tensor([1.0, -1.0], dtype=M.dtype, device=M.device).view(1, 2, 1, 1)
            Wp = M.unsqueeze(0).unsqueeze(0) + noise * sign * delta.unsqueeze(1)
            x = obs.view(delta.shape[0], 2, -1, 1).to(M.dtype)
            terms = x * Wp                                             # [P][2][D][A]
            top2 = terms.sum(2).topk(2, dim=-1).values
            margin = 1e-9 * (1.0 + terms.abs().sum(2).max(-1).values)
            PerStep.gaps.append(bool((((top2[..., 0] - top2[..., 1]) < margin).view(-1) & active).any()))
            return ARSModel.batched_actions(obs, M, delta, noise, active, *a, **k)

    # every update advances `step` by P x 251 live rows = 2008; num_updates = 20000 // P * 2 = 5000 -> exactly three updates
    def run(model, fused):
        return model.train(args(fused))

    ref = run(PerStep(), False)
    assert len(ref.history) == 3
    assert not any(PerStep.gaps), "the seed must keep every argmax clear of a tie"
    fused = run(ARSModel(), True)
    assert len(fused.history) == 3
    assert np.abs(fused.M).max() > 0
    assert np.abs(fused.M - ref.M).max() <= 1e-12
    assert fused.history == ref.history
