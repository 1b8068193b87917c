"""GPU checks of the SAMPLED fused linear-policy rollout (srlhip_rollout_policy_sampled): the MobileRobot family and the full-model Kuka
envs, discrete actions — ARS's default action selection inside the physics kernels.

Every rollout case checks on one run:
  1. sampling  for every (t, env) the numpy linear policy (tests/policy_sample_ref.py) is applied to the recorded previous raw observation
               and the recorded action is held to the acceptance rule, u from the env's action stream at counter c0 + t; frozen entries are
               exactly -1.  At most 1 live decision in 10^5 may pass only through the tolerance band (printed; the CPU test shows the
               reference alone needs none).
  2. dynamics  a second handle with the same seed, run through srlhip_rollout with the recorded actions as the GIVEN plane, is
               bit-identical in observations, rewards, dones and final state;
  3. oracle    the CPU oracle with the recorded actions: MobileRobot bit for bit; KukaButton as tests/test_gpu_policy_rollout.py holds the
               deterministic kernel (reward / done bit for bit and |obs - oracle| <= 1e-4 up to an env's first IK-flagged step).
Then the counter semantics, shards, graph replays, the distribution, refusals and ARS end to end."""
import argparse
import ctypes

import numpy as np
import pytest

import policy_sample_ref as psr
from oracle import clib
from srlhip import _lib
from test_gpu_policy_rollout import KUKA_FIELDS, REFUSALS, STATE_FIELDS, make, state_of

pytestmark = pytest.mark.gpu

KEYS = ("obs", "reward", "done", "actions")
N, T = 64, 260                                     # one full 251-step episode plus the auto-reset
SEED0 = 3
MEAN, STD, CLIP = np.array([0.2, -0.3, 0.1]), np.array([0.9, 1.3, 0.7]), 5.0


def weights_for(h, per_env, seed):
    """the range tests/test_policy_sample_cpu.py pins the reference on"""
    return np.random.RandomState(seed).uniform(-2.0, 2.0, size=h.policy_shape(per_env))


def check_sampling(h, seeds, c0, obs0, out, W, per_env, freeze, mean=None, std=None, clip=10.0, need_frozen=False):
    n, D = h.num_envs, h.obs_dim
    Tn = len(out["actions"])
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    sc = [psr.scores(prev[t], W, per_env, mean, std, clip) for t in range(Tn)]
    score, S = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
    done = (out["done"] & 1) != 0
    seen_before = np.concatenate([np.zeros((1, n), bool), np.cumsum(done, 0)[:-1] > 0], 0)
    frozen = seen_before if freeze else np.zeros_like(seen_before)
    if need_frozen:
        assert frozen.any(), "the case must freeze somebody"
    u = psr.draws(seeds, c0, Tn)
    ok, differs, banded = psr.sample_check(score, S, D, u, out["actions"], frozen)
    live = int((~frozen).sum())
    print("sampling check: {} live decisions, {} decided differently by numpy at rho = 0, {} inside the tolerance band".format(
        live, int(differs.sum()), int(banded.sum())))
    assert np.all(out["actions"][frozen] == -1), "frozen envs take -1"
    assert ok.all(), "the acceptance rule fails on {} entries".format(int((~ok).sum()))
    assert banded.sum() * 10 ** 5 <= live, "more than 1 decision in 1e5 passes only through the band"
    return frozen


MOBILE_CASES = [
    # kind, rng, per_env, normalize, freeze
    (0, "PHILOX", 1, 0, 1), (0, "MT19937", 0, 1, 0),
    (1, "PHILOX", 0, 1, 1), (1, "MT19937", 1, 0, 0),
    (2, "PHILOX", 1, 1, 0), (2, "MT19937", 0, 0, 1),
    (3, "PHILOX", 0, 0, 0), (3, "MT19937", 1, 1, 1),
]


@pytest.mark.parametrize("kind,rng,per_env,normalize,freeze", MOBILE_CASES)
def test_mobile_sampled_rollout_sampling_dynamics_oracle(kind, rng, per_env, normalize, freeze):
    rng_mode = getattr(_lib, "RNG_" + rng)
    kw = dict(is_discrete=1, random_target=1)
    h = make(kind, N, rng_mode, seed0=SEED0, **kw)
    W = weights_for(h, per_env, 100 + kind)
    mean, std = (MEAN[:h.obs_dim], STD[:h.obs_dim]) if normalize else (None, None)
    obs0 = h.reset()
    out = h.rollout_policy(T, W, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=CLIP, sample=True)
    assert (out["done"] & 1).any(0).all()              # every env crosses the 251-step limit at the latest
    check_sampling(h, SEED0 + np.arange(N), 0, obs0, out, W, per_env, freeze, mean, std, CLIP, need_frozen=bool(freeze))
    g = make(kind, N, rng_mode, seed0=SEED0, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(T, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    sa, sb = state_of(h), state_of(g)
    for f in STATE_FIELDS:
        assert np.array_equal(sa[f], sb[f]), f
    ora = clib.mobile_rollout(kind, SEED0 + np.arange(N), T, actions=out["actions"], is_discrete=True, random_target=True,
                              rng_mode=getattr(clib, "RNG_" + rng))
    assert np.array_equal(ora["obs0"], obs0)
    for k in ("obs", "reward", "done"):
        assert np.array_equal(ora[k], out[k]), "oracle " + k
    # it does sample: the argmax rollout from the same state takes other actions
    d = make(kind, N, rng_mode, seed0=SEED0, **kw)
    d.reset()
    det = d.rollout_policy(T, W, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=CLIP)
    assert not np.array_equal(det["actions"], out["actions"])
    h.close(); g.close(); d.close()


KUKA_CASES = [
    # env, rng, n, T, per_env, normalize, freeze, oracle
    ("KUKA_BUTTON", "PHILOX", 16, 48, 1, 0, 0, 1),
    ("KUKA_BUTTON", "MT19937", 16, 48, 0, 1, 0, 1),
    ("KUKA_MOVING", "PHILOX", 16, 48, 1, 1, 0, 0),
    ("KUKA_MOVING", "MT19937", 16, 48, 1, 0, 0, 0),
    ("KUKA_2BUTTON", "PHILOX", 16, 48, 0, 0, 0, 0),
    ("KUKA_2BUTTON", "MT19937", 16, 48, 1, 1, 0, 0),
    ("KUKA_BUTTON", "PHILOX", 8, 1010, 1, 0, 1, 0),             # across the 1001-step limit: auto-reset, then frozen
]


@pytest.mark.parametrize("env,rng,n,T_,per_env,normalize,freeze,oracle", KUKA_CASES)
def test_kuka_sampled_rollout_sampling_dynamics_oracle(env, rng, n, T_, per_env, normalize, freeze, oracle):
    from oracle import kuka_clib
    kind, rng_mode, seed0 = getattr(_lib, "ENV_" + env), getattr(_lib, "RNG_" + rng), 23
    kw = dict(is_discrete=1, info_bits=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = weights_for(h, per_env, 2001)
    mean, std = (np.array([-0.1, 0.05, 0.2]), np.array([0.3, 0.25, 0.15])) if normalize else (None, None)
    obs0 = h.reset()
    out = h.rollout_policy(T_, W, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=2.0, sample=True)
    if freeze:
        assert (out["done"] & 1).any(0).all()
    frozen = check_sampling(h, seed0 + np.arange(n), 0, obs0, out, W, per_env, freeze, mean, std, 2.0, need_frozen=bool(freeze))
    if freeze:
        assert frozen[-1].all()
    g = make(kind, n, rng_mode, seed0=seed0, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(T_, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    for f in KUKA_FIELDS:
        assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    if freeze:                                         # the counter stands at c0 + T although every env was frozen at the end
        nxt = h.rollout_policy(1, W, per_env=bool(per_env), sample=True)
        score, S = psr.scores(out["obs"][-1], W, per_env)
        ok, _, _ = psr.sample_check(score, S, 3, psr.draws(seed0 + np.arange(n), T_, 1)[0], nxt["actions"][0])
        assert ok.all()
    h.close(); g.close()
    if not oracle:
        return
    ora = kuka_clib.rollout(seed0 + np.arange(n), T_, actions=out["actions"], is_discrete=True, action_joints=False,
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


# ---- counter semantics -------------------------------------------------------------------------------------------------------------------
def _fresh(kind, n, seed0, rng_mode=_lib.RNG_PHILOX, **kw):
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    return h, h.reset()


@pytest.mark.parametrize("kind,n,T_", [(0, 65, 40), (_lib.ENV_KUKA_BUTTON, 9, 24)])
def test_chunked_calls_equal_one_call_and_null_planes(kind, n, T_):
    (a, _), (b, _) = _fresh(kind, n, 31), _fresh(kind, n, 31)
    W = weights_for(a, True, 41)
    whole = a.rollout_policy(T_, W, sample=True)
    parts = [b.rollout_policy(1, W, sample=True), b.rollout_policy(7, W, sample=True), b.rollout_policy(T_ - 8, W, sample=True)]
    for k in KEYS:
        assert np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint8), whole[k].view(np.uint8)), k
    assert b._lib.srlhip_rollout_policy_sampled(b._h, 4, _pol(W), None, None, None, None) == 0      # every plane NULL
    a.rollout_policy(4, W, sample=True, want=())
    assert np.array_equal(a.rollout(8)["actions"], b.rollout(8)["actions"])                         # both counters stand at c0 + T + 4
    a.close(); b.close()


@pytest.mark.parametrize("kind,n", [(0, 65), (1, 5), (_lib.ENV_KUKA_BUTTON, 5)])
def test_sampled_call_continues_the_synthetic_agents_stream_and_the_reverse(kind, n):
    """rollout(40) with device-sampled actions moves the action-stream counter by 40 (MobileRobot: a count of actions, which the sampled
    call reads as a BLOCK index; Kuka: one block per action) — the sampled call that follows draws at blocks 40, 41, ...; a second one
    goes on at 40 + T; then the synthetic agent goes on at 40 + 2 T."""
    T_, seed0 = 24, 12
    mk = (lambda: _fresh(kind, n, seed0, random_target=1)) if kind < _lib.ENV_KUKA_BUTTON else (lambda: _fresh(kind, n, seed0))
    h, _ = mk()
    W = weights_for(h, True, 43)
    seeds = seed0 + np.arange(n)
    D = h.obs_dim
    c = 40
    last = h.rollout(40)["obs"][-1]
    for _ in range(2):
        out = h.rollout_policy(T_, W, sample=True)
        prev = np.concatenate([last[None], out["obs"][:-1]], 0)
        sc = [psr.scores(prev[t], W) for t in range(T_)]
        score, S = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
        ok, _, _ = psr.sample_check(score, S, D, psr.draws(seeds, c, T_), out["actions"])
        assert ok.all(), c
        wrong, _, _ = psr.sample_check(score, S, D, psr.draws(seeds, c + 1, T_), out["actions"])
        assert not wrong.all(), "the check must tell one counter from the next"
        c += T_
        last = out["obs"][-1]
    g, _ = mk()
    ref_acts = g.rollout(40 + 2 * T_ + 8)["actions"]
    assert np.array_equal(h.rollout(8)["actions"], ref_acts[40 + 2 * T_:])
    g.close(); h.close()


# ---- equalities --------------------------------------------------------------------------------------------------------------------------
def _run(kind, n, rng_mode, seed, wseed, T_, **kw):
    h = make(kind, n, rng_mode, seed0=seed, **kw)
    W = weights_for(h, True, wseed)
    obs0 = h.reset()
    out = h.rollout_policy(T_, W, freeze_after_done=True, sample=True)
    h.close()
    return obs0, out, W


def test_sharded_host_vec_env_equals_single_handle():
    from srlhip.vec_env import HipVecEnv
    n, seed = 65, 4
    env = HipVecEnv("MobileRobotGymEnv-v0", n, seed=seed, env_kwargs={"srl_model": "ground_truth"}, device_ids=[0, 0, 0], rng_mode="mt19937")
    obs0, want, W = _run(0, n, _lib.RNG_MT19937, seed, 8, T)
    assert np.array_equal(env.reset(), obs0)
    out = env.rollout_policy(T, W, freeze_after_done=True, sample=True)
    for k in KEYS:
        assert np.array_equal(out[k].view(np.uint8), want[k].view(np.uint8)), k
    env.close()


@pytest.mark.parametrize("name,n", [("MobileRobotGymEnv-v0", 65), ("KukaButtonGymEnv-v0", 9)])
def test_device_vec_env_equals_handle_and_graph_replays_draw_afresh(name, n):
    import torch
    from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize
    T_, seed = 24, 9
    env = DeviceVecEnv(name, n, seed=seed, rng_mode="philox")
    mirror = make(env.cfg.env_kind, n, _lib.RNG_PHILOX, seed0=seed)
    W = weights_for(mirror, True, 77)
    Wd = torch.as_tensor(W, device=env.device)
    D = env.h.obs_dim

    def same(out, want, tag):
        for k in KEYS:
            assert np.array_equal(out[k].cpu().numpy(), want[k]), tag + " " + k

    with torch.cuda.stream(env.torch_stream):
        o0 = env.reset().clone()
        out = env.rollout_policy(T_, Wd, freeze_after_done=True, sample=True)
    env.torch_stream.synchronize()
    assert np.array_equal(o0.cpu().numpy(), mirror.reset())
    same(out, mirror.rollout_policy(T_, W, freeze_after_done=True, sample=True), "on stream")
    bufs = (torch.zeros((T_, n, D), dtype=torch.float32, device=env.device), torch.zeros((T_, n), dtype=torch.float32, device=env.device),
            torch.zeros((T_, n), dtype=torch.uint8, device=env.device), torch.zeros((T_, n), dtype=torch.int32, device=env.device))
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_policy(T_, Wd.data_ptr(), True, False, out=tuple(b.data_ptr() for b in bufs), sample=True)
    g = h.graph_end()
    replays = []
    for rep in range(2):
        h.graph_launch(g)
        h.sync()
        same(dict(zip(KEYS, bufs)), mirror.rollout_policy(T_, W, sample=True), "graph replay %d" % rep)
        replays.append(bufs[3].cpu().numpy().copy())
    assert not np.array_equal(replays[0], replays[1])              # fresh numbers at every replay
    h.graph_destroy(g)
    same(DeviceVecFrameStack(env, 1).rollout_policy(4, Wd, sample=True), mirror.rollout_policy(4, W, sample=True), "stack of 1")
    with pytest.raises(NotImplementedError):
        DeviceVecFrameStack(env, 4).rollout_policy(4, Wd, sample=True)
    norm = DeviceVecNormalize(env, training=False, norm_reward=False, clip_obs=1.5)
    m, v = np.array([-0.3, 0.45, 0.1])[:D], np.array([0.49, 3.61, 0.3])[:D]
    norm.obs_rms.mean, norm.obs_rms.var = torch.tensor(m, dtype=torch.float64, device=env.device), torch.tensor(v, dtype=torch.float64, device=env.device)
    same(norm.rollout_policy(T_, Wd, freeze_after_done=True, sample=True),
         mirror.rollout_policy(T_, W, freeze_after_done=True, obs_mean=m, obs_std=np.sqrt(v + norm.epsilon), clip_obs=1.5, sample=True), "normalised")
    env.close(); mirror.close()


def test_persistent_kernel_parks_for_the_sampled_call():
    n = 16
    a, b = make(0, n, _lib.RNG_PHILOX, seed0=5), make(0, n, _lib.RNG_PHILOX, seed0=5)
    W = weights_for(a, True, 3)
    a.reset(); b.reset()
    a.set_persistent(True)
    acts = np.zeros(n, np.int32)
    a.step(acts); b.step(acts)
    x, y = a.rollout_policy(12, W, sample=True), b.rollout_policy(12, W, sample=True)
    for k in KEYS:
        assert np.array_equal(x[k], y[k]), k
    a.step(acts); b.step(acts)
    assert np.array_equal(a.rollout(4)["obs"], b.rollout(4)["obs"])
    a.close(); b.close()


# ---- the distribution ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,A", [(_lib.ENV_MOBILE_1D, 2), (_lib.ENV_MOBILE, 4), (_lib.ENV_KUKA_BUTTON, 6)])
def test_action_counts_follow_the_softmax(kind, A):
    """Fixed scores: a frozen normalisation with mean -1000 clips every input to +clip, so score_a = clip sum_d W[d][a] whatever the env
    does.  N = 4096 x 16 independent draws: every action's count lies within 5 binomial standard deviations of N softmax_a — a
    condition derived from N (a fair sampler fails it with probability < 6e-7 per action)."""
    n, T_ = 4096, 16
    h = make(kind, n, _lib.RNG_PHILOX, seed0=77, is_discrete=1)
    D = h.obs_dim
    W = np.random.RandomState(A).uniform(-0.4, 0.4, size=(D, A))
    h.reset()
    out = h.rollout_policy(T_, W, per_env=False, obs_mean=np.full(D, -1000.0), obs_std=np.ones(D), clip_obs=1.0, sample=True, want=("actions",))
    score = W.sum(0)
    p = np.exp(score - score.max()); p /= p.sum()
    Ntot = n * T_
    counts = np.bincount(out["actions"].reshape(-1), minlength=A)
    assert counts.sum() == Ntot and len(counts) == A
    sd = np.sqrt(Ntot * p * (1 - p))
    print("counts", counts, "expected", Ntot * p, "deviations in sd", (counts - Ntot * p) / sd)
    assert (np.abs(counts - Ntot * p) <= 5 * sd).all()
    h.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _call(h, T_, pol):
    return h._lib.srlhip_rollout_policy_sampled(h._h, T_, pol, None, None, None, None)


def _pol(W, **kw):
    p = _lib.LinearPolicy()
    p.struct_size, p.per_env, p.weights, p.clip_obs = ctypes.sizeof(_lib.LinearPolicy), 1, W.ctypes.data, 10.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


CONTINUOUS = [("mobile_continuous", _lib.ENV_MOBILE, dict(is_discrete=0), "discrete"),
              ("kuka_continuous", _lib.ENV_KUKA_BUTTON, dict(is_discrete=0), "discrete"),
              ("kuka_joint_actions", _lib.ENV_KUKA_BUTTON, dict(is_discrete=0, action_joints=1), "discrete")]


@pytest.mark.parametrize("name,kind,kw,word", REFUSALS + CONTINUOUS, ids=[r[0] for r in REFUSALS + CONTINUOUS])
def test_refusals_name_what_they_refuse_and_leave_the_handle_usable(name, kind, kw, word):
    n = 5
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.rng_mode, cfg.seed0 = n, _lib.RNG_PHILOX, 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = _lib.Handle(cfg)
    host_rand = np.full((n, h.reset_rand_count), 0.5) if cfg.rng_mode == _lib.RNG_HOST else None
    h.reset(host_rand=host_rand)
    W = np.zeros((n, 32, 8))                          # larger than any policy shape: never read
    assert _call(h, 4, _pol(W)) == -95
    assert word in h.last_error(), h.last_error()
    assert h.last_error().startswith("rollout_policy_sampled:"), h.last_error()
    plain = h._lib.srlhip_rollout_policy(h._h, 4, _pol(W), None, None, None, None)
    if (name, kind, kw, word) in REFUSALS:             # worded alike: the plain call's message under the other prefix
        msg = h.last_error()
        assert plain == -95 and msg.startswith("rollout_policy:")
        assert _call(h, 4, _pol(W)) == -95 and h.last_error() == "rollout_policy_sampled:" + msg[len("rollout_policy:"):]
    else:
        assert plain == 0                              # the plain call takes the continuous modes
    h.close()


def test_host_pointer_validation_returns_einval_and_leaves_the_handle_usable():
    n = 7
    h = make(0, n, _lib.RNG_PHILOX, seed0=1)
    h.reset()
    W = weights_for(h, True, 2)
    ok = np.array([0.1, 0.2]), np.array([1.0, 2.0])
    assert _call(h, 4, _pol(W, struct_size=8)) == -22 and "struct_size" in h.last_error()
    assert _call(h, 4, None) == -22 and "null policy" in h.last_error()
    assert _call(h, 0, _pol(W)) == -22 and "T must be positive" in h.last_error()
    assert _call(h, 4, _pol(W, weights=None)) == -22 and "weights" in h.last_error()
    assert _call(h, 4, _pol(W, normalize=1, obs_mean=ok[0].ctypes.data)) == -22
    for bad in (np.array([1.0, 0.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])):
        assert _call(h, 4, _pol(W, normalize=1, obs_mean=ok[0].ctypes.data, obs_std=bad.ctypes.data)) == -22, bad
        assert "obs_std" in h.last_error() and h.last_error().startswith("rollout_policy_sampled:")
    Wb = W.copy(); Wb[3, 1, 2] = np.nan
    assert _call(h, 4, _pol(Wb)) == -22 and "weights" in h.last_error()
    h.step_async(np.zeros(n, np.int32))
    assert _call(h, 4, _pol(W)) == -22 and "pending" in h.last_error()
    h.step_wait()
    g = make(0, n, _lib.RNG_PHILOX, seed0=1)
    g.reset(); g.step(np.zeros(n, np.int32))
    a, b = h.rollout_policy(40, W, sample=True), g.rollout_policy(40, W, sample=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    h.close(); g.close()


# ---- ARS end to end ------------------------------------------------------------------------------------------------------------------------
def test_ars_trains_with_fused_sampling():
    from rl_baselines.evolution_strategies.ars import ARSModel
    P = 4

    def run():
        a = argparse.Namespace(env="MobileRobotGymEnv-v0", num_population=P, top_population=2, step_size=0.02, exploration_noise=0.5,
                               algo_type="v1", max_step_amplitude=10, deterministic=False, continuous_actions=False, fused_rollout=True,
                               fused_sampling=True, num_timesteps=3000, seed=1, srl_model="ground_truth", num_stack=1,
                               num_cpu=2 * P, log_dir=None)
        steps = []
        m = ARSModel().train(a, callback=lambda l, g: steps.append((l["step"] - l["step0"], l["live_rows"])))
        return m, steps

    m, steps = run()
    assert len(m.history) == 2 and m.M.shape == (2, 4) and np.isfinite(m.M).all()
    assert np.any(m.M != 0), "M moves"
    for d, live_rows in steps:
        assert d == P * live_rows and 1 <= live_rows <= 252
    m2, _ = run()
    assert np.array_equal(m.M.view(np.uint64), m2.M.view(np.uint64)) and m.history == m2.history
