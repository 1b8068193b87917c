"""GPU checks of the SAMPLED fused MLP-policy rollout (srlhip_rollout_mlp_policy_sampled): the MobileRobot family and the full-model
Kuka envs, discrete actions.

Every rollout case checks three things on the same run, as tests/test_gpu_mlp_policy_rollout.py does:
  1. sampling  for every (t, env) the float64 numpy MLP is applied to the recorded previous raw observation and the recorded action is
               held to the interval rule of tests/mlp_sample_ref.py (rho = expm1(2 max_k tol_k) + 2^-48; u from the env's action stream
               at counter c0 + t).  Frozen entries are exactly -1.  Prints how many live steps numpy decides differently at rho = 0.
               Condition on the inputs (asserted: "choose another parameter seed"): at least 5 % of the live steps record another
               action than argmax(score) — otherwise a kernel that ignored u would pass.  The seeds are the ones
               tests/mlp_sample_closed_loop.py found on the CPU.  No step is excluded.
               (The 1 ulp of the device exp behind the 2^-48 is the device library's documented figure; nothing here measures it.)
  2. dynamics  a second handle with the same seed, run through srlhip_rollout with the recorded actions as the GIVEN plane, is
               bit-identical: planes, episode statistics, final state; the env streams continue identically afterwards;
  3. oracle    the CPU oracle with the recorded actions: MobileRobot bit for bit; Kuka reward / done bit for bit and
               |obs - oracle| <= 1e-4 on EVERY step, and no compared step carries the IK conditioning flag.
Shapes: MobileRobot n = 1 / 65 / 257, T = 300 (crosses the 251-step limit: auto-reset and freeze); Kuka n = 1 / 5 / 9, T = 24;
H = 5 / 100 / 128.  Then the counter semantics, equalities between surfaces, refusals and CMA-ES."""
import argparse
import ctypes

import numpy as np
import pytest

import kuka_mlp_closed_loop as kcl
import mlp_policy_ref as ref
import mlp_sample_closed_loop as scl
import mlp_sample_ref as sref
from oracle import clib
from srlhip import _lib
from test_gpu_policy_rollout import KUKA_FIELDS, REFUSALS, STATE_FIELDS, make, state_of

pytestmark = pytest.mark.gpu

T = scl.MOBILE_T
KEYS = ("obs", "reward", "done", "actions")
MOBILE_SEED, KUKA_SEED = 4000, 5000          # parameter seeds: tests/mlp_sample_closed_loop.py, the first candidates that qualify


def dims(h):
    return h.obs_dim, h.num_actions


def params_for(h, H, per_env, seed):
    return ref.random_params(seed, (h.num_envs, h.mlp_param_count(H)) if per_env else (h.mlp_param_count(H),))


def check_sampling(h, seeds, c0, obs0, out, W, H, freeze, mean=None, std=None, clip=10.0, need_frozen=False, need_off_argmax=True):
    n = h.num_envs
    D, A = dims(h)
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    score, S = ref.forward(W, ref.normalise(prev, mean, std, clip), D, H, A)          # [T][N][A]
    done = (out["done"] & 1) != 0
    seen_before = np.concatenate([np.zeros((1, n), bool), np.cumsum(done, 0)[:-1] > 0], 0)
    frozen = seen_before if freeze else np.zeros_like(seen_before)
    if need_frozen:
        assert frozen.any(), "the case must freeze somebody"
    act = out["actions"]
    u = sref.draws(seeds, c0, len(act))
    ok, differs = sref.sample_check(score, S, u, act, frozen)
    live = ~frozen
    off = float((act != score.argmax(2))[live].mean())
    print("sampling check: {} of {} live steps decided differently by numpy at rho = 0; {:.1%} off the argmax".format(
        int(differs.sum()), int(live.sum()), off))
    assert np.all(act[frozen] == -1), "frozen envs take -1"
    assert ok.all(), "the interval rule fails on {} entries".format(int((~ok).sum()))
    if need_off_argmax:
        assert off >= scl.MIN_OFF_ARGMAX, "condition on the inputs: choose another parameter seed"
    return frozen


@pytest.mark.parametrize("kind,rng,n,H,per_env,normalize,freeze", scl.MOBILE_CASES)
def test_mobile_sampled_rollout_sampling_dynamics_oracle(kind, rng, n, H, per_env, normalize, freeze):
    rng_mode, seed0 = getattr(_lib, "RNG_" + rng), scl.MOBILE_ENV_SEED
    kw = dict(is_discrete=1, random_target=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = scl.mobile_params((kind, rng, n, H, per_env, normalize, freeze), MOBILE_SEED)
    assert W.shape[-1] == h.mlp_param_count(H)
    mean = std = None
    if normalize:
        mean, std = scl.MOBILE_MEAN[:h.obs_dim], scl.MOBILE_STD[:h.obs_dim]
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T, W, H, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std,
                               clip_obs=scl.MOBILE_CLIP, sample=True)
    assert (out["done"] & 1).any(0).all()              # every env crosses the 251-step limit at the latest
    # 1. sampling
    check_sampling(h, seed0 + np.arange(n), 0, obs0, out, W, H, freeze, mean, std, scl.MOBILE_CLIP, need_frozen=bool(freeze))
    # 2. dynamics against the existing GIVEN path
    g = make(kind, n, rng_mode, seed0=seed0, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(T, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    sa, sb = state_of(h), state_of(g)
    for f in STATE_FIELDS:
        assert np.array_equal(sa[f], sb[f]), f
    for a, b in zip(h.episode_stats(), g.episode_stats()):
        assert np.array_equal(a, b)
    acts = np.random.RandomState(9).randint(h.num_actions, size=(40, n)).astype(np.int32)
    assert np.array_equal(h.rollout(40, actions=acts)["obs"], g.rollout(40, actions=acts)["obs"])       # the env streams continue identically
    # 3. the CPU oracle with the recorded actions
    ora = clib.mobile_rollout(kind, seed0 + np.arange(n), T, actions=out["actions"], is_discrete=True, random_target=True,
                              rng_mode=getattr(clib, "RNG_" + rng))
    assert np.array_equal(ora["obs0"], obs0)
    for k in ("obs", "reward", "done"):
        assert np.array_equal(ora[k], out[k]), "oracle " + k
    h.close(); g.close()


@pytest.mark.parametrize("case", scl.KUKA_CASES)
def test_kuka_sampled_rollout_sampling_dynamics_oracle(case):
    env, discrete, joints, rng, n, H, per_env, normalize, freeze = case
    kind, rng_mode = getattr(_lib, "ENV_" + env), getattr(_lib, "RNG_" + rng)
    kw = dict(is_discrete=1, info_bits=1)
    h = make(kind, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    assert bool(h.cfg.force_down) == kcl.ENV_KW[env]["force_down"] and h.cfg.max_distance == kcl.ENV_KW[env]["max_distance"]
    W = kcl.params_for(case, KUKA_SEED)
    assert W.shape[-1] == h.mlp_param_count(H)
    mean, std = (kcl.MEAN, kcl.STD) if normalize else (None, None)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(kcl.T, W, H, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std,
                               clip_obs=kcl.CLIP, sample=True)
    check_sampling(h, kcl.ENV_SEED + np.arange(n), 0, obs0, out, W, H, freeze, mean, std, kcl.CLIP)
    g = make(kind, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(kcl.T, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    for f in KUKA_FIELDS:
        assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    acts = np.random.RandomState(9).randint(6, size=(8, n)).astype(np.int32)
    assert np.array_equal(h.rollout(8, actions=acts)["obs"], g.rollout(8, actions=acts)["obs"])         # the env streams continue identically
    h.close(); g.close()
    assert not ((out["done"] >> 1) & 1).any(), "an IK conditioning flag: the parameter seed is wrong (tests/mlp_sample_closed_loop.py)"
    ora = kcl.oracle_rollout(case, out["actions"], kcl.T)
    err = np.abs(out["obs"] - ora["obs"]).max()
    print("oracle check: max |obs - oracle| = {:.3g}".format(float(err)))
    assert np.array_equal(ora["obs0"], obs0)
    assert np.array_equal(ora["reward"], out["reward"])
    assert np.array_equal(ora["done"], out["done"] & 1)
    assert err <= 1e-4


def test_kuka_sampled_rollout_freezes_after_the_episode_limit():
    """KukaButton ends an episode inside a short call only at its 1001-step limit, so this case runs T = 1010 on n = 5: every env
    reports done, is auto-reset and then takes -1 for the remaining steps, while its draws go on being consumed.  Sampling and `None`
    encoding against numpy, dynamics bit for bit against srlhip_rollout.  No oracle comparison here: the 1010-step closed loop was not
    searched for a flag-free seed (as in the deterministic suite)."""
    n, T_, H = 5, 1010, 100
    kw = dict(is_discrete=1, info_bits=1)
    h = make(_lib.ENV_KUKA_BUTTON, n, _lib.RNG_PHILOX, seed0=kcl.ENV_SEED, **kw)
    W = params_for(h, H, True, 3100)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T_, W, H, freeze_after_done=True, sample=True)
    assert (out["done"] & 1).any(0).all()
    frozen = check_sampling(h, kcl.ENV_SEED + np.arange(n), 0, obs0, out, W, H, True, need_frozen=True)
    assert frozen[-1].all() and frozen.sum() >= n * (T_ - 1001)
    g = make(_lib.ENV_KUKA_BUTTON, n, _lib.RNG_PHILOX, seed0=kcl.ENV_SEED, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(T_, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    for f in KUKA_FIELDS:
        assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    # the counter stands at c0 + T although every env was frozen at the end
    nxt = h.rollout_mlp_policy(1, W, H, sample=True)
    score, S = ref.forward(W, out["obs"][-1], 3, H, 6)
    ok, _ = sref.sample_check(score, S, sref.draws(kcl.ENV_SEED + np.arange(n), T_, 1)[0], nxt["actions"][0])
    assert ok.all()
    h.close(); g.close()


# ---- counter semantics -------------------------------------------------------------------------------------------------------------------
def _fresh(kind, n, seed0, rng_mode=_lib.RNG_PHILOX, **kw):
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    return h, h.reset()


@pytest.mark.parametrize("kind,n", [(0, 65), (_lib.ENV_KUKA_BUTTON, 9)])
def test_chunked_calls_equal_one_call_and_null_planes(kind, n):
    H = 100
    (a, _), (b, _) = _fresh(kind, n, 31), _fresh(kind, n, 31)
    W = params_for(a, H, True, 41)
    whole = a.rollout_mlp_policy(24, W, H, sample=True)
    first = b.rollout_mlp_policy(10, W, H, want=("done",), sample=True)
    assert first["obs"] is None and first["reward"] is None and first["actions"] is None
    rest = b.rollout_mlp_policy(14, W, H, sample=True)
    assert np.array_equal(first["done"], whole["done"][:10])
    for k in KEYS:
        assert np.array_equal(rest[k], whole[k][10:]), k
    assert b._lib.srlhip_rollout_mlp_policy_sampled(b._h, 4, _pol(W, H), None, None, None, None) == 0      # every plane NULL
    a.close(); b.close()


@pytest.mark.parametrize("kind,n,per_step", [(0, 65, 1), (3, 5, 1), (_lib.ENV_KUKA_BUTTON, 5, 1)])
def test_sampled_call_continues_the_synthetic_agents_stream_and_seed_restarts_it(kind, n, per_step):
    """rollout(40) with device-sampled actions moves the env's action-stream counter by 40 in both families with discrete actions
    (csrc/mobile.hip: mobile_rollout_k's `rs.act_ctr[e] += T`, a count of actions; csrc/kuka_tree_kernels.hpp: GroupActions::next, one
    block per action) — the sampled call that follows draws at counters 40, 41, ...; a second one goes on at 40 + T; srlhip_seed
    restarts the stream at 0."""
    H, T_, seed0 = 100, 24, 12
    h, _ = _fresh(kind, n, seed0, random_target=1) if kind < _lib.ENV_KUKA_BUTTON else _fresh(kind, n, seed0)
    W = params_for(h, H, True, 43)
    seeds = seed0 + np.arange(n)
    D, A = dims(h)
    c = 40 * per_step
    last = h.rollout(40)["obs"][-1]
    for _ in range(2):
        out = h.rollout_mlp_policy(T_, W, H, sample=True)
        prev = np.concatenate([last[None], out["obs"][:-1]], 0)
        score, S = ref.forward(W, prev.astype(np.float32), D, H, A)
        u = sref.draws(seeds, c, T_)
        ok, _ = sref.sample_check(score, S, u, out["actions"])
        assert ok.all(), c
        wrong, _ = sref.sample_check(score, S, sref.draws(seeds, c + 1, T_), out["actions"])
        assert not wrong.all(), "the check must tell one counter from the next"
        c += T_
        last = out["obs"][-1]
    # ... and the synthetic agent goes on where the sampled calls left the counter
    g, _ = _fresh(kind, n, seed0, random_target=1) if kind < _lib.ENV_KUKA_BUTTON else _fresh(kind, n, seed0)
    ref_acts = g.rollout(40 + 2 * T_ + 8)["actions"]
    assert np.array_equal(h.rollout(8)["actions"], ref_acts[40 + 2 * T_:])
    g.close()
    h.seed(seeds)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T_, W, H, sample=True)
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    score, S = ref.forward(W, prev.astype(np.float32), D, H, A)
    ok, _ = sref.sample_check(score, S, sref.draws(seeds, 0, T_), out["actions"])
    assert ok.all()
    h.close()


def test_counter_advances_by_T_when_every_env_is_frozen_from_step_one():
    """Step counters set to 250: every MobileRobot env reports done at its first step (`done = counter > 250`), so with
    freeze_after_done it is frozen from step 1 on; the next call still draws at c0 + T"""
    n, H, T_, seed0 = 65, 100, 20, 3
    h, _ = _fresh(0, n, seed0, random_target=1)
    h.set_state(_lib.F_STEP_COUNT, np.full(n, 250, np.int32))
    W = params_for(h, H, True, 44)
    out = h.rollout_mlp_policy(T_, W, H, freeze_after_done=True, sample=True)
    assert (out["done"][0] & 1).all() and np.all(out["actions"][1:] == -1) and np.all(out["actions"][0] >= 0)
    nxt = h.rollout_mlp_policy(1, W, H, sample=True)
    score, S = ref.forward(W, out["obs"][-1], 2, H, 4)
    seeds = seed0 + np.arange(n)
    ok, _ = sref.sample_check(score, S, sref.draws(seeds, T_, 1)[0], nxt["actions"][0])
    assert ok.all()
    wrong, _ = sref.sample_check(score, S, sref.draws(seeds, 1, 1)[0], nxt["actions"][0])       # had the frozen draws been skipped
    assert not wrong.all()
    h.close()


# ---- equalities --------------------------------------------------------------------------------------------------------------------------
def _run(kind, n, rng_mode, seed, H, wseed, T_, **kw):
    h = make(kind, n, rng_mode, seed0=seed, **kw)
    W = params_for(h, H, True, wseed)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T_, W, H, freeze_after_done=True, sample=True)
    h.close()
    return obs0, out, W


@pytest.mark.parametrize("kind,n,T_", [(0, 65, T), (_lib.ENV_KUKA_2BUTTON, 5, 24)])
def test_two_handles_seeded_alike_give_identical_bits(kind, n, T_):
    a = _run(kind, n, _lib.RNG_PHILOX, 12, 100, 70, T_)
    b = _run(kind, n, _lib.RNG_PHILOX, 12, 100, 70, T_)
    assert np.array_equal(a[0], b[0])
    for k in KEYS:
        assert np.array_equal(a[1][k].view(np.uint8), b[1][k].view(np.uint8)), k
    det = make(kind, n, _lib.RNG_PHILOX, seed0=12)
    det.reset()
    assert not np.array_equal(det.rollout_mlp_policy(T_, a[2], 100, freeze_after_done=True)["actions"], a[1]["actions"])       # it does sample
    det.close()


def test_sharded_host_vec_env_equals_single_handle():
    from srlhip.vec_env import HipVecEnv
    n, seed, H = 65, 4, 100
    env = HipVecEnv("MobileRobotGymEnv-v0", n, seed=seed, env_kwargs={"srl_model": "ground_truth"}, device_ids=[0, 0, 0, 0], rng_mode="mt19937")
    obs0, want, W = _run(0, n, _lib.RNG_MT19937, seed, H, 8, T)
    assert np.array_equal(env.reset(), obs0)
    out = env.rollout_mlp_policy(T, W, H, freeze_after_done=True, sample=True)
    for k in KEYS:
        assert np.array_equal(out[k], want[k]), k
    env.close()


@pytest.mark.parametrize("name,n", [("MobileRobotGymEnv-v0", 65), ("KukaButtonGymEnv-v0", 9)])
def test_device_vec_env_equals_handle_and_graph_replays_twice(name, n):
    import torch
    from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize
    T_, seed, H = 24, 9, 100
    env = DeviceVecEnv(name, n, seed=seed, rng_mode="philox")
    mirror = make(env.cfg.env_kind, n, _lib.RNG_PHILOX, seed0=seed)
    W = params_for(mirror, H, True, 77)
    Wd = torch.as_tensor(W, device=env.device)
    D = env.h.obs_dim

    def same(out, want, tag):
        for k in KEYS:
            assert np.array_equal(out[k].cpu().numpy(), want[k]), tag + " " + k

    with torch.cuda.stream(env.torch_stream):
        o0 = env.reset().clone()
        out = env.rollout_mlp_policy(T_, Wd, H, freeze_after_done=True, sample=True)
    env.torch_stream.synchronize()
    assert np.array_equal(o0.cpu().numpy(), mirror.reset())
    same(out, mirror.rollout_mlp_policy(T_, W, H, freeze_after_done=True, sample=True), "on stream")
    same(env.rollout_mlp_policy(T_, Wd, H, sample=True), mirror.rollout_mlp_policy(T_, W, H, sample=True), "off stream")
    # graph capture: replaying twice equals two direct calls
    bufs = (torch.zeros((T_, n, D), dtype=torch.float32, device=env.device), torch.zeros((T_, n), dtype=torch.float32, device=env.device),
            torch.zeros((T_, n), dtype=torch.uint8, device=env.device), torch.zeros((T_, n), dtype=torch.int32, device=env.device))
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_mlp_policy(T_, Wd.data_ptr(), H, True, False, out=tuple(b.data_ptr() for b in bufs), sample=True)
    g = h.graph_end()
    for rep in range(2):
        h.graph_launch(g)
        h.sync()
        same(dict(zip(KEYS, bufs)), mirror.rollout_mlp_policy(T_, W, H, sample=True), "graph replay %d" % rep)
    h.graph_destroy(g)
    # wrappers
    same(DeviceVecFrameStack(env, 1).rollout_mlp_policy(4, Wd, H, sample=True), mirror.rollout_mlp_policy(4, W, H, sample=True), "stack of 1")
    with pytest.raises(NotImplementedError):
        DeviceVecFrameStack(env, 4).rollout_mlp_policy(4, Wd, H, sample=True)
    norm = DeviceVecNormalize(env, training=False, norm_reward=False, clip_obs=1.5)
    m, v = np.array([-0.3, 0.45, 0.1])[:D], np.array([0.49, 3.61, 0.3])[:D]
    norm.obs_rms.mean, norm.obs_rms.var = torch.tensor(m, dtype=torch.float64, device=env.device), torch.tensor(v, dtype=torch.float64, device=env.device)
    same(norm.rollout_mlp_policy(T_, Wd, H, freeze_after_done=True, sample=True),
         mirror.rollout_mlp_policy(T_, W, H, freeze_after_done=True, obs_mean=m, obs_std=np.sqrt(v + norm.epsilon), clip_obs=1.5, sample=True), "normalised")
    count0 = float(norm.obs_rms.count)
    norm.training = True
    out = norm.rollout_mlp_policy(T_, Wd, H, freeze_after_done=True, sample=True)
    done = (out["done"].cpu().numpy() & 1) != 0
    live_rows = int((np.concatenate([np.zeros((1, n), int), np.cumsum(done, 0)[:-1]], 0) == 0).sum())
    assert float(norm.obs_rms.count) == count0 + live_rows      # updated once, from the rows up to and including each env's first done
    env.close(); mirror.close()


def test_persistent_handle_parks_and_resumes_around_the_call():
    n, H = 64, 100
    hs = [make(0, n, _lib.RNG_PHILOX, seed0=6, random_target=1) for _ in range(2)]
    W = params_for(hs[0], H, True, 11)
    acts = np.random.RandomState(3).randint(4, size=(6, n)).astype(np.int32)
    hs[0].set_persistent(True)
    res = []
    for h in hs:
        r = [h.reset()]
        for t in range(3):
            r += [x.copy() for x in h.step(acts[t])]
        pol = h.rollout_mlp_policy(T, W, H, sample=True)
        r += [pol[k] for k in KEYS]
        for t in range(3, 6):
            r += [x.copy() for x in h.step(acts[t])]
        res.append(r)
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for h in hs:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
PREFIX = "rollout_mlp_policy_sampled:"


def _call(h, T_, pol):
    return h._lib.srlhip_rollout_mlp_policy_sampled(h._h, T_, pol, None, None, None, None)


def _pol(W, H, **kw):
    p = _lib.MlpPolicy()
    p.struct_size, p.per_env, p.params, p.clip_obs, p.hidden = ctypes.sizeof(_lib.MlpPolicy), 1, W.ctypes.data, 10.0, H
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kind,kw", [(0, dict(is_discrete=0)), (3, dict(is_discrete=0)), (_lib.ENV_KUKA_BUTTON, dict(is_discrete=0)),
                                     (_lib.ENV_KUKA_BUTTON, dict(is_discrete=0, action_joints=1)),
                                     (_lib.ENV_KUKA_2BUTTON, dict(is_discrete=0, action_joints=1))])
def test_continuous_handles_are_refused_by_name(kind, kw):
    n = 5
    h = make(kind, n, _lib.RNG_PHILOX, seed0=2, **kw)
    before = h.reset()
    W = np.zeros((n, 4096), np.float32)               # never read
    assert _call(h, 4, _pol(W, 100)) == -95
    assert "discrete" in h.last_error() and h.last_error().startswith(PREFIX), h.last_error()
    assert h.reset().shape == before.shape            # the refusal left the handle usable
    assert h._lib.srlhip_rollout_mlp_policy(h._h, 4, _pol(np.zeros((n, h.mlp_param_count(100)), np.float32), 100), None, None, None, None) == \
        (-95 if kw.get("action_joints") and kind == _lib.ENV_KUKA_2BUTTON else 0)                 # the deterministic call is as it was
    h.close()


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
    W = np.zeros((n, 4096), np.float32)               # never read
    assert _call(h, 4, _pol(W, 100)) == -95
    assert word in h.last_error() and h.last_error().startswith(PREFIX), h.last_error()
    again = h.reset(host_rand=host_rand)              # the refusal left the handle usable
    assert again.shape == before.shape
    if cfg.rng_mode != _lib.RNG_HOST:
        o, r, d = h.step(np.zeros(n, np.int32))
        assert d.shape == (n,) and np.isfinite(r).all()
    h.close()


def test_host_pointer_validation_returns_einval_and_leaves_the_handle_usable():
    n, H = 7, 100
    h = make(0, n, _lib.RNG_PHILOX, seed0=1)
    h.reset()
    W = params_for(h, H, True, 2)
    big = np.zeros((n, 2048), np.float32)              # larger than any parameter block: hidden = 128 still reads inside it
    ok = np.array([0.1, 0.2]), np.array([1.0, 2.0])

    def einval(pol, word, T_=4):
        assert _call(h, T_, pol) == -22
        assert word in h.last_error() and h.last_error().startswith(PREFIX), h.last_error()

    einval(_pol(W, H, struct_size=48), "struct_size")
    einval(_pol(W, H), "T must be positive", T_=0)
    for bad in (0, -1, 129):
        einval(_pol(big, bad), "hidden")
    assert _call(h, 4, _pol(big, 1)) == 0 and _call(h, 4, _pol(big, 128)) == 0
    einval(_pol(W, H, reserved=1), "reserved")
    einval(_pol(W, H, params=None), "params")
    einval(_pol(W, H, normalize=1, obs_mean=ok[0].ctypes.data), "obs_mean and obs_std")
    for bad in (np.array([1.0, 0.0]), np.array([-1.0, 1.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])):
        einval(_pol(W, H, normalize=1, obs_mean=ok[0].ctypes.data, obs_std=bad.ctypes.data), "obs_std")
    nan_mean = np.array([np.nan, 0.0])
    einval(_pol(W, H, normalize=1, obs_mean=nan_mean.ctypes.data, obs_std=ok[1].ctypes.data), "obs_mean")
    for v in (np.nan, np.inf):
        Wb = W.copy(); Wb[3, 17] = v
        einval(_pol(Wb, H), "params")
    h.step_async(np.zeros(n, np.int32))
    einval(_pol(W, H), "pending")
    h.step_wait()
    # ... and the handle still equals one that made the same successful calls only: no failed call drew from the action stream
    g = make(0, n, _lib.RNG_PHILOX, seed0=1)
    g.reset()
    assert _call(g, 4, _pol(big, 1)) == 0 and _call(g, 4, _pol(big, 128)) == 0
    g.step(np.zeros(n, np.int32))
    a, b = h.rollout_mlp_policy(T, W, H, sample=True), g.rollout_mlp_policy(T, W, H, sample=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    h.close(); g.close()


# ---- CMA-ES ------------------------------------------------------------------------------------------------------------------------------
CMA_SEED = 5


def _cma_args(env, P, num_timesteps, **kw):
    base = dict(env=env, num_population=P, mu=0.0, sigma=0.14, deterministic=False, continuous_actions=False, fused_rollout=True,
                fused_sampling=True, num_timesteps=num_timesteps, seed=CMA_SEED, srl_model="ground_truth", num_stack=1, log_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_cma_evaluate_fused_equals_the_reference_accounting_of_a_direct_sampled_rollout():
    """MobileRobot, P = 16, one generation: evaluate_fused of a stochastic discrete model returns what returns_from_planes makes of the
    planes of rollout_mlp_policy(sample=True) on a twin env — and not what the argmax rollout gives."""
    import torch
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP, CMAES, CMAESModel
    from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize
    P, H, limit = 16, 100, 252

    def build():
        env = DeviceVecEnv("MobileRobotGymEnv-v0", P, seed=CMA_SEED, rng_mode="philox")
        return DeviceVecNormalize(DeviceVecFrameStack(env, 1), norm_obs=True, norm_reward=False, training=False)

    model = CMAESModel()
    model.policy, model.deterministic, model.continuous_actions = BatchedMLP(2, 4, H), False, False
    es = CMAES(model.policy.n_params * [0.0], 0.14, P, "cuda", seed=CMA_SEED)
    population = es.ask()
    env = build()
    env.reset()
    rf, lf = model.evaluate_fused(env, population, limit)
    env.close()
    twin = build()
    twin.reset()
    w32 = population.to(torch.float32).contiguous()
    planes = twin.rollout_mlp_policy(limit, w32, H, per_env=True, freeze_after_done=True, sample=True)
    r, live = CMAESModel.returns_from_planes(planes["reward"], planes["done"])
    assert torch.equal(rf, r) and torch.equal(lf, live) and int(live.min()) >= 1
    twin.reset()
    det = twin.rollout_mlp_policy(limit, w32, H, per_env=True, freeze_after_done=True)
    assert not torch.equal(det["actions"], planes["actions"])
    twin.close()


@pytest.mark.parametrize("env,P", [("MobileRobotGymEnv-v0", 16), ("KukaButtonGymEnv-v0", 8)])
def test_cma_train_fused_sampling_runs_three_generations(env, P, tmp_path):
    """train --fused-rollout --fused-sampling, three generations: one callback per generation, finite history and best_model, every
    generation sampled, and the saved pickle acts on the host."""
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    fired, sampled = [], []

    class ThreeGenerations(CMAESModel):
        calls = 0

        def evaluate_fused(self, env_, population, T_):
            inner = env_.venv.venv
            real = inner.rollout_mlp_policy
            inner.rollout_mlp_policy = lambda *a, **kw: (sampled.append(kw.get("sample")), real(*a, **kw))[1]
            try:
                r, live = CMAESModel.evaluate_fused(self, env_, population, T_)
            finally:
                del inner.rollout_mlp_policy
            assert T_ == (252 if env.startswith("Mobile") else 1002) and tuple(r.shape) == (P,) and int(live.min()) >= 1
            self.calls += 1
            return r, live + (10 ** 9 if self.calls == 3 else 0)

    m = ThreeGenerations().train(_cma_args(env, P, 10 ** 8), callback=lambda l, g: fired.append(int(l["live"])))
    assert m.calls == 3 and len(fired) == 3 and len(m.history) == 3 and sampled == [True, True, True]
    assert m.deterministic is False
    assert np.isfinite(m.history).all() and np.isfinite(m.best_model).all() and np.abs(m.best_model).max() > 0
    path = str(tmp_path / "cma.pkl")
    m.save(path)
    loaded = CMAESModel.load(path)
    D, A = (2, 4) if env.startswith("Mobile") else (3, 6)
    act = loaded.getAction(np.zeros((2, D)))
    assert act.shape == (2,) and ((act >= 0) & (act < A)).all()
