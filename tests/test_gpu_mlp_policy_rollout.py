"""GPU checks of the fused MLP-policy rollout (srlhip_rollout_mlp_policy): the MobileRobot family and the full-model Kuka envs.

Every case checks three things on the same run:
  1. policy    for every (t, env) the float64 numpy MLP (tests/mlp_policy_ref.py) is applied to the recorded previous raw
               observation (at t = 0 the one reset() returned).  The kernel's summation order over the hidden units is its own, so
               with tol_a = 2^-44 S_a, S_a = |b2_a| + sum_j |W2[a][j]| (|b1_j| + sum_d |W1[j][d] x_d|)  (gamma_(H+D+2) <= 132 * 2^-53
               at H = 128 bounds a float64 sum of H + D + 2 terms in any order, ReLU is 1-Lipschitz, a factor 4 for the two layers and
               the comparison of two scores): a discrete action a has score[a] >= max(score) - tol and every k < a has
               score[k] < score[a] + tol; a continuous one lies in [f32(score - tol), f32(score + tol)].  Frozen envs take exactly
               the `None` encoding;
  2. dynamics  a second handle with the same seed, run through srlhip_rollout with the recorded actions as the GIVEN plane, is
               bit-identical: planes, episode statistics, final state;
  3. oracle    the CPU oracle with the recorded actions: MobileRobot bit for bit; Kuka reward / done bit for bit and
               |obs - oracle| <= 1e-4 on EVERY step — the parameter seeds are ones for which the oracle's own closed loop never
               raises the IK conditioning flag (tests/kuka_mlp_closed_loop.py), and the test asserts that no compared step carries it.
Shapes: MobileRobot n = 1 / 65 / 257 (a partial lane group's wavefront, a partial wavefront, a partial block), T = 300 (crosses the
251-step limit: auto-reset and freeze); Kuka n = 1 / 5 / 9 (four envs share a wavefront), T = 24; H = 5 / 100 / 128.
Then determinism, the surfaces, refusals and CMA-ES."""
import ctypes

import numpy as np
import pytest

import kuka_mlp_closed_loop as kcl
import mlp_policy_ref as ref
from oracle import clib
from srlhip import _lib
from test_gpu_policy_rollout import KUKA_FIELDS, REFUSALS, STATE_FIELDS, make, state_of

pytestmark = pytest.mark.gpu

T = 300
KEYS = ("obs", "reward", "done", "actions")


def dims(h):
    return h.obs_dim, (h.num_actions if h.cfg.is_discrete else h.action_dim)


def params_for(h, H, per_env, seed):
    P = h.mlp_param_count(H)
    assert P == ref.param_count(*((dims(h)[0], H, dims(h)[1])))
    return ref.random_params(seed, (h.num_envs, P) if per_env else (P,))


def check_policy(h, obs0, out, W, H, freeze, mean=None, std=None, clip=10.0, need_frozen=False):
    n = h.num_envs
    D, A = dims(h)
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    score, S = ref.forward(W, ref.normalise(prev, mean, std, clip), D, H, A)          # [T][N][A]
    tol = ref.TOL_FACTOR * S
    done = (out["done"] & 1) != 0                     # (bit 1: info_bits)
    seen_before = np.concatenate([np.zeros((1, n), bool), np.cumsum(done, 0)[:-1] > 0], 0)       # done at an EARLIER step
    frozen = seen_before if freeze else np.zeros_like(seen_before)
    if need_frozen:
        assert frozen.any(), "the case must freeze somebody"
    act = out["actions"]
    if h.cfg.is_discrete:
        assert np.all(act[frozen] == -1), "frozen envs take -1"
        live = ~frozen
        assert np.all((act[live] >= 0) & (act[live] < A))
        a = np.where(live, act, 0)
        sa = np.take_along_axis(score, a[..., None], 2)[..., 0]
        ta = np.take_along_axis(tol, a[..., None], 2)[..., 0]
        tmax = ta[..., None]                           # tol_a of the recorded action
        slack = (score.max(2) - sa) / np.maximum(ta, 1e-300)
        print("policy check: max (max(score) - score[a]) / tol = {:.3g}".format(float(slack[live].max())))
        assert np.all((sa >= (score - tmax).max(2))[live]), "score[a] >= max(score) - tol"
        lower = np.arange(A)[None, None, :] < a[..., None]
        assert np.all((~lower | (score < sa[..., None] + tmax))[live]), "no lower index beats a"
    else:
        if h.cfg.env_kind >= _lib.ENV_KUKA_BUTTON:
            assert np.isnan(act[frozen]).all(), "frozen Kuka envs take a row of NaNs"
        else:
            assert np.all(act[frozen] == 0.0), "frozen MobileRobot envs take a zero row"
        lo, hi = (score - tol).astype(np.float32), (score + tol).astype(np.float32)
        live = ~frozen
        print("policy check: {} of {} live entries have more than one float32 in their interval".format(int((lo != hi)[live].sum()), int(live.sum()) * A))
        assert np.all((lo <= act)[live] & (act <= hi)[live]), "f32(score - tol) <= a <= f32(score + tol)"
    return frozen


MOBILE_CASES = [
    # kind, discrete, rng, n, H, per_env, normalize, freeze
    (0, 1, "MT19937", 257, 100, 1, 0, 0),
    (0, 1, "PHILOX", 1, 5, 1, 0, 1),
    (0, 1, "PHILOX", 65, 128, 0, 1, 1),
    (1, 1, "PHILOX", 257, 128, 1, 0, 0),
    (1, 1, "MT19937", 65, 5, 1, 1, 1),
    (1, 1, "MT19937", 1, 100, 0, 0, 0),
    (2, 1, "MT19937", 257, 5, 1, 0, 1),
    (2, 1, "PHILOX", 65, 100, 0, 1, 0),
    (3, 1, "PHILOX", 257, 100, 1, 1, 1),
    (3, 1, "MT19937", 1, 128, 1, 0, 0),
    (0, 0, "PHILOX", 257, 100, 1, 0, 1),
    (0, 0, "MT19937", 65, 128, 1, 1, 0),
    (3, 0, "MT19937", 257, 5, 0, 0, 0),
    (3, 0, "PHILOX", 1, 100, 1, 1, 1),
]


@pytest.mark.parametrize("kind,discrete,rng,n,H,per_env,normalize,freeze", MOBILE_CASES)
def test_mlp_rollout_policy_dynamics_oracle(kind, discrete, rng, n, H, per_env, normalize, freeze):
    rng_mode, seed0 = getattr(_lib, "RNG_" + rng), 17
    kw = dict(is_discrete=discrete, random_target=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = params_for(h, H, per_env, 1000 + kind)
    mean = std = None
    if normalize:
        mean, std = np.array([-0.3, 0.45])[:h.obs_dim], np.array([0.7, 1.9])[:h.obs_dim]
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T, W, H, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=1.5)
    assert (out["done"] & 1).any(0).all()              # every env crosses the 251-step limit at the latest
    # 1. policy
    check_policy(h, obs0, out, W, H, freeze, mean, std, 1.5, need_frozen=bool(freeze))
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
    assert np.array_equal(h.rollout(40)["obs"], g.rollout(40)["obs"])       # the streams continue identically
    # 3. the CPU oracle with the recorded actions
    ora = clib.mobile_rollout(kind, seed0 + np.arange(n), T, actions=out["actions"], is_discrete=bool(discrete), random_target=True,
                              rng_mode=getattr(clib, "RNG_" + rng))
    assert np.array_equal(ora["obs0"], obs0)
    for k in ("obs", "reward", "done"):
        assert np.array_equal(ora[k], out[k]), "oracle " + k
    h.close(); g.close()


# parameter seeds: tests/kuka_mlp_closed_loop.py (CPU oracle, closed loop): the first of 3000, 3001, ... without an IK flag
KUKA_SEEDS = [3000, 3000, 3000, 3000, 3000, 3000, 3000, 3000, 3000, 3000]
KUKA_T = kcl.T


@pytest.mark.parametrize("case,wseed", list(zip(kcl.CASES, KUKA_SEEDS)))
def test_kuka_mlp_rollout_policy_dynamics_oracle(case, wseed):
    env, discrete, joints, rng, n, H, per_env, normalize, freeze = case
    kind, rng_mode = getattr(_lib, "ENV_" + env), getattr(_lib, "RNG_" + rng)
    kw = dict(is_discrete=discrete, action_joints=joints, info_bits=1)
    h = make(kind, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    assert bool(h.cfg.force_down) == kcl.ENV_KW[env]["force_down"] and h.cfg.max_distance == kcl.ENV_KW[env]["max_distance"]
    W = kcl.params_for(case, wseed)
    assert W.shape[-1] == h.mlp_param_count(H)
    mean, std = (kcl.MEAN, kcl.STD) if normalize else (None, None)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(KUKA_T, W, H, per_env=bool(per_env), freeze_after_done=bool(freeze), obs_mean=mean, obs_std=std, clip_obs=kcl.CLIP)
    check_policy(h, obs0, out, W, H, freeze, mean, std, kcl.CLIP)
    g = make(kind, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(KUKA_T, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    for f in KUKA_FIELDS:
        assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    h.close(); g.close()
    assert not ((out["done"] >> 1) & 1).any(), "an IK conditioning flag: the parameter seed is wrong (tests/kuka_mlp_closed_loop.py)"
    ora = kcl.oracle_rollout(case, out["actions"], KUKA_T)
    err = np.abs(out["obs"] - ora["obs"]).max()
    print("oracle check: max |obs - oracle| = {:.3g}".format(float(err)))
    assert np.array_equal(ora["obs0"], obs0)
    assert np.array_equal(ora["reward"], out["reward"])
    assert np.array_equal(ora["done"], out["done"] & 1)
    assert err <= 1e-4


@pytest.mark.parametrize("discrete,rng", [(1, "PHILOX"), (0, "MT19937")])
def test_kuka_mlp_rollout_freezes_after_the_episode_limit(discrete, rng):
    """KukaButton ends an episode inside a short call only at its 1001-step limit (no small max_distance does: 5000 steps outside
    are needed), so this case runs T = 1010 on n = 5: every env reports done, is auto-reset and then takes the `None` action — -1, or
    the all-NaN row — for the remaining steps.  Policy and `None` encoding against numpy, dynamics (the `None` steps included) bit for
    bit against srlhip_rollout.  No oracle comparison here: the 1010-step closed loop was not searched for a flag-free seed."""
    n, T_, H = 5, 1010, 100
    rng_mode = getattr(_lib, "RNG_" + rng)
    kw = dict(is_discrete=discrete, info_bits=1)
    h = make(_lib.ENV_KUKA_BUTTON, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    W = params_for(h, H, True, 3100)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T_, W, H, freeze_after_done=True)
    assert (out["done"] & 1).any(0).all()
    frozen = check_policy(h, obs0, out, W, H, True, need_frozen=True)
    assert frozen[-1].all() and frozen.sum() >= n * (T_ - 1001)
    g = make(_lib.ENV_KUKA_BUTTON, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(T_, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    for f in KUKA_FIELDS:
        assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    h.close(); g.close()


def _run(kind, n, rng_mode, seed, H, wseed, T_, **kw):
    h = make(kind, n, rng_mode, seed0=seed, **kw)
    W = params_for(h, H, True, wseed)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T_, W, H, freeze_after_done=True)
    h.close()
    return obs0, out, W


@pytest.mark.parametrize("kind,n,T_,discrete", [(0, 65, T, 0), (_lib.ENV_KUKA_BUTTON, 5, 24, 0)])
def test_two_handles_seeded_alike_give_identical_bits(kind, n, T_, discrete):
    """continuous actions: the float32 scores themselves are compared, not only their argmax"""
    a = _run(kind, n, _lib.RNG_PHILOX, 12, 100, 70, T_, is_discrete=discrete)
    b = _run(kind, n, _lib.RNG_PHILOX, 12, 100, 70, T_, is_discrete=discrete)
    assert np.array_equal(a[0], b[0])
    for k in KEYS:
        assert np.array_equal(a[1][k].view(np.uint8), b[1][k].view(np.uint8)), k


def test_sharded_host_vec_env_equals_single_handle():
    from srlhip.vec_env import HipVecEnv
    n, seed, H = 65, 4, 100
    env = HipVecEnv("MobileRobotGymEnv-v0", n, seed=seed, env_kwargs={"srl_model": "ground_truth"}, device_ids=[0, 0, 0, 0], rng_mode="mt19937")
    obs0, want, W = _run(0, n, _lib.RNG_MT19937, seed, H, 8, T)
    assert np.array_equal(env.reset(), obs0)
    out = env.rollout_mlp_policy(T, W, H, freeze_after_done=True)
    for k in KEYS:
        assert np.array_equal(out[k], want[k]), k
    env.close()


@pytest.mark.parametrize("kind,n", [(0, 65), (_lib.ENV_KUKA_BUTTON, 9)])
def test_chunked_calls_continue_and_null_planes(kind, n):
    """10 + 14 steps equal one call of 24 (the kernel recomputes the first observation from the state it loads); any plane may be
    missing"""
    H = 100
    hs = [make(kind, n, _lib.RNG_PHILOX, seed0=31) for _ in range(2)]
    W = params_for(hs[0], H, True, 41)
    for h in hs:
        h.reset()
    whole = hs[0].rollout_mlp_policy(24, W, H)
    a = hs[1].rollout_mlp_policy(10, W, H, want=("done",))
    assert a["obs"] is None and a["reward"] is None and a["actions"] is None
    b = hs[1].rollout_mlp_policy(14, W, H)
    assert np.array_equal(a["done"], whole["done"][:10])
    for k in KEYS:
        assert np.array_equal(b[k], whole[k][10:]), k
    assert hs[1]._lib.srlhip_rollout_mlp_policy(hs[1]._h, 4, _pol(W, H), None, None, None, None) == 0      # every plane NULL
    for h in hs:
        h.close()


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
        out = env.rollout_mlp_policy(T_, Wd, H, freeze_after_done=True)
    env.torch_stream.synchronize()
    assert np.array_equal(o0.cpu().numpy(), mirror.reset())
    same(out, mirror.rollout_mlp_policy(T_, W, H, freeze_after_done=True), "on stream")
    same(env.rollout_mlp_policy(T_, Wd, H), mirror.rollout_mlp_policy(T_, W, H), "off stream")
    # graph capture: replaying twice equals two direct calls
    bufs = [(torch.zeros((T_, n, D), dtype=torch.float32, device=env.device), torch.zeros((T_, n), dtype=torch.float32, device=env.device),
             torch.zeros((T_, n), dtype=torch.uint8, device=env.device), torch.zeros((T_, n), dtype=torch.int32, device=env.device))]
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_mlp_policy(T_, Wd.data_ptr(), H, True, False, out=tuple(b.data_ptr() for b in bufs[0]))
    g = h.graph_end()
    for rep in range(2):
        h.graph_launch(g)
        h.sync()
        same(dict(zip(KEYS, bufs[0])), mirror.rollout_mlp_policy(T_, W, H), "graph replay %d" % rep)
    h.graph_destroy(g)
    # wrappers
    same(DeviceVecFrameStack(env, 1).rollout_mlp_policy(4, Wd, H), mirror.rollout_mlp_policy(4, W, H), "stack of 1")
    with pytest.raises(NotImplementedError):
        DeviceVecFrameStack(env, 4).rollout_mlp_policy(4, Wd, H)
    norm = DeviceVecNormalize(env, training=False, norm_reward=False, clip_obs=1.5)
    m, v = np.array([-0.3, 0.45, 0.1])[:D], np.array([0.49, 3.61, 0.3])[:D]
    norm.obs_rms.mean, norm.obs_rms.var = torch.tensor(m, dtype=torch.float64, device=env.device), torch.tensor(v, dtype=torch.float64, device=env.device)
    same(norm.rollout_mlp_policy(T_, Wd, H, freeze_after_done=True),
         mirror.rollout_mlp_policy(T_, W, H, freeze_after_done=True, obs_mean=m, obs_std=np.sqrt(v + norm.epsilon), clip_obs=1.5), "normalised")
    count0 = float(norm.obs_rms.count)
    norm.training = True
    out = norm.rollout_mlp_policy(T_, Wd, H, freeze_after_done=True)
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
        pol = h.rollout_mlp_policy(T, W, H)
        r += [pol[k] for k in KEYS]
        for t in range(3, 6):
            r += [x.copy() for x in h.step(acts[t])]
        res.append(r)
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for h in hs:
        h.close()


def _call(h, T_, pol):
    return h._lib.srlhip_rollout_mlp_policy(h._h, T_, pol, None, None, None, None)


def _pol(W, H, **kw):
    p = _lib.MlpPolicy()
    p.struct_size, p.per_env, p.params, p.clip_obs, p.hidden = ctypes.sizeof(_lib.MlpPolicy), 1, W.ctypes.data, 10.0, H
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_host_pointer_validation_returns_einval_and_leaves_the_handle_usable():
    n, H = 7, 100
    h = make(0, n, _lib.RNG_PHILOX, seed0=1)
    h.reset()
    W = params_for(h, H, True, 2)
    big = np.zeros((n, 2048), np.float32)              # larger than any parameter block: hidden = 128 still reads inside it
    ok = np.array([0.1, 0.2]), np.array([1.0, 2.0])
    assert _call(h, 4, _pol(W, H, struct_size=48)) == -22 and "struct_size" in h.last_error()
    assert _call(h, 0, _pol(W, H)) == -22
    for bad in (0, -1, 129):
        assert _call(h, 4, _pol(big, bad)) == -22 and "hidden" in h.last_error(), bad
    assert _call(h, 4, _pol(big, 1)) == 0 and _call(h, 4, _pol(big, 128)) == 0
    assert _call(h, 4, _pol(W, H, reserved=1)) == -22 and "reserved" in h.last_error()
    assert _call(h, 4, _pol(W, H, params=None)) == -22 and "params" in h.last_error()
    assert _call(h, 4, _pol(W, H, normalize=1, obs_mean=ok[0].ctypes.data)) == -22
    for bad in (np.array([1.0, 0.0]), np.array([-1.0, 1.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])):
        assert _call(h, 4, _pol(W, H, normalize=1, obs_mean=ok[0].ctypes.data, obs_std=bad.ctypes.data)) == -22, bad
        assert "obs_std" in h.last_error()
    nan_mean = np.array([np.nan, 0.0])
    assert _call(h, 4, _pol(W, H, normalize=1, obs_mean=nan_mean.ctypes.data, obs_std=ok[1].ctypes.data)) == -22 and "obs_mean" in h.last_error()
    for v in (np.nan, np.inf):
        Wb = W.copy(); Wb[3, 17] = v
        assert _call(h, 4, _pol(Wb, H)) == -22 and "params" in h.last_error()
    h.step_async(np.zeros(n, np.int32))
    assert _call(h, 4, _pol(W, H)) == -22 and "pending" in h.last_error()
    h.step_wait()
    # ... and the handle still equals one that made the same successful calls only
    g = make(0, n, _lib.RNG_PHILOX, seed0=1)
    g.reset()
    assert _call(g, 4, _pol(big, 1)) == 0 and _call(g, 4, _pol(big, 128)) == 0
    g.step(np.zeros(n, np.int32))
    a, b = h.rollout_mlp_policy(T, W, H), g.rollout_mlp_policy(T, W, H)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    h.close(); g.close()


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
    assert word in h.last_error() and "rollout_mlp_policy" in h.last_error(), h.last_error()
    assert h.last_error().startswith("rollout_mlp_policy:"), h.last_error()
    again = h.reset(host_rand=host_rand)              # the refusal left the handle usable
    assert again.shape == before.shape
    if cfg.rng_mode != _lib.RNG_HOST:
        o, r, d = h.step(np.zeros(n, np.int32))
        assert d.shape == (n,) and np.isfinite(r).all()
    h.close()


def test_two_button_joint_space_actions_are_refused_by_name():
    """The two-button kernels have six score rows (no joints-mode instantiation); a joint-space policy has seven, so the MLP rollout
    refuses the combination instead of dropping fc_out's seventh row."""
    n = 5
    cfg = _lib.default_config(_lib.ENV_KUKA_2BUTTON)
    cfg.num_envs, cfg.rng_mode, cfg.seed0, cfg.is_discrete, cfg.action_joints = n, _lib.RNG_PHILOX, 2, 0, 1
    h = _lib.Handle(cfg)
    before = h.reset()
    W = np.zeros((n, 4096), np.float32)               # never read
    assert _call(h, 4, _pol(W, 100)) == -95
    assert "Kuka2Button" in h.last_error() and "joint-space" in h.last_error() and "rollout_mlp_policy" in h.last_error(), h.last_error()
    assert h.last_error().startswith("rollout_mlp_policy:"), h.last_error()
    assert h.reset().shape == before.shape            # the refusal left the handle usable
    h.close()


CMA_SEED = 5


def _cma_args(env, P, fused, num_timesteps, **kw):
    import argparse
    base = dict(env=env, num_population=P, mu=0.0, sigma=0.14, deterministic=True, continuous_actions=False, fused_rollout=fused,
                num_timesteps=num_timesteps, seed=CMA_SEED, srl_model="ground_truth", num_stack=1, log_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_cma_evaluate_fused_equals_a_per_step_evaluation():
    """MobileRobot, P = 16, deterministic discrete, one generation.  The per-step evaluation is written here: BatchedMLP.forward in
    float64 on population.float().double(), argmax, -1 after done, the reference's accounting (the finishing step's reward is not
    added; a member is live up to and including its first done).  Precondition, asserted first: on every live step of the per-step
    run the top-two score gap exceeds 2 tol (tol as in check_policy) — then the kernel's summation order cannot change an argmax and
    the equality is exact."""
    import torch
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP, CMAES, CMAESModel
    from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize
    P, H, limit = 16, 100, 252

    def build():
        env = DeviceVecEnv("MobileRobotGymEnv-v0", P, seed=CMA_SEED, rng_mode="philox")
        return DeviceVecNormalize(DeviceVecFrameStack(env, 1), norm_obs=True, norm_reward=False, training=False)

    model = CMAESModel()
    model.policy = BatchedMLP(2, 4, H)
    es = CMAES(model.policy.n_params * [0.0], 0.14, P, "cuda", seed=CMA_SEED)
    population = es.ask()
    p64 = population.float().double()
    # per-step
    env = build()
    obs = env.reset()
    mean, std = env.obs_rms.mean.cpu().numpy(), torch.sqrt(env.obs_rms.var + env.epsilon).cpu().numpy()
    r = torch.zeros(P, dtype=torch.float64, device="cuda")
    done = torch.zeros(P, dtype=torch.bool, device="cuda")
    live = torch.zeros(P, dtype=torch.int64, device="cuda")
    min_margin = np.inf
    for t in range(limit):
        scores = model.policy.forward(p64, obs.double())
        _, S = ref.forward(p64.cpu().numpy(), obs.cpu().numpy(), 2, H, 4)
        top2 = scores.topk(2, dim=1)
        tol = ref.TOL_FACTOR * np.take_along_axis(S, top2.indices.cpu().numpy(), 1).max(1)
        gap = (top2.values[:, 0] - top2.values[:, 1]).cpu().numpy()
        alive = ~done.cpu().numpy()
        min_margin = min(min_margin, float((gap / (2 * tol))[alive].min()) if alive.any() else np.inf)
        a = torch.where(done, torch.full((P,), -1, device="cuda"), scores.argmax(1)).to(torch.int32).contiguous()
        live += (~done).to(torch.int64)
        obs, reward, new_done = env.step(a)
        done = done | (new_done != 0)
        r += reward.to(torch.float64) * (~done).to(torch.float64)
    print("smallest top-two gap / (2 tol) on a live step: {:.3g}".format(min_margin))
    assert min_margin > 1.0, "precondition on the inputs: choose another seed"
    assert bool(done.all())
    env.close()
    # fused
    env = build()
    env.reset()
    assert np.array_equal(env.obs_rms.mean.cpu().numpy(), mean)
    rf, lf = model.evaluate_fused(env, population, limit)
    assert torch.equal(rf, r) and torch.equal(lf, live)
    env.close()


@pytest.mark.parametrize("env,P", [("MobileRobotGymEnv-v0", 16), ("KukaButtonGymEnv-v0", 8)])
def test_cma_train_fused_rollout_runs_three_generations(env, P, tmp_path):
    """train --fused-rollout, three generations (the third one reports enough live steps to end the run, whatever the episodes'
    lengths were): one callback per generation, finite history and best_model, and the saved pickle acts on the host."""
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    fired = []

    class ThreeGenerations(CMAESModel):
        calls = 0

        def evaluate_fused(self, env_, population, T_):
            r, live = CMAESModel.evaluate_fused(self, env_, population, T_)
            assert T_ == (252 if env.startswith("Mobile") else 1002) and tuple(r.shape) == (P,) and int(live.min()) >= 1
            self.calls += 1
            return r, live + (10 ** 9 if self.calls == 3 else 0)

    m = ThreeGenerations().train(_cma_args(env, P, True, 10 ** 8), callback=lambda l, g: fired.append(int(l["live"])))
    assert m.calls == 3 and len(fired) == 3 and len(m.history) == 3
    assert np.isfinite(m.history).all() and np.isfinite(m.best_model).all() and np.abs(m.best_model).max() > 0
    path = str(tmp_path / "cma.pkl")
    m.save(path)
    loaded = CMAESModel.load(path)
    D, A = (2, 4) if env.startswith("Mobile") else (3, 6)
    act = loaded.getAction(np.zeros((2, D)))
    assert act.shape == (2,) and ((act >= 0) & (act < A)).all()
