"""The fused policy rollouts held to their arithmetic contract (include/srlhip.h) bit for bit: srlhip_rollout_policy and
srlhip_rollout_mlp_policy on dyadic parameters (tests/policy_exact.py), for which every float64 summation order, fused or not, gives
the same bits — so the recorded action of every exact (t, env, a) has to EQUAL numpy's: np.argmax with its lowest-index-first ties
(duplicated action rows tie on every step, all-zero blocks and all-dead hidden layers tie everywhere), (float)score by bit pattern
(the sign of a zero included).  Every case asserts
  1. exact     on the triples order_free passes — all but at most 1 %, asserted; tests/test_policy_exact_cpu.py runs the same cases
               against the CPU oracle alone — actions == expectation, bit for bit;
  2. the rest  the tolerance form of the policy check of tests/test_gpu_policy_rollout.py / test_gpu_mlp_policy_rollout.py, on every triple;
  3. replay    a second handle, run through srlhip_rollout with the recorded actions as the GIVEN plane, is bit-identical: a wrong
               action cannot hide behind consistent dynamics;
  4. inputs    normalised cases reach +clip, -clip and the interior; tie cases tie; Kuka cases carry no IK conditioning flag.
Shapes: MobileRobot linear T = 32, n = 70 (one lane per env: a partial wavefront); MobileRobot MLP n = 21 (four envs per wavefront: a
partial row group, a partial wavefront) and n = 17 (the shadow lanes of envs >= n), H = 1 / 15 / 16 / 17 / 33 / 128 (hidden unit l + 16 u
sits on lane l); Kuka T = 12, n = 5 / 9, H = 1 / 17 / 128."""
import numpy as np
import pytest

import kuka_mlp_closed_loop as kcl
import policy_exact as pe
import test_gpu_mlp_policy_rollout as mlp_checks
import test_gpu_policy_rollout as linear_checks
from srlhip import _lib
from test_gpu_policy_rollout import KUKA_FIELDS, STATE_FIELDS, make, state_of

pytestmark = pytest.mark.gpu


def check_exact(h, obs0, out, params, hidden, per_env, norm, want_ties=False, want_ties_off0=False):
    discrete = bool(h.cfg.is_discrete)
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    score, exact, want = pe.expected(prev, params, discrete, hidden, per_env, *norm)
    act = out["actions"]
    if discrete:
        exact = exact.all(-1)
        assert act.dtype == np.int32 and want.dtype == np.int32
    else:
        assert act.dtype == np.float32 and want.dtype == np.float32
    share = 1.0 - exact.mean()
    wrong = pe.bits(act)[exact] != pe.bits(want)[exact]
    ties, off0 = pe.tie_stats(score, np.ones(score.shape[:2], bool))
    print("exact check: share of non-exact triples {:.4f}; {} of {} exact triples differ; {} tied env-steps, {} of them off index 0".format(
        share, int(wrong.sum()), int(exact.sum()), ties, off0))
    assert share <= pe.MAX_SHARE
    assert not wrong.any(), "first differing triples (t, env[, a]): {}".format(np.argwhere((pe.bits(act) != pe.bits(want)) & exact)[:5].tolist())
    if discrete and want_ties:
        assert ties > 0
    if discrete and want_ties_off0:
        assert off0 > 0
    if norm[0] is not None:
        assert pe.clamp_sides(prev, *norm) == (True, True, True), "+clip, -clip and the interior all have to occur"
    return score, want


def replay(h, kind, n, rng_mode, seed0, kw, obs0, out, T, fields):
    g = make(kind, n, rng_mode, seed0=seed0, **kw)
    assert np.array_equal(g.reset(), obs0)
    given = g.rollout(T, actions=out["actions"])
    for k in ("obs", "reward", "done"):
        assert np.array_equal(given[k], out[k]), k
    if fields is STATE_FIELDS:
        sa, sb = state_of(h), state_of(g)
        for f in fields:
            assert np.array_equal(sa[f], sb[f]), f
    else:
        for f in fields:
            assert np.array_equal(h.get_state(getattr(_lib, f)), g.get_state(getattr(_lib, f))), f
    g.close()


def ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


@pytest.mark.parametrize("case", pe.MOBILE_LINEAR, ids=ids(pe.MOBILE_LINEAR))
def test_mobile_linear_policy_actions_equal_numpy_bit_for_bit(case):
    kind, discrete, rng, n, per_env, normalize, what, seed = case
    rng_mode, seed0, T = getattr(_lib, "RNG_" + rng), 17, pe.MOBILE_T
    kw = dict(is_discrete=discrete, random_target=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = pe.mobile_linear_params(case)
    assert W.shape == h.policy_shape(per_env)
    norm = pe.norm_of(normalize, pe.MOBILE_NORM, h.obs_dim)
    obs0 = h.reset()
    out = h.rollout_policy(T, W, per_env=bool(per_env), obs_mean=norm[0], obs_std=norm[1], clip_obs=norm[2])
    score, want = check_exact(h, obs0, out, W, None, per_env, norm, want_ties=what is not None, want_ties_off0=what == "ties" and per_env and kind != 1)
    if what == "zero":
        # all-zero weights (ARS's first policy): every step is a tie of all actions.  Discrete: action 0.  Continuous: a zero whose
        # sign is the contract's, x_0 * (+0.0) + x_1 * (+0.0) in float64 — +0.0 unless every x_d is negative (then -0.0); both occur
        assert not score.any()
        if discrete:
            assert not out["actions"].any()
        else:
            prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
            minus = np.signbit(prev).all(-1)
            assert minus.any() and not minus.all()
            assert np.array_equal(pe.bits(out["actions"]), np.where(minus, 0x80000000, 0).astype(np.uint32)[..., None].repeat(2, -1))
    linear_checks.check_policy(h, obs0, out, W, per_env, False, *norm)
    replay(h, kind, n, rng_mode, seed0, kw, obs0, out, T, STATE_FIELDS)
    h.close()


@pytest.mark.parametrize("case", pe.MOBILE_MLP, ids=ids(pe.MOBILE_MLP))
def test_mobile_mlp_policy_actions_equal_numpy_bit_for_bit(case):
    kind, discrete, rng, n, H, per_env, normalize, seed = case
    rng_mode, seed0, T = getattr(_lib, "RNG_" + rng), 17, pe.MOBILE_T
    kw = dict(is_discrete=discrete, random_target=1)
    h = make(kind, n, rng_mode, seed0=seed0, **kw)
    W = pe.mobile_mlp_params(case)
    assert W.shape[-1] == h.mlp_param_count(H)
    norm = pe.norm_of(normalize, pe.MOBILE_NORM, h.obs_dim)
    obs0 = h.reset()
    out = h.rollout_mlp_policy(T, W, H, per_env=bool(per_env), obs_mean=norm[0], obs_std=norm[1], clip_obs=norm[2])
    score, want = check_exact(h, obs0, out, W, H, per_env, norm, want_ties=True, want_ties_off0=kind != 1)
    if not discrete and per_env:
        # env 0 has b2 = -0.0; wherever its hidden layer gives nothing the score is a zero, and the kernel's zero is +0.0
        zero = score == 0.0
        print("exact check: {} zero scores".format(int(zero.sum())))
        assert zero.any() and not pe.bits(out["actions"])[zero].any()
    mlp_checks.check_policy(h, obs0, out, W, H, False, *norm)
    replay(h, kind, n, rng_mode, seed0, kw, obs0, out, T, STATE_FIELDS)
    h.close()


@pytest.mark.parametrize("case", pe.KUKA, ids=ids(pe.KUKA))
def test_kuka_policy_actions_equal_numpy_bit_for_bit(case):
    """POLICY == 1 (H = 0 in the case: the linear policy, scores by DPP row broadcast from the lanes that hold them) and POLICY == 2
    (the MLP) of the full-model Kuka kernels."""
    env, discrete, joints, rng, n, H, per_env, normalize, seed = case
    kind, rng_mode, T = getattr(_lib, "ENV_" + env), getattr(_lib, "RNG_" + rng), pe.KUKA_T
    kw = dict(is_discrete=discrete, action_joints=joints, info_bits=1)
    h = make(kind, n, rng_mode, seed0=kcl.ENV_SEED, **kw)
    assert bool(h.cfg.force_down) == kcl.ENV_KW[env]["force_down"] and h.cfg.max_distance == kcl.ENV_KW[env]["max_distance"]
    W = pe.kuka_params(case)
    norm = pe.norm_of(normalize, pe.KUKA_NORM, 3)
    obs0 = h.reset()
    if H:
        assert W.shape[-1] == h.mlp_param_count(H)
        out = h.rollout_mlp_policy(T, W, H, per_env=bool(per_env), obs_mean=norm[0], obs_std=norm[1], clip_obs=norm[2])
    else:
        assert W.shape == h.policy_shape(per_env)
        out = h.rollout_policy(T, W, per_env=bool(per_env), obs_mean=norm[0], obs_std=norm[1], clip_obs=norm[2])
    assert not ((out["done"] >> 1) & 1).any(), "an IK conditioning flag: the parameter seed is wrong (tests/test_policy_exact_cpu.py)"
    check_exact(h, obs0, out, W, H or None, per_env, norm, want_ties=True, want_ties_off0=bool(per_env))
    if H:
        mlp_checks.check_policy(h, obs0, out, W, H, False, *norm)
    else:
        linear_checks.check_policy(h, obs0, out, W, per_env, False, *norm)
    replay(h, kind, n, rng_mode, kcl.ENV_SEED, kw, obs0, out, T, KUKA_FIELDS)
    h.close()
