"""CPU: the reference of the sampled MLP-policy rollout against itself (tests/mlp_sample_ref.py), and the --fused-sampling argument
rules of CMA-ES.  No GPU."""
import argparse

import numpy as np
import pytest

import mlp_policy_ref as ref
import mlp_sample_ref as sref
import rng_stream_ref as rsr
from rl_baselines.evolution_strategies.ars import ARSModel
from rl_baselines.evolution_strategies.cma_es import CMAESModel

T, N, D, H, A = 40, 33, 2, 100, 4
SEEDS = 17 + np.arange(N)
C0 = 7


def _inputs():
    W = ref.random_params(4000, (N, ref.param_count(D, H, A)))
    x = np.random.RandomState(1).uniform(-1.5, 1.5, size=(T, N, D)).astype(np.float32)
    score, S = ref.forward(W, x, D, H, A)
    return score, S


def test_draws_are_the_action_stream_of_the_definition():
    u = sref.draws(SEEDS, C0, T)
    assert u.shape == (T, N) and u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    for t, e in ((0, 0), (5, 3), (T - 1, N - 1)):
        o = rsr.project_block(int(SEEDS[e]) & rsr.M32, int(SEEDS[e]) >> 32, C0 + t, 1)
        assert u[t, e] == rsr.to_double(o[0], o[1])
    # random access: a later start is the same plane, shifted; per-env starts are honoured
    assert np.array_equal(sref.draws(SEEDS, C0 + 10, T - 10), u[10:])
    c0 = C0 + np.arange(N)
    assert np.array_equal(sref.draws(SEEDS, c0, 3)[0, 5], u[5, 5])
    big = sref.draws(np.array([2 ** 40 + 7]), 2 ** 32 - 2, 4)         # key and counter high words
    o = rsr.project_block(7, 2 ** 8, 2 ** 32 + 1, 1)
    assert big[3, 0] == rsr.to_double(o[0], o[1])


def test_a_kernel_that_follows_the_contract_is_accepted_and_others_are_not():
    score, S = _inputs()
    u = sref.draws(SEEDS, C0, T)
    a = sref.contract(score, u)
    assert a.min() >= 0 and a.max() <= A - 1 and len(np.unique(a)) == A
    off = float((a != score.argmax(-1)).mean())
    assert off >= 0.05, "precondition on the inputs: choose another parameter seed"
    ok, differs = sref.sample_check(score, S, u, a)
    assert ok.all() and not differs.any()
    # frozen entries are -1 and nothing else
    frozen = np.zeros((T, N), bool); frozen[20:, ::3] = True
    ok, _ = sref.sample_check(score, S, u, np.where(frozen, -1, a), frozen)
    assert ok.all()
    ok, _ = sref.sample_check(score, S, u, a, frozen)
    assert not ok[frozen].any() and ok[~frozen].all()
    ok, _ = sref.sample_check(score, S, u, np.where(frozen, -1, a))
    assert not ok[frozen].any()
    # the draw shifted by one counter, and the argmax, are rejected on the same inputs
    shifted = sref.contract(score, sref.draws(SEEDS, C0 + 1, T))
    ok, differs = sref.sample_check(score, S, u, shifted)
    assert not ok.all() and (~ok).sum() == (shifted != a).sum() == differs.sum()
    ok, _ = sref.sample_check(score, S, u, score.argmax(-1).astype(np.int32))
    assert (~ok).sum() == (score.argmax(-1) != a).sum() > 0
    # a neighbouring index is accepted only inside the rounding margin: one step up or down is rejected wherever it is in range
    for d in (-1, 1):
        b = a + d
        inside = (b >= 0) & (b < A)
        ok, _ = sref.sample_check(score, S, u, np.clip(b, 0, A - 1).astype(np.int32))
        assert not ok[inside].any()


def test_the_margin_admits_both_sides_of_a_tie_within_rounding():
    """z exactly on c_0: the contract says 1 (z >= c_0); within rho the rule accepts 0 and 1, never 2"""
    score = np.zeros((1, 4))
    S = np.ones((1, 4))
    u = np.array([0.25])
    assert sref.contract(score, u)[0] == 1
    for a, want in ((0, True), (1, True), (2, False), (3, False)):
        assert bool(sref.sample_check(score, S, u, np.array([a], np.int32))[0][0]) is want


def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", fused_rollout=True, fused_sampling=False, deterministic=False, continuous_actions=False, num_stack=1,
                srl_model="ground_truth")
    base.update(kw)
    return argparse.Namespace(**base)


def test_cma_parser_has_fused_sampling_off_by_default():
    parser = CMAESModel().customArguments(argparse.ArgumentParser())
    assert parser.parse_args([]).fused_sampling is False
    assert parser.parse_args(["--fused-rollout", "--fused-sampling"]).fused_sampling is True
    assert "--fused-sampling" not in ARSModel().customArguments(argparse.ArgumentParser()).format_help()      # ARS does not change


def test_cma_fused_sampling_argument_rules():
    CMAESModel.check_fused_arguments(_args(fused_sampling=True))                       # the flag meets the --deterministic requirement
    CMAESModel.check_fused_arguments(_args(fused_sampling=True, env="KukaButtonGymEnv-v0"))
    CMAESModel.check_fused_arguments(_args(fused_sampling=True, deterministic=True))
    with pytest.raises(ValueError) as old:                                             # without it: the old text, word for word
        CMAESModel.check_fused_arguments(_args())
    with pytest.raises(ValueError) as ars:
        ARSModel.check_fused_arguments(_args())
    assert str(old.value) == str(ars.value) and "--deterministic" in str(old.value) and "softmax" in str(old.value)
    with pytest.raises(ValueError, match="--deterministic"):                           # a namespace from before the flag existed
        CMAESModel.check_fused_arguments(argparse.Namespace(env="MobileRobotGymEnv-v0", fused_rollout=True, num_stack=1, srl_model="ground_truth"))
    with pytest.raises(ValueError, match="continuous"):
        CMAESModel.check_fused_arguments(_args(fused_sampling=True, continuous_actions=True))
    with pytest.raises(ValueError, match="--fused-rollout"):
        CMAESModel.check_fused_arguments(_args(fused_sampling=True, fused_rollout=False))
    # ARS's other rules still stand behind the flag
    with pytest.raises(ValueError, match="num-stack"):
        CMAESModel.check_fused_arguments(_args(fused_sampling=True, num_stack=4))
    with pytest.raises(ValueError, match="srl-model ground_truth"):
        CMAESModel.check_fused_arguments(_args(fused_sampling=True, srl_model="raw_pixels"))
    with pytest.raises(ValueError, match="KukaRandButton"):
        CMAESModel.check_fused_arguments(_args(fused_sampling=True, env="KukaRandButtonGymEnv-v0"))
    with pytest.raises(ValueError, match="--deterministic"):                           # ARS itself does not know the flag
        ARSModel.check_fused_arguments(_args(fused_sampling=True))
    with pytest.raises(ValueError, match="--fused-sampling"):                          # train() refuses before it builds an env
        CMAESModel().train(_args(fused_sampling=True, fused_rollout=False, num_population=4))


def test_evaluate_fused_samples_only_for_a_stochastic_discrete_model():
    class Env(object):
        def rollout_mlp_policy(self, T_, params, hidden, **kw):
            import torch
            self.kw = kw
            return {"reward": torch.zeros((T_, 2)), "done": torch.ones((T_, 2), dtype=torch.uint8)}

    import torch
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP
    for det, cont, want in ((False, False, True), (True, False, False), (False, True, False), (None, None, False)):
        m = CMAESModel()
        m.policy, m.deterministic, m.continuous_actions = BatchedMLP(2, 4, 5), det, cont
        env = Env()
        m.evaluate_fused(env, torch.zeros((2, m.policy.n_params), dtype=torch.float64), 3)
        assert env.kw.get("sample", False) is want, (det, cont)
        assert env.kw["per_env"] is True and env.kw["freeze_after_done"] is True
