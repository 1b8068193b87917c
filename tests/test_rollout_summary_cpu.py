"""CPU checks around srlhip_rollout_policy_summary: the export and its struct, the argument rules through the hostcheck program,
tests/rollout_summary_ref.py against the torch rules the learners and DeviceVecNormalize apply to the planes, and the wording of
--fused-returns' refusals."""
import argparse
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import api_rules_lines
import rollout_summary_ref as ref
from srlhip import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_struct_and_abi_version():
    with open(os.path.join(REPO, "include", "srlhip.h")) as f:
        header = f.read()
    assert re.search(r"^int srlhip_rollout_policy_summary\(srlhip_handle h, int32_t T, const srlhip_linear_policy \*linear, "
                     r"const srlhip_mlp_policy \*mlp,\s+int32_t sample, const srlhip_rollout_summary \*out\);", header, re.M)
    assert "srlhip_rollout_policy_summary" in _lib.EXPORTS
    assert re.search(r"#define SRLHIP_ABI_VERSION 5\b", header)
    lib = _lib.load()
    assert lib.srlhip_abi_version() == 5
    assert hasattr(lib, "srlhip_rollout_policy_summary")
    assert ctypes.sizeof(_lib.RolloutSummary) == 40
    assert [(n, getattr(_lib.RolloutSummary, n).offset) for n, _ in _lib.RolloutSummary._fields_] == [
        ("struct_size", 0), ("reserved", 4), ("ret", 8), ("length", 16), ("obs_sum", 24), ("obs_sqsum", 32)]


@pytest.mark.parametrize("program", api_rules_lines.PROGRAMS)
def test_the_argument_rules_through_the_hostcheck_program(program):
    api_rules_lines.build()
    lines = subprocess.check_output([os.path.join(api_rules_lines.CSRC, "build", program), "summary"]).decode().splitlines()
    want = ["summary null | -22 null out"]
    for size in (40, 32, 0):
        for reserved in (0, 1):
            for r in (0, 1):
                for le in (0, 1):
                    for a in (0, 1):
                        for b in (0, 1):
                            if size != 40:
                                verdict = "-22 srlhip_rollout_summary.struct_size mismatch (ABI)"
                            elif reserved:
                                verdict = "-22 reserved must be 0"
                            elif not r:
                                verdict = "-22 null ret"
                            elif a != b:
                                verdict = "-22 obs_sum and obs_sqsum come together (both or neither)"
                            else:
                                verdict = "0 -"
                            want.append("summary {} {} {} {} {} {} | {}".format(size, reserved, r, le, a, b, verdict))
    want.append("summary-size | 40")
    assert lines == want


def _planes(seed, T=37, N=9, D=3):
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((T, N, D)).astype(np.float32)
    reward = rs.randint(-1, 2, size=(T, N)).astype(np.float32)                  # integer-valued: exact in any summation order
    done = (rs.uniform(size=(T, N)) < 0.05).astype(np.uint8)
    done[:, 0] = 0                                                                 # an env without a done
    done[0, 1] = 1                                                                 # ... and one that reports at the first row
    done |= (rs.uniform(size=(T, N)) < 0.5).astype(np.uint8) << 1                  # bit 1 (info_bits) does not count
    return obs, reward, done


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_equals_the_learners_rules_on_random_planes(seed):
    from rl_baselines.evolution_strategies.ars import ARSModel
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    obs, reward, done = _planes(seed)
    want = ref.summary_from_planes(obs, reward, done)
    T = obs.shape[0]
    assert want["first"][0] == T and want["length"][0] == T and want["first"][1] == 0 and want["length"][1] == 1 and want["ret"][1] == 0.0
    r, d = torch.as_tensor(reward), torch.as_tensor(done)
    ret, live_rows = ARSModel.returns_from_planes(r, d)
    assert np.array_equal(ret.numpy(), want["ret"]) and int(live_rows) == int(want["length"].max())
    ret, live = CMAESModel.returns_from_planes(r, d)
    assert np.array_equal(ret.numpy(), want["ret"]) and np.array_equal(live.numpy(), want["length"].astype(np.int64))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_update_from_sums_against_update_weighted_within_the_summation_bounds(seed):
    """|mean difference| <= n 2^-52 max|x|, |var difference| <= 4 n 2^-52 mean(x^2), n the live rows: the float64 summation bounds
    of the two formulas (sum / n against a weighted mean; sqsum / n - mean^2 against the two-pass variance)."""
    from srlhip.device_env import RunningMeanStd, first_done_masks
    obs, reward, done = _planes(seed)
    want = ref.summary_from_planes(obs, reward, done)
    a, b = RunningMeanStd((3,), "cpu"), RunningMeanStd((3,), "cpu")
    a.update_from_sums(torch.as_tensor(want["length"]).sum(), torch.as_tensor(want["obs_sum"]).sum(0), torch.as_tensor(want["obs_sqsum"]).sum(0))
    live = ~first_done_masks(torch.as_tensor(done))[1]
    b.update_weighted(torch.as_tensor(obs), live)
    x = obs.astype(np.float64)[live.numpy()]
    n = x.shape[0]
    assert n == int(want["length"].sum()) and float(a.count) == float(b.count) == 1e-4 + n
    mean, var = ref.moments_from_sums(n, want["obs_sum"].sum(0), want["obs_sqsum"].sum(0))
    assert np.all(np.abs(mean - x.mean(0)) <= n * 2.0 ** -52 * np.abs(x).max(0))
    assert np.all(np.abs(a.mean.numpy() - b.mean.numpy()) <= n * 2.0 ** -52 * np.abs(x).max(0))
    assert np.all(np.abs(a.var.numpy() - b.var.numpy()) <= 4 * n * 2.0 ** -52 * (x * x).mean(0))


def test_fused_returns_refusals_name_the_flag():
    from rl_baselines.evolution_strategies.ars import ARSModel
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    base = dict(env="MobileRobotGymEnv-v0", deterministic=True, continuous_actions=False, num_stack=1, fused_returns=True)
    refused = [
        (dict(fused_rollout=False, srl_model="ground_truth"), "--fused-returns needs --fused-rollout"),
        (dict(fused_rollout=True, srl_model="raw_pixels", pixel_policy=True), "--pixel-policy"),
        (dict(fused_rollout=True, srl_model="raw_pixels", cnn_policy=True), "--cnn-policy"),
        (dict(fused_rollout=True, srl_model="autoencoder"), "learned SRL model"),
    ]
    for check in (ARSModel.check_arguments, ARSModel.check_returns_arguments, CMAESModel.check_fused_arguments):
        for kw, word in refused:
            with pytest.raises(ValueError) as e:
                check(argparse.Namespace(**dict(base, **kw)))
            assert str(e.value).startswith("--fused-returns") and word in str(e.value), str(e.value)
        check(argparse.Namespace(**dict(base, fused_rollout=True, srl_model="ground_truth")))
        check(argparse.Namespace(**dict(base, fused_returns=False, fused_rollout=False, srl_model="autoencoder", deterministic=False)))      # without the flag nothing changes
    for model in (ARSModel(), CMAESModel()):
        assert "--fused-returns" in model.customArguments(argparse.ArgumentParser()).format_help()
