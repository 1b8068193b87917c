"""CPU-side checks of the fused MLP-policy rollout (srlhip_rollout_mlp_policy): the ABI surface, the Python struct's layout against
the header's, the parameter order against torch.nn.Linear, CMA-ES's --fused-rollout argument handling and its return / live-step
accounting on reward / done planes."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mlp_policy_ref as ref
from srlhip import _lib
from rl_baselines.evolution_strategies.cma_es import BatchedMLP, CMAESModel
from test_policy_rollout_cpu import _header_struct_layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srlhip.h")


def test_symbol_is_declared_exported_and_listed():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+srlhip_rollout_mlp_policy\s*\(", text)
    assert "srlhip_rollout_mlp_policy" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "srlhip_rollout_mlp_policy")
    assert lib.srlhip_abi_version() == 5           # an additive change
    assert lib.srlhip_rollout_mlp_policy(None, 4, None, None, None, None, None) == -22


def test_python_struct_matches_header_layout():
    size, fields = _header_struct_layout("srlhip_mlp_policy")
    assert ctypes.sizeof(_lib.MlpPolicy) == size == 56
    assert [f for f, _ in fields] == [f for f, _ in _lib.MlpPolicy._fields_]
    for f, off in fields:
        assert getattr(_lib.MlpPolicy, f).offset == off, f
    # srlhip_linear_policy keeps its layout
    assert ctypes.sizeof(_lib.LinearPolicy) == 48


def test_header_documents_the_arithmetic_contract():
    text = open(HEADER).read()
    doc = text[text.index("ONE-HIDDEN-LAYER"):text.index("typedef struct srlhip_mlp_policy")]
    for word in ("fc_in.weight [H][D]", "fc_in.bias [H]", "fc_out.weight [A][H]", "fc_out.bias [A]", "float64", "FIXED", "equal bits"):
        assert word in doc, word


@pytest.mark.parametrize("H", [5, 100])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("A", [2, 4, 6, 7])
def test_parameter_order_is_nn_module_parameters_order(H, D, A):
    """torch.nn.Linear(D, H) -> ReLU -> Linear(H, A), parameters() flattened in order, against the float64 numpy reference the GPU
    tests use and against BatchedMLP (what CMA-ES hands over): 1e-5 relative to the score's scale."""
    torch.manual_seed(100 * H + 10 * D + A)
    fc_in, fc_out = torch.nn.Linear(D, H), torch.nn.Linear(H, A)
    flat = torch.cat([p.detach().reshape(-1) for m in (fc_in, fc_out) for p in m.parameters()])
    assert flat.dtype == torch.float32 and flat.numel() == ref.param_count(D, H, A) == BatchedMLP(D, A, H).n_params
    x = torch.randn(9, D)
    with torch.no_grad():
        want = fc_out(torch.relu(fc_in(x))).double().numpy()
    got, S = ref.forward(flat.numpy(), x.numpy(), D, H, A)
    assert got.shape == want.shape == (9, A)
    assert np.all(np.abs(got - want) <= 1e-5 * np.maximum(S, np.abs(want)))
    bm = BatchedMLP(D, A, H).forward(flat.double().unsqueeze(0).expand(9, -1), x.double()).numpy()
    assert np.all(np.abs(got - bm) <= 1e-12 * S)
    w1, b1, w2, b2 = ref.split(flat.numpy(), D, H, A)
    assert np.array_equal(w1, fc_in.weight.detach().numpy()) and np.array_equal(b1, fc_in.bias.detach().numpy())
    assert np.array_equal(w2, fc_out.weight.detach().numpy()) and np.array_equal(b2, fc_out.bias.detach().numpy())


def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", fused_rollout=True, deterministic=False, continuous_actions=False, num_stack=1,
                srl_model="ground_truth")
    base.update(kw)
    return argparse.Namespace(**base)


def test_cma_parser_has_the_flag_off_by_default():
    parser = CMAESModel().customArguments(argparse.ArgumentParser())
    assert parser.parse_args([]).fused_rollout is False
    assert parser.parse_args(["--fused-rollout"]).fused_rollout is True


def test_cma_fused_rollout_argument_handling():
    CMAESModel.check_fused_arguments(_args(fused_rollout=False))                      # off: nothing to check
    CMAESModel.check_fused_arguments(_args(deterministic=True))
    CMAESModel.check_fused_arguments(_args(continuous_actions=True))
    with pytest.raises(ValueError, match="--deterministic"):
        CMAESModel.check_fused_arguments(_args())
    with pytest.raises(ValueError, match="softmax"):
        CMAESModel.check_fused_arguments(_args())
    with pytest.raises(ValueError, match="num-stack"):
        CMAESModel.check_fused_arguments(_args(deterministic=True, num_stack=4))
    with pytest.raises(ValueError, match="srl-model ground_truth"):
        CMAESModel.check_fused_arguments(_args(deterministic=True, srl_model="raw_pixels"))
    CMAESModel.check_fused_arguments(_args(deterministic=True, env="KukaButtonGymEnv-v0"))
    with pytest.raises(ValueError, match="KukaRandButton"):
        CMAESModel.check_fused_arguments(_args(deterministic=True, env="KukaRandButtonGymEnv-v0"))
    # train() refuses before it builds an env (no GPU is touched)
    with pytest.raises(ValueError, match="--fused-rollout"):
        CMAESModel().train(_args(num_population=4))


def test_return_and_live_step_accounting_on_hand_made_planes():
    """3 members, 5 steps.  Member 0 reports done at step 1: the reward of that step is NOT added (the reference updates `done`
    first) and it was live in rows 0 and 1; member 1 at step 3 and again at step 4 (only the first matters); member 2 never."""
    reward = torch.tensor([[1., 10., 100.], [2., 20., 200.], [4., 40., 400.], [8., 80., 800.], [16., 160., 1600.]], dtype=torch.float32)
    done = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 3, 2]], dtype=torch.uint8)      # (bit 1: info_bits, not a done)
    ret, live = CMAESModel.returns_from_planes(reward, done)
    assert ret.dtype == torch.float64 and live.dtype == torch.int64
    assert ret.tolist() == [1.0, 70.0, 3100.0]
    assert live.tolist() == [2, 4, 5]
    done0 = torch.zeros_like(done); done0[0] = 1
    ret0, live0 = CMAESModel.returns_from_planes(reward, done0)
    assert ret0.tolist() == [0.0, 0.0, 0.0] and live0.tolist() == [1, 1, 1]
