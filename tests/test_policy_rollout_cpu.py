"""CPU-side checks of the fused linear-policy rollout (srlhip_rollout_policy): the ABI surface, the Python struct's layout
against the header's, ARS's --fused-rollout argument handling and the return rule on reward / done planes."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from srlhip import _lib
from rl_baselines.evolution_strategies.ars import ARSModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srlhip.h")


def test_symbol_is_declared_exported_and_listed():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+srlhip_rollout_policy\s*\(", text)
    assert "srlhip_rollout_policy" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "srlhip_rollout_policy")
    assert lib.srlhip_abi_version() == 5           # an additive change


def _header_struct_layout(name):
    """(size, [(field, offset)]) of a plain struct in the header under the C ABI's natural alignment"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "double": 8, "int64_t": 8, "float": 4}
    off, align, fields = 0, 1, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s+(.*)", decl)
        ctype, names = m.group(2), [x.strip() for x in m.group(3).split(",")]
        for nm in names:
            size = 8 if nm.startswith("*") else sizes[ctype]
            off = (off + size - 1) // size * size
            fields.append((nm.lstrip("*"), off))
            off += size
            align = max(align, size)
    return (off + align - 1) // align * align, fields


def test_python_struct_matches_header_layout():
    size, fields = _header_struct_layout("srlhip_linear_policy")
    assert ctypes.sizeof(_lib.LinearPolicy) == size == 48
    assert [f for f, _ in fields] == [f for f, _ in _lib.LinearPolicy._fields_]
    for f, off in fields:
        assert getattr(_lib.LinearPolicy, f).offset == off, f


def test_entry_point_validates_before_it_touches_anything():
    lib = _lib.load()
    assert lib.srlhip_rollout_policy(None, 4, None, None, None, None, None) == -22


def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", fused_rollout=True, deterministic=False, continuous_actions=False, num_stack=1,
                srl_model="ground_truth")
    base.update(kw)
    return argparse.Namespace(**base)


def test_ars_parser_has_the_flag_off_by_default():
    parser = ARSModel().customArguments(argparse.ArgumentParser())
    assert parser.parse_args([]).fused_rollout is False
    assert parser.parse_args(["--fused-rollout"]).fused_rollout is True


def test_ars_fused_rollout_argument_handling():
    ARSModel.check_fused_arguments(_args(fused_rollout=False))                        # off: nothing to check
    ARSModel.check_fused_arguments(_args(deterministic=True))
    ARSModel.check_fused_arguments(_args(continuous_actions=True))
    with pytest.raises(ValueError, match="--deterministic or --continuous-actions"):
        ARSModel.check_fused_arguments(_args())
    with pytest.raises(ValueError, match="num-stack"):
        ARSModel.check_fused_arguments(_args(deterministic=True, num_stack=4))
    ARSModel.check_fused_arguments(_args(deterministic=True, env="KukaButtonGymEnv-v0"))
    with pytest.raises(ValueError, match="KukaRandButton"):
        ARSModel.check_fused_arguments(_args(deterministic=True, env="KukaRandButtonGymEnv-v0"))
    # train() refuses before it builds an env (no GPU is touched)
    bad = _args(num_population=2, top_population=1)
    with pytest.raises(ValueError, match="--fused-rollout"):
        ARSModel().train(bad)


def test_return_rule_on_hand_made_planes():
    """3 envs, 5 steps.  env 0 reports done at step 1 (its reward there does not count), env 1 at step 3 and again at step 4
    (only the first matters), env 2 never."""
    reward = torch.tensor([[1., 10., 100.], [2., 20., 200.], [4., 40., 400.], [8., 80., 800.], [16., 160., 1600.]], dtype=torch.float32)
    done = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0]], dtype=torch.uint8)
    ret, live_rows = ARSModel.returns_from_planes(reward, done)
    assert ret.dtype == torch.float64
    assert ret.tolist() == [1.0, 70.0, 3100.0]
    assert int(live_rows) == 5                      # env 2 is live in every row
    # every env done at step 1: rows 0 and 1 are acted in live, rows 2.. are all frozen
    done2 = torch.tensor([[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.uint8)
    ret2, live2 = ARSModel.returns_from_planes(reward, done2)
    assert ret2.tolist() == [1.0, 10.0, 100.0] and int(live2) == 2
