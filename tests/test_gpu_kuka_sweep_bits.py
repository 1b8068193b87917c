"""The contact-free solver of the full-model Kuka kernels (csrc/kuka_tree.hpp sweeps_free) on a small launch: 8 envs (two
workgroups; one wavefront = 4 envs already has every lane role) x 64 steps from reset.

What checks the solver's asm statements against an independent reference here is the CPU oracle on Kuka2ButtonGymEnv (its middle
sweeps are the one-sweep statement with the second button's rows between the sweeps, its last sweep the capture inside the rows),
at the tolerance of tests/test_gpu_kuka.py.  For the one-button env that role is tests/test_gpu_kuka_rollout_bits.py (a recorded
fixture) and the oracle comparisons of tests/test_gpu_kuka.py: the cases below compare the configuration-specialised instantiation
(SRLHIP_KUKA_SPEC=1, the default) with the generic one (=0; the library reads the variable once per process, hence the child
process).  Both run the SAME looping statement, so an error inside it would show in both; what the pair checks is that the
statement behaves the same under two different register allocations and schedules around it — reward / done / sampled actions bit
for bit, joints to 1e-9, as test_configuration_specialised_instantiation_equals_the_generic_one has it, for both device RNG streams.
Kuka2ButtonGymEnv has no specialised instantiation: its pair is the same kernel twice, a determinism check.

The oracle test comes first and the pair tests hang on the child's fixture: if the child fails, nothing more is started on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import kuka_clib
from srlhip import _lib

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
N, T, SEED0 = 8, 64, 5
TOL = 1e-4           # GPU against the oracle: the bar of tests/test_gpu_kuka.py
CASES = ("button_philox", "button_mt19937", "two_button")


def _actions():
    return np.random.RandomState(17).randint(6, size=(T, N)).astype(np.int32)


def run_case(case):
    two = case == "two_button"
    cfg = _lib.default_config(_lib.ENV_KUKA_2BUTTON if two else _lib.ENV_KUKA_BUTTON)
    cfg.num_envs, cfg.seed0, cfg.auto_reset = N, SEED0, 1
    if not two:
        cfg.rng_mode = _lib.RNG_PHILOX if case == "button_philox" else _lib.RNG_MT19937
    h = _lib.Handle(cfg)
    try:
        obs0 = h.reset()
        out = h.rollout(T, actions=_actions()) if two else h.rollout(T)       # one button: device-sampled actions, as bench.py
        res = {"obs0": np.asarray(obs0), "obs": out["obs"], "reward": out["reward"], "done": out["done"], "q": h.get_state(_lib.F_KUKA_Q)}
        if not two:
            res["actions"] = out["actions"]
        return res
    finally:
        h.close()


def test_two_button_free_sweeps_against_the_oracle():
    got = run_case("two_button")
    kuka_clib.set_variant(kuka_clib.VARIANT_TWO)
    try:
        ora = kuka_clib.rollout(SEED0 + np.arange(N), T, actions=_actions(), force_down=False, max_distance=2.0, trace=False)
    finally:
        kuka_clib.set_variant(kuka_clib.VARIANT_BUTTON)
    assert np.abs(ora["obs0"] - got["obs0"]).max() <= TOL and np.abs(ora["obs"] - got["obs"]).max() <= TOL
    assert np.array_equal(ora["done"], got["done"]) and np.array_equal(ora["reward"], got["reward"])
    assert np.abs(got["q"].T - ora["final_state"][:, :7]).max() <= TOL


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    """every case once with SRLHIP_KUKA_SPEC=0, in one child process"""
    path = str(tmp_path_factory.mktemp("sweep_bits") / "generic.npz")
    code = ("import sys, numpy as np; sys.path[:0] = {!r}; import torch; import test_gpu_kuka_sweep_bits as t; "
            "np.savez({!r}, **{{c + '_' + k: v for c in t.CASES for k, v in t.run_case(c).items()}})").format(
                [TESTS, os.path.join(REPO, "robotics-rl-srl_amd"), REPO], path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRLHIP_KUKA_SPEC="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("case", CASES)
def test_specialised_and_generic_free_sweeps_agree(generic, case):
    got = run_case(case)
    assert not got["done"].any()                                             # 64 steps from reset: no episode ends
    assert np.array_equal(got["obs0"], generic[case + "_obs0"])
    for k in ("reward", "done") + (() if case == "two_button" else ("actions",)):
        assert np.array_equal(got[k], generic[case + "_" + k]), k
    assert np.abs(got["q"] - generic[case + "_q"]).max() <= 1e-9
    assert np.abs(got["obs"] - generic[case + "_obs"]).max() <= 1e-6
    assert np.abs(got["q"]).max() > 0.1 and np.ptp(got["obs"], axis=0).max() > 1e-3      # the arm moved
