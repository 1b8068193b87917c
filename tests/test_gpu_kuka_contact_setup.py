"""Bit pin of the contact step's SETUP of the fused full-model Kuka rollouts (csrc/kuka_tree.hpp general_path: candidates -> row
definitions, W J, the own bank-B row, the outputs behind the sweeps): the rollouts tests/golden/make_kuka_tree_contact_setup_bits.py
recorded BEFORE the setup was restructured — pressing scripts with action_repeat = 8, 8 envs x 300 steps on both env RNG streams
(one wavefront with a single env in contact next to three free ones, one with one- and two-normal presses) and a Kuka2Button case
of 4 envs x 300 steps — must reproduce every byte of the fixture: observations, rewards, done flags, final joint positions and
velocities.  The fixture is not vacuous: the recorder's own conditions on the CPU oracle's rows (20 and more contact steps per
scripted env, five and more two-normal steps) are re-asserted here on the rows it stored."""
import importlib.util
import os

import numpy as np
import pytest

# the recorder, loaded from its file (no sys.path entry: other tests hand sys.path[:4] to child processes)
_spec = importlib.util.spec_from_file_location(
    "make_kuka_tree_contact_setup_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_kuka_tree_contact_setup_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "kuka_tree_contact_setup_bits.npz"))


@pytest.mark.parametrize("case", rec.CASES)
def test_contact_setup_rollout_bits_match_fixture(fixture, case):
    ref = fixture
    rec.check_counts(case, ref[case + "_rows"], 0)                 # the recording reaches the contacts it is there for
    assert np.array_equal(ref[case + "_actions"], rec.actions(case))
    got = rec.record(case)
    for k, v in got.items():
        want = ref[case + "_" + k]
        v = np.ascontiguousarray(v)
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.tobytes() != want.tobytes():
            diff = np.flatnonzero(v.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
            pytest.fail("{} {}: {} of {} bytes differ, first at byte {}".format(case, k, diff.size, v.nbytes, diff[0]))
    # the presses happened on the device too: a contact step of the one-button env is a reward of 1, and the free envs see none
    if case != "two":
        assert got["reward"][:, 0].sum() >= rec.MIN_CONTACT_STEPS and not got["reward"][:, 1:rec.WAVE_ENVS].any()
