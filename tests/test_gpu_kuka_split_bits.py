"""Bit pin of the physics step cut at the action (csrc/kuka_tree.hpp tphysics_pre2 / tphysics_post2): the default-configuration
KukaButton handle stepped one step per call on given actions, as tests/golden/make_kuka_split_bits.py recorded it, must reproduce
every byte of the fixture — observations, rewards, done flags and the final joint positions — on the launching path and under
persistent stepping, for Philox and MT19937."""
import importlib.util
import os

import numpy as np
import pytest

# the recorder, loaded from its file (no sys.path entry: other tests hand sys.path[:4] to child processes)
_spec = importlib.util.spec_from_file_location(
    "make_kuka_split_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_kuka_split_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("persistent", [False, True], ids=["launching", "persistent"])
@pytest.mark.parametrize("mode", rec.MODES)
def test_split_step_bits_match_fixture(golden_dir, mode, persistent):
    ref = np.load(os.path.join(golden_dir, "kuka_split_bits.npz"))
    got = rec.record(mode, persistent=persistent)
    for k, v in got.items():
        want = ref[mode + "_" + k]
        v = np.ascontiguousarray(v)
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.tobytes() != want.tobytes():
            diff = np.flatnonzero(v.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
            pytest.fail("{} {}: {} of {} bytes differ, first at byte {}".format(mode, k, diff.size, v.nbytes, diff[0]))
