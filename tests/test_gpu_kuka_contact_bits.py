"""Bit pin of the CONTACT steps of the fused full-model KukaButton rollout (the configuration-specialised kernel, given actions that
press the button): the same rollout as tests/golden/make_kuka_tree_contact_bits.py recorded, for Philox and MT19937, must reproduce
every byte of the fixture — observations, rewards, done flags and the final joint state.  The fixture's wavefront-steps run the
contact sweeps with one and with two normal slots (its `slots` plane, counted on the CPU by the oracle's rows)."""
import importlib.util
import os

import numpy as np
import pytest

# the recorder, loaded from its file (no sys.path entry: other tests hand sys.path[:4] to child processes)
_spec = importlib.util.spec_from_file_location(
    "make_kuka_tree_contact_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_kuka_tree_contact_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", rec.MODES)
def test_contact_rollout_bits_match_fixture(golden_dir, mode):
    ref = np.load(os.path.join(golden_dir, "kuka_tree_contact_bits.npz"))
    slots = ref[mode + "_slots"]
    assert (slots == 1).any() and (slots == 2).any()              # the recording runs cn_sweeps<1> and cn_sweeps<2>
    assert np.array_equal(ref[mode + "_actions"], rec.actions(mode))
    got = rec.record(mode)
    for k, v in got.items():
        want = ref[mode + "_" + k]
        v = np.ascontiguousarray(v)
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.tobytes() != want.tobytes():
            diff = np.flatnonzero(v.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
            pytest.fail("{} {}: {} of {} bytes differ, first at byte {}".format(mode, k, diff.size, v.nbytes, diff[0]))
    # the presses happened on the device as counted: an episode ends on the fifth contact step of each env's press
    done_at = [int(np.flatnonzero(got["done"][:, e])[0]) for e in range(rec.N_ENVS)]
    want_at = [int(np.flatnonzero(ref[mode + "_rows"][:, e])[-1]) for e in range(rec.N_ENVS)]
    assert done_at == want_at
