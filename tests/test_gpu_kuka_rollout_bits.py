"""Bit pin of the fused full-model KukaButton rollout (the configuration-specialised kernel bench.py times): the same rollout as
tests/golden/make_kuka_tree_rollout_bits.py recorded, for Philox and MT19937, must reproduce every byte of the fixture —
observations, rewards, done flags, sampled actions and the final joint state."""
import importlib.util
import os

import numpy as np
import pytest

# the recorder, loaded from its file (no sys.path entry: other tests hand sys.path[:4] to child processes)
_spec = importlib.util.spec_from_file_location(
    "make_kuka_tree_rollout_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_kuka_tree_rollout_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", rec.MODES)
def test_rollout_bits_match_fixture(golden_dir, mode):
    ref = np.load(os.path.join(golden_dir, "kuka_tree_rollout_bits.npz"))
    got = rec.record(mode)
    for k, v in got.items():
        want = ref[mode + "_" + k]
        v = np.ascontiguousarray(v)
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.tobytes() != want.tobytes():
            diff = np.flatnonzero(v.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
            pytest.fail("{} {}: {} of {} bytes differ, first at byte {}".format(mode, k, diff.size, v.nbytes, diff[0]))
