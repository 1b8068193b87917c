"""The reference's `step(None)` in the continuous Kuka action modes (kuka_button_gym_env.py:293-299), as recorded by
tests/golden/make_kuka_none_golden.py: the fixture is self-consistent — a `None` step leaves the IK target where it was (Cartesian) or
commands joint_positions[:7] (joints) and draws nothing from np_random; every other step draws exactly once."""
import os

import numpy as np
import pytest

# kuka.py:27 joint_positions (the seven arm joints)
JOINT_POSITIONS = np.array([0.006418, 0.113184, -0.011401, -1.289317, 0.005379, 1.737684, -0.006539])


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "kuka_none_reference.npz"))


def cases(golden):
    return sorted({k.rsplit("|", 1)[0] for k in golden.files})


def test_fixture_covers_the_issue_cases(golden):
    tags = cases(golden)
    assert len(tags) == 2 * 3 * (4 + 2)                       # 2 envs x 3 seeds x (4 Cartesian + 2 joint-space configurations)
    for tag in tags:
        none = golden[tag + "|none"]
        n = int(golden[tag + "|n_steps"])
        assert n == len(none) >= 250, tag
        assert none[0], tag                                    # the first step after reset is a `None`
        assert 0.2 <= none.mean() <= 0.45, tag
        runs = np.diff(np.flatnonzero(np.diff(np.r_[0, none.astype(np.int8), 0])))[::2]
        assert runs.max() >= 5, tag
        a = golden[tag + "|actions"]
        assert np.isnan(a[none]).all() and np.isfinite(a[~none]).all(), tag
        assert np.array_equal(a[~none], a[~none].astype(np.float32).astype(np.float64)), tag


def test_none_steps_draw_nothing_and_hold_the_command(golden):
    for tag in cases(golden):
        none, adv, drawn = golden[tag + "|none"], golden[tag + "|advanced"], golden[tag + "|drawn"]
        assert not adv[none].any() and np.isnan(drawn[none]).all(), tag
        assert adv[~none].all() and np.isfinite(drawn[~none]).all(), tag
        ik, motor = golden[tag + "|ik"], golden[tag + "|motor"]
        if "|joints|" in tag:
            assert np.isnan(ik).all()
            assert np.array_equal(motor[none], np.broadcast_to(JOINT_POSITIONS, (none.sum(), 7))), tag
            a = golden[tag + "|actions"].astype(np.float32)
            assert not np.array_equal(motor[~none][:, 0], np.full((~none).sum(), JOINT_POSITIONS[0])), tag
            assert np.isfinite(a[~none]).all()
        else:
            prev = np.concatenate([golden[tag + "|reset_ik"][-1:], ik[:-1]])
            assert np.array_equal(ik[none], prev[none]), tag  # step2([0, 0, 0, 0, 0]): the clipped target does not move
            assert not np.array_equal(ik[~none], prev[~none]), tag

