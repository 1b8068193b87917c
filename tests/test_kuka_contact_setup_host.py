"""CPU: the contact step's SETUP of the full-model Kuka stepper (csrc/kuka_tree.hpp general_path: contact geometry published by the
sphere's lane, Jacobian entries computed one per joint lane, W J and the bank-B couplings walked over the used slots only) executed
on the host — 16 lockstep fibers per env, LDS scratch poisoned with NaN (csrc/kuka_hostcheck.cpp) — against the oracle's full-model
mode, on SCRIPTED presses that spend 20 and more steps in contact (tests/golden/make_kuka_tree_contact_setup_bits.py: action_repeat
= 8, a press every ~45 env steps):
  * an env pressing with one contact normal, an env with two normals on the same step,
  * a group of four envs of which exactly one is in contact while three stay free.  The host harness runs ONE env per lane group
    (its wany() spans one env's 16 fibers), so the used-slot counts are per env here and no loop walks a slot that only ANOTHER env
    of a wavefront uses: that case — the select on a stale slot — is covered on the GPU alone, by wavefront 0 of the philox and
    mt19937 cases of tests/test_gpu_kuka_contact_setup.py.  What this case adds on the host: free envs next to a pressing one
    never enter the setup, and the pressing env's results do not depend on its neighbours,
  * steps with a joint-limit row next to the contact rows (a tightened model table: the general path's LDS sweep, which the setup
    feeds too), with a row budget that overflows,
  * the two-button variant (NB = 2).
Bar: the one of tests/test_kuka_tree_kernel_source_on_host.py — 1e-9 on every joint, discrete flags bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import hostcheck
from oracle import kuka_clib
from srlhip import kuka_model

TOL = 1e-9          # tests/test_kuka_tree_kernel_source_on_host.py

_spec = importlib.util.spec_from_file_location(
    "make_kuka_tree_contact_setup_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_kuka_tree_contact_setup_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(autouse=True)
def full_oracle():
    kuka_clib.set_full(True)
    yield
    kuka_clib.set_full(False)


def both(seeds, actions, variant=0, **kw):
    """(oracle, kernel source on the host) on the same seeds and actions; parity asserted"""
    T = actions.shape[0]
    kuka_clib.set_variant(variant); hostcheck.set_variant(variant)
    try:
        a = kuka_clib.rollout(seeds, T, actions=actions, aux=True, action_repeat=rec.ACTION_REPEAT, **kw)
        b = hostcheck.tree_rollout(seeds, T, actions=actions, action_repeat=rec.ACTION_REPEAT, **kw)
    finally:
        kuka_clib.set_variant(0); hostcheck.set_variant(0)
    assert np.array_equal(a["reward"], b["reward"]) and np.array_equal(a["done"], b["done"])
    assert np.abs(a["reward64"] - b["reward64"]).max() <= TOL
    assert np.abs(a["q"] - b["q"]).max() <= TOL and np.abs(a["gripper"] - b["gripper"]).max() <= TOL
    assert np.abs(a["final_state"][:, 30:35] - b["final_state"][:, 30:35]).max() <= TOL           # gripper joints
    assert np.array_equal(a["ep_stats"][:, 1:], b["ep_stats"][:, 1:])
    return a, b


def pressing(case, envs):
    seeds = rec.SEED0[case] + np.asarray(envs)
    return seeds, np.ascontiguousarray(rec.actions(case)[:, envs])


@pytest.mark.parametrize("case,rng_mode", [("philox", kuka_clib.RNG_PHILOX), ("mt19937", kuka_clib.RNG_MT19937)])
def test_one_env_pressing_with_one_normal_and_one_with_two(case, rng_mode):
    for env, two_normals in ((4, False), (5, True)):
        seeds, actions = pressing(case, [env])
        a, _ = both(seeds, actions, rng_mode=rng_mode)
        rows = a["rows"][:, 0, 0]
        assert (rows > 0).sum() >= rec.MIN_CONTACT_STEPS and (a["rows"][:, 0, 1] >= 1000).sum() == 0
        assert ((rows >= 2).sum() >= rec.MIN_TWO_NORMAL_STEPS) if two_normals else ((rows == 1).sum() >= rec.MIN_ONE_NORMAL_STEPS)


def test_group_of_four_with_exactly_one_env_in_contact():
    seeds, actions = pressing("philox", [0, 1, 2, 3])
    a, _ = both(seeds, actions, rng_mode=kuka_clib.RNG_PHILOX)
    contact = (a["rows"][:, :, 0] > 0).sum(axis=0)
    assert contact[0] >= rec.MIN_CONTACT_STEPS and not contact[1:].any(), contact


def test_contact_steps_with_a_joint_limit_row():
    """Limits of joints 3 and 5 at 0.3 rad around the settled pose and a row budget of 3: one or two limit rows stand next to the
    contact and friction rows of the press (the LDS general sweep on a setup that holds limit AND contact slots), and two limits
    with two normals overflow the budget."""
    t = kuka_clib.get_tree_model().copy()
    J = kuka_model.TREE_JOINT0 + kuka_model.TREE_JOINT_STRIDE * np.array([3, 5])
    q_settled = np.array([-0.86, 1.68])
    t[J + kuka_model.TREE_LOWER] = q_settled - 0.3
    t[J + kuka_model.TREE_UPPER] = q_settled + 0.3
    t[kuka_model.TREE_MAX_GENERIC_ROWS] = 3.0
    seeds, actions = pressing("philox", [0, 4, 5, 6])
    try:
        kuka_clib.set_tree_model(t); hostcheck.tree_set_model(t)
        a, _ = both(seeds, actions, rng_mode=kuka_clib.RNG_PHILOX)
    finally:
        hostcheck.tree_set_model(None); kuka_clib.set_full(True)
    lim, normals = a["rows"][:, :, 1] // 1000, a["rows"][:, :, 0]
    assert ((lim > 0) & (normals > 0)).sum() >= rec.MIN_CONTACT_STEPS and lim.max() == 2, (((lim > 0) & (normals > 0)).sum(), lim.max())


def test_two_button_variant():
    case = "two"
    seeds, actions = pressing(case, list(range(rec.N_ENVS[case])))
    a, b = both(seeds, actions, variant=2, rng_mode=kuka_clib.RNG_MT19937)
    rows = a["rows"][:, :, 0]
    assert (rows > 0).sum() >= rec.MIN_CONTACT_STEPS and (rows >= 2).sum() >= rec.MIN_TWO_NORMAL_STEPS
    assert np.array_equal(a["final_state"][:, 26:28], b["final_state"][:, 26:28])                 # goal_id, n_contacts[1]
    assert np.abs(a["final_state"][:, 24:26] - b["final_state"][:, 24:26]).max() <= TOL           # second glider
