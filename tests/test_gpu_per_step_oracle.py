"""GPU: the three per-step paths of HipVecEnv.step — the single-step launch with the early completion signal (the default), the resident
kernel of srlhip_set_persistent (mobile_persist_k; kuka_tree_rollout_k<PERSIST = 1>) and its staged output form
(SRLHIP_PERSIST_STAGED=1) — against the CPU ORACLE at every step, not against each other (tests/test_gpu_persistent_step.py holds them
to each other).  One handle per test, the oracle is the twin; the handle is closed in try / finally.  Cases, actions and the oracle's
side: tests/per_step_oracle_common.py.

MobileRobot family — bit for bit (np.array_equal) at every one of T = 2 * 251 + 9 steps: obs0, obs, reward, done; at the end position,
step count and the episode statistics; every env has finished two episodes.  Persistent cases park and restart the resident kernel
three times (two state reads, one sleep past the idle timeout); the signalled cases put a synchronising state read between signalled
steps at the same places.  Every path alternates srlhip_step with srlhip_step_async + srlhip_step_wait.

    kind          signal                          persistent                                   staged
    0 Mobile      n 130 mt19937 shaped            n 7 philox continuous random_target;         n 65 mt19937 random_target
                                                  n 65 mt19937 shaped
    1 1D          n 7 philox random_target        n 65 mt19937                                 n 130 philox
    2 2Target     n 65 mt19937 random_target      n 130 philox shaped                          n 7 mt19937 random_target shaped
    3 LineTarget  n 65 philox continuous          n 130 mt19937 random_target                  n 7 philox continuous random_target
  (discrete unless "continuous": only kinds 0 and 3 take continuous actions; with Philox streams the actions are still the caller's.)

Kuka (full model) — the project's bar BEFORE the IK conditioning flag (tests/kuka_scripts.py): 1e-7.  At every step `done`
and a discrete / sparse reward bit for bit, observations (and a shaped reward) within 1e-7 — the step of an auto-reset included: its
frame is the new episode's; F_KUKA_Q against the oracle's q trace within 1e-7 for every env that did not just reset (the trace holds the
old episode's last q).  The flag is read from bit 1 of the done bytes (info_bits = 1) and from the oracle's ik trace and has to go up at
the same step on both sides; from an env's first flagged step to the end of the run nothing is asserted for that env, the env-steps
are counted, printed, and capped at 5 % of the case (the oracle alone: 0 in every case, smallest IK det 9e-8 against the threshold
3e-9 — `python tests/per_step_oracle_common.py`).  Actions are random (never held), a quarter of the discrete ones turned into 'down'.

    reference (one oracle rollout each)             n x T       persistent   signal   staged    every env ends an episode
    plain discrete KukaButton, mt19937              130 x 600   n 130        n 5      n 65      asserted
    random_target, mt19937                          65 x 1200   n 65                            asserted
    continuous + shape_reward, philox               65 x 600    n 65         n 65               asserted
    joint-space continuous, joints_position, mt     5 x 1010    n 5                             (the step limit ends them; not asserted)
    joints + action_repeat 2, philox                65 x 400    n 65                            asserted
    KukaMovingButton, mt19937                       130 x 600   n 130                           asserted
    Kuka2Button ground_truth, mt19937               65 x 550    n 65                            (not asserted)
    Kuka2Button joints_position, philox             5 x 600     n 5                             (not asserted)
  A case steps the first n envs of its reference (an env's streams depend on its seed alone).

  Reading F_KUKA_Q parks the resident kernel, so a persistent case that read it after every step would never take two steps in
  residence.  Persistent and staged cases therefore alternate blocks of 25 steps: a resident block (no state read; observation, reward,
  done and flag compared at every step) and a read block (F_KUKA_Q compared after every step, each a park and a restart).  An error in
  the joint state does not heal, so the next read block sees what a resident block did to q.  One sleep past the idle timeout sits in a
  resident block.  The signalled cases read F_KUKA_Q after every step.

  Kuka2Button is the documented exception of DESIGN.md 6 ("a second amplifier": every contact event multiplies the difference between
  two float64 steppers by 50 - 100) and is held to 1e-7 all the same; its T is kept where the kernel's own source on the CPU
  (tests/hostcheck.py, the harness of tests/test_kuka_tree_kernel_source_on_host.py) stays within 1e-8 of the oracle on the same seeds
  and actions: ground_truth 5.3e-12 at T = 550 (4109 contact rows, 52 episode ends; 2.6e-10 by T = 800), joints_position 9.4e-14 at
  T = 600 (245 contact rows).  Before step 300 no env of either reference touches anything.

Measured on the MI355X (profiles/NOTES.md, section AV): see there for every case's worst |q_gpu - q_oracle| and flagged share."""
import time

import numpy as np
import pytest

import per_step_oracle_common as common
from srlhip import _lib

pytestmark = pytest.mark.gpu

BAR = 1e-7                  # rad on the joints, metres on the observations: the pre-flag bar of DESIGN.md 6
FLAG_CAP = 0.05             # share of a case's env-steps that may lie behind the IK conditioning flag
BLOCK = 25                  # persistent Kuka cases: steps per resident / read block
MOBILE_PARKS = {100: "read", 230: "sleep", 390: "read"}        # step -> what happens after it


def _idle_past_the_park_timeout():
    time.sleep(0.02)        # srlhip_set_persistent's default idle timeout: 2 ms


@pytest.mark.parametrize("case", common.MOBILE_CASES, ids=common.mobile_id)
def test_mobile_family_per_step_paths_equal_the_oracle_bit_for_bit(case, monkeypatch):
    n, T = case.n, common.MOBILE_T
    actions, ora = common.mobile_oracle(case)
    h = common.open_handle(_lib, case.kind, n, common.MOBILE_SEED0, case.rng, case.path, monkeypatch, is_discrete=case.discrete,
                           random_target=case.random_target, shape_reward=case.shape_reward)
    try:
        assert np.array_equal(h.reset(), ora["obs0"])
        out = (h.new_obs(), np.zeros(n, np.float32), np.zeros(n, np.uint8))
        for t in range(T):
            common.step(h, t, actions[t], out)
            assert np.array_equal(out[0], ora["obs"][t]), (t, "obs")
            assert np.array_equal(out[1], ora["reward"][t]), (t, "reward")
            assert np.array_equal(out[2], ora["done"][t]), (t, "done")
            what = MOBILE_PARKS.get(t)
            if what == "read":                               # persistent: parks the resident kernel; the next step restarts it
                assert h.get_state(_lib.F_STEP_COUNT).shape == (n,)
            elif what == "sleep":
                _idle_past_the_park_timeout()
        fs = ora["final_state"]
        assert np.array_equal(h.get_state(_lib.F_POS_X), fs[:, 0])
        assert np.array_equal(h.get_state(_lib.F_POS_Y), fs[:, 1])
        assert np.array_equal(h.get_state(_lib.F_STEP_COUNT), fs[:, 6].astype(np.int32))
        ret, length, fin = h.episode_stats()
        assert np.array_equal(ret, ora["ep_stats"][:, 0])
        assert np.array_equal(length, ora["ep_stats"][:, 1].astype(np.int32))
        assert np.array_equal(fin, ora["ep_stats"][:, 2].astype(np.int32))
        assert fin.min() == 2
    finally:
        h.close()


@pytest.mark.parametrize("case", common.KUKA_CASES, ids=common.kuka_id)
def test_kuka_per_step_paths_against_the_oracle_before_the_ik_flag(case, monkeypatch):
    ref = common.KUKA_REFS[case.ref]
    n, T = case.n, ref.T
    assert n <= ref.n and ref.n * T <= 80000
    actions, ora = common.kuka_oracle(case.ref)
    exact_reward = not ref.cfg.get("shape_reward")
    persistent = case.path != "signal"
    behind_ora = common.behind_flag(ora["ik_crossed"][:, :n])
    assert behind_ora.mean() <= FLAG_CAP                      # the oracle alone stays under the cap
    h = common.open_handle(_lib, ref.kind, n, ref.seed0, ref.rng, case.path, monkeypatch, **ref.cfg)
    try:
        assert h.kuka_kernel() == "tree"
        obs0 = h.reset()
        assert np.abs(obs0 - ora["obs0"][:n]).max() <= BAR
        out = (h.new_obs(), np.zeros(n, np.float32), np.zeros(n, np.uint8))
        behind = np.zeros(n, bool)                            # env is behind its flag, to the end of the run
        n_behind, worst_q, worst_obs, q_reads = 0, 0.0, 0.0, 0
        for t in range(T):
            common.step(h, t, actions[t, :n], out)
            done, flag = out[2] & 1, (out[2] >> 1) & 1
            before = ~behind
            assert np.array_equal(flag[before], ora["ik_crossed"][t, :n][before]), (t, "the flag goes up at the oracle's step")
            behind |= ora["ik_crossed"][t, :n] != 0
            n_behind += int(behind.sum())
            ok = ~behind
            assert np.array_equal(done[ok], ora["done"][t, :n][ok]), (t, "done")
            if exact_reward:
                assert np.array_equal(out[1][ok], ora["reward"][t, :n][ok]), (t, "reward")
            elif ok.any():
                assert np.abs(out[1][ok] - ora["reward"][t, :n][ok]).max() <= BAR, (t, "shaped reward")
            if ok.any():
                d_obs = float(np.abs(out[0][ok] - ora["obs"][t, :n][ok]).max())
                worst_obs = max(worst_obs, d_obs)
                assert d_obs <= BAR, (t, "obs", d_obs)
            if not persistent or (t // BLOCK) % 2 == 1:
                live = ok & (done == 0)                       # q of a just-reset env belongs to the next episode
                q = h.get_state(_lib.F_KUKA_Q).T
                q_reads += 1
                if live.any():
                    d_q = float(np.abs(q[live] - ora["q"][t, :n][live]).max())
                    worst_q = max(worst_q, d_q)
                    assert d_q <= BAR, (t, "q", d_q)
            elif t == 2 * BLOCK + 10:
                _idle_past_the_park_timeout()
        share = n_behind / float(n * T)
        print("{}: worst |q_gpu - q_oracle| = {:.3e} rad over {} reads, worst |obs_gpu - obs_oracle| = {:.3e}, env-steps behind the IK flag {} of {} ({:.2%})".format(
            common.kuka_id(case), worst_q, q_reads, worst_obs, n_behind, n * T, share))
        assert share <= FLAG_CAP
        assert worst_q <= BAR and worst_obs <= BAR
        ret, length, fin = h.episode_stats()
        ok = ~behind
        assert np.array_equal(fin[ok], ora["ep_stats"][:n, 2].astype(np.int32)[ok])
        assert np.array_equal(length[ok], ora["ep_stats"][:n, 1].astype(np.int32)[ok])
        if exact_reward:
            assert np.array_equal(ret[ok], ora["ep_stats"][:n, 0][ok])
        if ref.ends:
            assert fin.min() >= 1
    finally:
        h.close()
