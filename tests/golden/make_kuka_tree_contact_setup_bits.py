"""Record tests/golden/kuka_tree_contact_setup_bits.npz: the exact bytes of fused full-model Kuka rollouts that spend MANY steps in
contact, as the pin of the contact step's SETUP (csrc/kuka_tree.hpp general_path: candidates -> row definitions, W J, the own
bank-B row, the outputs behind the sweeps).  tests/golden/kuka_tree_contact_bits.npz pins the default configuration, in which a
press is five contact steps behind ~310 approach steps (the episode ends on the fifth); here every env step repeats its action
over ACTION_REPEAT = 8 physics steps, so the arm reaches the button in ~40 env steps, and 300 steps hold four to six presses per
env: 20 and more contact steps.  (With action_repeat = 1 no script reaches the button within 300 steps.)  The configuration with
action_repeat != 1 runs the generic instantiation of the rollout kernel; the configuration-specialised one shares general_path and
stays pinned by kuka_tree_contact_bits.npz / kuka_tree_rollout_bits.npz.

Cases (tests/kuka_scripts.py style: a short sideways prefix, then "down" held to the end; auto-reset on):
  * "philox", "mt19937": KukaButton, 8 envs (two wavefronts of four) x 300 steps, one per env RNG stream.
      env 0      presses; envs 1, 2, 3 never leave free space (they alternate -x / +x): the wavefront's contact steps have exactly
                 ONE env in contact, the other three envs' slots hold what earlier steps left there
      env 4      a press whose contact steps are mostly one-normal steps
      env 5      a press with two contact normals (both finger tips) on five or more steps
      envs 6, 7  two more presses, starting at other steps
  * "two": Kuka2Button, 4 envs x 300 steps (MT19937), every env pressing the first button.

Not vacuous: check_counts() asserts on the CPU oracle's own rows (oracle.kuka_clib.rollout(aux=True), no GPU), before anything is
recorded, that env 0, env 4 and env 5 have at least 20 contact steps each, that envs 1-3 have none, that env 4 has five or more
one-normal steps and env 5 five or more two-normal steps, that the Kuka2Button case has at least 20 contact steps and five with
two normals, and that no step carries a joint-limit row.

Per case: obs0, obs / reward / done of every step, the final joint positions / velocities, the actions and the oracle's rows.
tests/test_gpu_kuka_contact_setup.py re-runs the rollouts and asserts byte equality.

Run on a GPU box from the repository root:  python tests/golden/make_kuka_tree_contact_setup_bits.py [out.npz]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

T, ACTION_REPEAT, WAVE_ENVS = 300, 8, 4
CASES = ("philox", "mt19937", "two")
N_ENVS = {"philox": 8, "mt19937": 8, "two": 4}
SEED0 = {"philox": 11, "mt19937": 11, "two": 60}
MIN_CONTACT_STEPS, MIN_TWO_NORMAL_STEPS, MIN_ONE_NORMAL_STEPS = 20, 5, 5
FREE = None      # an env that stays in free space
# per env: (x action, steps of it, y action, steps of it); then action 4 (down) to the end.  0 -x, 1 +x, 2 -y, 3 +y.
PREFIX = {
    "philox": ((0, 0, 2, 0), FREE, FREE, FREE, (0, 2, 2, 1), (0, 0, 2, 0), (0, 1, 2, 0), (1, 1, 2, 0)),
    "mt19937": ((0, 0, 2, 0), FREE, FREE, FREE, (0, 1, 2, 0), (1, 1, 2, 1), (0, 0, 2, 1), (1, 1, 2, 0)),
    "two": ((0, 0, 2, 4), (0, 0, 2, 4), (0, 0, 2, 4), (0, 0, 2, 4)),
}


def actions(case):
    """int32 [T][n]"""
    a = np.full((T, N_ENVS[case]), 4, np.int32)
    for e, pre in enumerate(PREFIX[case]):
        if pre is FREE:
            a[:, e] = np.arange(T) % 2
        else:
            ax, k, ay, m = pre
            a[:k, e] = ax
            a[k:k + m, e] = ay
    return a


def record(case):
    from srlhip import _lib
    cfg = _lib.default_config(_lib.ENV_KUKA_2BUTTON if case == "two" else _lib.ENV_KUKA_BUTTON)
    cfg.num_envs, cfg.seed0, cfg.auto_reset, cfg.action_repeat = N_ENVS[case], SEED0[case], 1, ACTION_REPEAT
    cfg.rng_mode = _lib.RNG_PHILOX if case == "philox" else _lib.RNG_MT19937
    h = _lib.Handle(cfg)
    try:
        obs0 = h.reset()
        out = h.rollout(T, actions=actions(case))
        return {"obs0": np.asarray(obs0), "obs": out["obs"], "reward": out["reward"], "done": out["done"],
                "q": h.get_state(_lib.F_KUKA_Q), "qd": h.get_state(_lib.F_KUKA_QD)}
    finally:
        h.close()


def oracle_rows(case):
    """(rows [T][n] contact-normal rows per env-step, env-steps with a joint-limit row) by the CPU oracle; no GPU."""
    from oracle import kuka_clib
    full = kuka_clib.is_full()
    kuka_clib.set_full(True)
    kuka_clib.set_variant(kuka_clib.VARIANT_TWO if case == "two" else kuka_clib.VARIANT_BUTTON)
    try:
        o = kuka_clib.rollout(SEED0[case] + np.arange(N_ENVS[case]), T, actions=actions(case), aux=True, trace=False, action_repeat=ACTION_REPEAT,
                              rng_mode=kuka_clib.RNG_PHILOX if case == "philox" else kuka_clib.RNG_MT19937)
    finally:
        kuka_clib.set_variant(kuka_clib.VARIANT_BUTTON)
        kuka_clib.set_full(full)
    return o["rows"][:, :, 0].astype(np.int32), int((o["rows"][:, :, 1] >= 1000).sum())


def check_counts(case, rows, nlimit):
    """the conditions of the module docstring on one case's rows"""
    assert nlimit == 0
    contact, one, two = (rows > 0).sum(axis=0), (rows == 1).sum(axis=0), (rows >= 2).sum(axis=0)
    if case == "two":
        assert contact.sum() >= MIN_CONTACT_STEPS and two.sum() >= MIN_TWO_NORMAL_STEPS, (contact, two)
        return
    for e in (0, 4, 5):
        assert contact[e] >= MIN_CONTACT_STEPS, (case, e, contact)
    assert not contact[1:WAVE_ENVS].any(), contact                        # wavefront 0: one env in contact, three free
    assert one[4] >= MIN_ONE_NORMAL_STEPS and two[5] >= MIN_TWO_NORMAL_STEPS, (case, one, two)
    starts = {int(np.flatnonzero(rows[:, e])[0]) for e in (4, 5, 6, 7)}
    assert len(starts) >= 2, starts                                       # wavefront 1: presses that start at different steps


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "kuka_tree_contact_setup_bits.npz")
    planes = {}
    for case in CASES:
        rows, nlimit = oracle_rows(case)
        check_counts(case, rows, nlimit)
        planes[case + "_rows"], planes[case + "_actions"] = rows, actions(case)
    if path != "--check":
        for case in CASES:
            for k, v in record(case).items():
                planes[case + "_" + k] = v
        np.savez_compressed(path, **planes)
        print(path, os.path.getsize(path), "bytes", {k: (v.shape, str(v.dtype)) for k, v in planes.items()})
    for case in CASES:
        r = planes[case + "_rows"]
        print(case, "contact steps per env:", (r > 0).sum(axis=0).tolist(), "with two normals:", (r >= 2).sum(axis=0).tolist())


if __name__ == "__main__":
    main()
