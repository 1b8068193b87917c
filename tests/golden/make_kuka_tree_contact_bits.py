"""Record tests/golden/kuka_tree_contact_bits.npz: the exact bytes of a fused full-model KukaButton rollout (the configuration-
specialised kernel bench.py times) whose GIVEN actions press the button, for both env RNG streams, Philox and MT19937.
tests/golden/kuka_tree_rollout_bits.npz pins a random agent, whose 32 envs x 1100 steps hold a handful of contact steps; this one
pins the contact sweeps (csrc/kuka_tree.hpp cn_sweeps<NG>): 8 envs (two wavefronts of four) x 400 steps.

Every env runs `k` steps of -x / +x, `m` steps of -y / +y, then holds "down" (tests/kuka_scripts.py's pressing scripts with a short
sideways prefix that decides where on the cap the finger tips land and when).  A press is five contact steps, then the episode
ends and the env resets (auto-reset on).  Placed per stream so that wavefront 0 has
  * two envs in contact on the SAME five steps,
  * a single env in contact (two of them, at different steps),
  * presses that start at three or more different steps,
and wavefront 1 two envs whose presses coincide with two contact normals each.  What a wavefront runs is cn_sweeps<NG> with NG the
largest number of contact-normal rows among its four envs: the fixture holds wavefront-steps with NG = 1 and with NG = 2.  No
script of this family reaches three normal rows in an env (a random agent does not either: profiles/NOTES.md section J counts 283 /
15 / 0 env-steps with 1 / 2 / 3), so NG = 3 is not in it.

The row counts are established WITHOUT the GPU, by the CPU oracle's own rows (oracle.kuka_clib.rollout(aux=True)): `rows` [T][8] is
the number of contact-normal rows of every env-step, `slots` [T][2] its maximum over each wavefront's envs; no step of the
recording has a joint-limit row (which would send the wavefront down the general LDS path instead).  check_counts() asserts all of
the above before anything is written.

Per stream: obs0, obs / reward / done of every step, the final joint positions / velocities, the actions, rows and slots.
tests/test_gpu_kuka_contact_bits.py re-runs the rollout and asserts byte equality.

Run on a GPU box from the repository root:  python tests/golden/make_kuka_tree_contact_bits.py [out.npz]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

N_ENVS, T, SEED0, WAVE_ENVS = 8, 400, 11, 4
MODES = ("philox", "mt19937")
# per env: (x action, steps of it, y action, steps of it); then action 4 (down) to the end.  0 -x, 1 +x, 2 -y, 3 +y.
PREFIX = {
    "philox": ((1, 1, 3, 2), (1, 4, 2, 1), (1, 1, 2, 3), (0, 0, 2, 2), (0, 0, 2, 1), (1, 2, 2, 4), (1, 3, 2, 2), (1, 1, 2, 3)),
    "mt19937": ((1, 1, 2, 2), (1, 1, 2, 1), (0, 1, 2, 3), (1, 3, 2, 4), (1, 2, 2, 2), (1, 2, 3, 1), (1, 2, 2, 2), (1, 1, 3, 1)),
}


def actions(mode):
    """int32 [T][N_ENVS]"""
    a = np.full((T, N_ENVS), 4, np.int32)
    for e, (ax, k, ay, m) in enumerate(PREFIX[mode]):
        a[:k, e] = ax
        a[k:k + m, e] = ay
    return a


def record(mode):
    from srlhip import _lib
    cfg = _lib.default_config(_lib.ENV_KUKA_BUTTON)
    cfg.num_envs, cfg.seed0, cfg.auto_reset = N_ENVS, SEED0, 1
    cfg.rng_mode = _lib.RNG_PHILOX if mode == "philox" else _lib.RNG_MT19937
    h = _lib.Handle(cfg)
    try:
        obs0 = h.reset()
        out = h.rollout(T, actions=actions(mode))
        return {"obs0": np.asarray(obs0), "obs": out["obs"], "reward": out["reward"], "done": out["done"],
                "q": h.get_state(_lib.F_KUKA_Q), "qd": h.get_state(_lib.F_KUKA_QD)}
    finally:
        h.close()


def oracle_rows(mode):
    """(rows [T][N_ENVS] contact-normal rows per env-step, joint-limit rows in the whole rollout) by the CPU oracle; no GPU."""
    from oracle import kuka_clib
    full = kuka_clib.is_full()
    kuka_clib.set_full(True)
    try:
        o = kuka_clib.rollout(SEED0 + np.arange(N_ENVS), T, actions=actions(mode), aux=True, trace=False,
                              rng_mode=kuka_clib.RNG_PHILOX if mode == "philox" else kuka_clib.RNG_MT19937)
    finally:
        kuka_clib.set_full(full)
    return o["rows"][:, :, 0].astype(np.int32), int((o["rows"][:, :, 1] >= 1000).sum())


def check_counts(rows, nlimit):
    """the conditions of the module docstring on one stream's rows; returns slots [T][2]"""
    assert nlimit == 0 and rows.max() <= 2
    slots = rows.reshape(T, N_ENVS // WAVE_ENVS, WAVE_ENVS).max(axis=2).astype(np.int32)
    for w in range(N_ENVS // WAVE_ENVS):
        assert (slots[:, w] == 1).any() and (slots[:, w] == 2).any(), w            # cn_sweeps<1> and cn_sweeps<2> in each wavefront
    w0 = rows[:, :WAVE_ENVS] > 0
    assert ((w0.sum(axis=1) == 1).any() and (w0.sum(axis=1) == 2).any())            # one env alone; two envs on the same steps
    starts = sorted(int(np.flatnonzero(w0[:, e])[0]) for e in range(WAVE_ENVS) if w0[:, e].any())
    assert len(starts) == WAVE_ENVS and len(set(starts)) >= 3, starts               # every env presses; different start steps
    return slots


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "kuka_tree_contact_bits.npz")
    planes = {}
    for mode in MODES:
        rows, nlimit = oracle_rows(mode)
        planes[mode + "_rows"], planes[mode + "_slots"], planes[mode + "_actions"] = rows, check_counts(rows, nlimit), actions(mode)
        for k, v in record(mode).items():
            planes[mode + "_" + k] = v
    np.savez_compressed(path, **planes)
    print(path, os.path.getsize(path), "bytes", {k: (v.shape, str(v.dtype)) for k, v in planes.items()})
    for mode in MODES:
        s = planes[mode + "_slots"]
        print(mode, "wavefront-steps with 1 / 2 normal slots:", [(int((s[:, w] == 1).sum()), int((s[:, w] == 2).sum())) for w in range(s.shape[1])])


if __name__ == "__main__":
    main()
