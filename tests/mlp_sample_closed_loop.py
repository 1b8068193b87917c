"""The CPU oracles run closed-loop under the numpy contract of the SAMPLED MLP policy (tests/mlp_sample_ref.py; no GPU): how the
parameter seeds of tests/test_gpu_mlp_policy_sampled.py were chosen.  A seed is good when at least 5 % of the live steps of the closed
loop take another action than argmax(score) — otherwise a kernel that ignored its draw would pass the sampling check — and, for the
Kuka cases, when no env-step carries the IK conditioning flag, so that the GPU test compares every step with the oracle.

    python tests/mlp_sample_closed_loop.py             (prints, for every case, the first candidate seed that qualifies)

The loops are closed as in tests/kuka_mlp_closed_loop.py: the oracle's rollout is re-run on a growing action plane, one step at a time."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import kuka_mlp_closed_loop as kcl  # noqa: E402
import mlp_policy_ref as ref  # noqa: E402
import mlp_sample_ref as sref  # noqa: E402

MIN_OFF_ARGMAX = 0.05

MOBILE_T, MOBILE_ENV_SEED = 300, 17
MOBILE_MEAN, MOBILE_STD, MOBILE_CLIP = np.array([-0.3, 0.45]), np.array([0.7, 1.9]), 1.5
MOBILE_CASES = [
    # kind, rng, n, H, per_env, normalize, freeze
    (0, "MT19937", 257, 100, 1, 0, 0),
    (0, "PHILOX", 1, 5, 1, 0, 1),
    (0, "PHILOX", 65, 128, 0, 1, 1),
    (1, "PHILOX", 257, 128, 1, 0, 0),
    (1, "MT19937", 65, 5, 1, 1, 1),
    (1, "MT19937", 1, 100, 0, 0, 0),
    (2, "MT19937", 257, 5, 1, 0, 1),
    (2, "PHILOX", 65, 100, 0, 1, 0),
    (3, "PHILOX", 257, 100, 1, 1, 1),
    (3, "MT19937", 1, 128, 1, 0, 0),
]
# env, discrete, joints, rng, n, H, per_env, normalize, freeze (kuka_mlp_closed_loop's layout; discrete actions only)
KUKA_CASES = [
    ("KUKA_BUTTON", 1, 0, "PHILOX", 1, 5, 1, 0, 0),
    ("KUKA_BUTTON", 1, 0, "MT19937", 9, 100, 1, 1, 1),
    ("KUKA_MOVING", 1, 0, "MT19937", 5, 100, 1, 0, 0),
    ("KUKA_MOVING", 1, 0, "PHILOX", 9, 128, 0, 1, 1),
    ("KUKA_2BUTTON", 1, 0, "PHILOX", 9, 100, 1, 0, 1),
    ("KUKA_2BUTTON", 1, 0, "MT19937", 5, 5, 0, 1, 0),
]


def mobile_dims(kind):
    return (1, 2) if kind == 1 else (2, 4)


def mobile_params(case, seed):
    kind, rng, n, H, per_env, normalize, freeze = case
    D, A = mobile_dims(kind)
    P = ref.param_count(D, H, A)
    return ref.random_params(seed, (n, P) if per_env else (P,))


def mobile_closed_loop(case, seed):
    """-> (fraction of live steps whose sampled action is not argmax(score), live steps)"""
    from oracle import clib
    kind, rng, n, H, per_env, normalize, freeze = case
    D, A = mobile_dims(kind)
    W = mobile_params(case, seed)
    seeds = MOBILE_ENV_SEED + np.arange(n)
    u = sref.draws(seeds, 0, MOBILE_T)
    acts = np.zeros((MOBILE_T, n), np.int32)

    def run(steps):
        return clib.mobile_rollout(kind, seeds, steps, actions=acts[:steps], is_discrete=True, random_target=True, rng_mode=getattr(clib, "RNG_" + rng))

    prev = run(1)["obs0"]
    frozen = np.zeros(n, bool)
    off = live = 0
    for t in range(MOBILE_T):
        x = ref.normalise(prev, MOBILE_MEAN[:D] if normalize else None, MOBILE_STD[:D], MOBILE_CLIP)
        sc, _ = ref.forward(W, x, D, H, A)
        a = sref.contract(sc, u[t])
        off += int(((a != sc.argmax(1)) & ~frozen).sum())
        live += int((~frozen).sum())
        acts[t] = np.where(frozen, -1, a)
        o = run(t + 1)
        prev = o["obs"][t]
        if freeze:
            frozen |= (o["done"][t] & 1) != 0
    return off / max(live, 1), live


def kuka_closed_loop(case, seed, T=kcl.T):
    """-> (fraction of live steps off the argmax, flagged env-steps of the oracle's closed loop)"""
    env, discrete, joints, rng, n, H, per_env, normalize, freeze = case
    W = kcl.params_for(case, seed)
    u = sref.draws(kcl.ENV_SEED + np.arange(n), 0, T)
    acts = np.zeros((T, n), np.int32)
    prev = kcl.oracle_rollout(case, acts, 1)["obs0"]
    frozen = np.zeros(n, bool)
    off = live = 0
    for t in range(T):
        x = ref.normalise(prev, kcl.MEAN if normalize else None, kcl.STD, kcl.CLIP)
        sc, _ = ref.forward(W, x, 3, H, 6)
        a = sref.contract(sc, u[t])
        off += int(((a != sc.argmax(1)) & ~frozen).sum())
        live += int((~frozen).sum())
        acts[t] = np.where(frozen, -1, a)
        o = kcl.oracle_rollout(case, acts, t + 1, ik_trace=(t == T - 1))
        prev = o["obs"][t]
        if freeze:
            frozen |= (o["done"][t] & 1) != 0
    return off / max(live, 1), int(np.asarray(o["ik_crossed"]).sum())


if __name__ == "__main__":
    from oracle import kuka_clib
    for case in MOBILE_CASES:
        for seed in range(4000, 4040):
            frac, live = mobile_closed_loop(case, seed)
            print(("" if frac >= MIN_OFF_ARGMAX else "    ") + "mobile", case, "seed", seed, "off-argmax {:.3f} of {} live steps".format(frac, live), flush=True)
            if frac >= MIN_OFF_ARGMAX:
                break
    was_full = kuka_clib.is_full()
    kuka_clib.set_full(True)
    try:
        for case in KUKA_CASES:
            for seed in range(5000, 5040):
                frac, flags = kuka_closed_loop(case, seed)
                good = frac >= MIN_OFF_ARGMAX and flags == 0
                print(("" if good else "    ") + "kuka", case, "seed", seed, "off-argmax {:.3f}".format(frac), "flags", flags, flush=True)
                if good:
                    break
    finally:
        kuka_clib.set_full(was_full)
