"""Record tests/golden/kuka_tree_rollout_bits.npz: the exact bytes of a fused full-model KukaButton rollout (the configuration-
specialised kernel bench.py times, device-sampled random actions) for both env RNG streams, Philox and MT19937.

Per stream: obs / reward / done / actions of every step and the final joint positions / velocities, 32 envs x 1100 steps
(past the 1000-step episode limit, so an auto-reset is inside).  tests/test_gpu_kuka_rollout_bits.py re-runs the same rollout
and asserts byte equality: a change to the kernel that moves one bit of the trajectory fails it.

Run on a GPU box from the repository root:  python tests/golden/make_kuka_tree_rollout_bits.py [out.npz]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

N_ENVS, T, SEED0 = 32, 1100, 11
MODES = ("philox", "mt19937")


def record(mode):
    from srlhip import _lib
    cfg = _lib.default_config(_lib.ENV_KUKA_BUTTON)
    cfg.num_envs, cfg.seed0, cfg.auto_reset = N_ENVS, SEED0, 1
    cfg.rng_mode = _lib.RNG_PHILOX if mode == "philox" else _lib.RNG_MT19937
    h = _lib.Handle(cfg)
    try:
        obs0 = h.reset()
        out = h.rollout(T)
        return {"obs0": np.asarray(obs0), "obs": out["obs"], "reward": out["reward"], "done": out["done"],
                "actions": out["actions"], "q": h.get_state(_lib.F_KUKA_Q), "qd": h.get_state(_lib.F_KUKA_QD)}
    finally:
        h.close()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "kuka_tree_rollout_bits.npz")
    planes = {}
    for mode in MODES:
        for k, v in record(mode).items():
            planes[mode + "_" + k] = v
    np.savez_compressed(path, **planes)
    print(path, os.path.getsize(path), "bytes", {k: (v.shape, str(v.dtype)) for k, v in planes.items()})


if __name__ == "__main__":
    main()
