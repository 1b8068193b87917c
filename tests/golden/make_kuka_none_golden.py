"""Generate tests/golden/kuka_none_reference.npz: the reference's `step(None)` in the CONTINUOUS Kuka action modes
(kuka_button_gym_env.py:293-299: Cartesian -> step2([0, 0, 0, 0, 0]), joints -> step2(joint_positions[:7] + [0, 0]); no draw from
np_random in either), run through the reference's own wrapper source against the scripted fake pybullet of
make_kuka_wrapper_golden.py.

Cases: KukaButtonGymEnv and KukaMovingButtonGymEnv, Cartesian continuous actions (force_down 0/1 x random_target 0/1) and joint-space
actions (random_target 0/1), seeds 0..2, T steps each; about 30 % of the steps are `None` — the first step after reset, two runs of
six, the rest at random.  Per case:
    actions   [T][adim] float64 copies of float32 values (make_kuka_wrapper_golden.py: numpy-version independent), NaN rows = None
    none      [T] bool
    ik        [T][3] the target handed to p.calculateInverseKinematics in the step (NaN in joint mode: no IK call)
    motor     [T][7] the arm's seven position targets of the step (joint mode; NaN otherwise)
    advanced  [T] bool, whether np_random's state moved during the step
    drawn     [T] the value np_random.normal returned in the step (NaN when nothing was drawn)
    reset_ik  [5][3] / reset_motor [5][7]: reset()'s five init actions
    n_steps   steps recorded (the scripted physics never ends an episode before T)

Run in the build container only, like the other generators:  PYTHONPATH=. python tests/golden/make_kuka_none_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_kuka_wrapper_golden as W  # noqa: E402  (installs the scripted pybullet, imports the reference's env classes)
from environments.kuka_gym.kuka_button_gym_env import KukaButtonGymEnv  # noqa: E402
from environments.kuka_gym.kuka_moving_button_gym_env import KukaMovingButtonGymEnv  # noqa: E402

T = 300
SEEDS = (0, 1, 2)


class DrawLog(object):
    """Stands in for env.np_random: forwards every call to the real RandomState and records what normal() returned."""

    def __init__(self, rng):
        self.rng, self.drawn = rng, []

    def normal(self, *a, **k):
        v = self.rng.normal(*a, **k)
        self.drawn.append(float(v))
        return v

    def __getattr__(self, name):
        return getattr(self.rng, name)


def none_mask(seed):
    r = np.random.RandomState(5150 + seed)
    m = r.rand(T) < 0.25
    m[0] = True                                    # the first step after reset
    a, b = 20 + r.randint(30), 150 + r.randint(60)
    m[a:a + 6] = True                              # runs of six
    m[b:b + 6] = True
    return m


def state_key(rng):
    s = rng.get_state()
    return s[1].tobytes() + bytes([s[2] & 0xff, (s[2] >> 8) & 0xff]) + np.float64(s[4]).tobytes() + bytes([s[3]])


def case(cls, seed, joints, random_target, force_down):
    kw = dict(srl_model="ground_truth", is_discrete=False, random_target=random_target, force_down=force_down)
    if joints:
        kw["action_joints"] = True
    env = cls(**kw)
    env.seed(seed)
    W.SCRIPT.reset(None, None, None)
    env.reset()
    out = {"reset_ik": np.array(W.SCRIPT.ik_targets[-5:]) if not joints else np.zeros((0, 3)),
           "reset_motor": np.array(W.SCRIPT.motor_targets[-35:]).reshape(5, 7) if joints else np.zeros((0, 7))}
    adim = 7 if joints else 3
    arng = np.random.RandomState(888 + seed)
    actions = arng.uniform(-1, 1, (T, adim)).astype(np.float32).astype(np.float64)
    none = none_mask(seed)
    actions[none] = np.nan
    real = env.np_random
    log = DrawLog(real)
    env.np_random = log
    ik, motor, advanced, drawn = [], [], [], []
    n = 0
    for t in range(T):
        W.SCRIPT.ik_targets, W.SCRIPT.motor_targets = [], []
        log.drawn = []
        before = state_key(real)
        a = None if none[t] else (actions[t].astype(np.float32) if joints else actions[t])
        _, _, d, _ = env.step(a)
        ik.append(W.SCRIPT.ik_targets[-1] if W.SCRIPT.ik_targets else np.full(3, np.nan))
        motor.append(W.SCRIPT.motor_targets[-7:] if joints else [np.nan] * 7)
        advanced.append(state_key(real) != before)
        assert len(log.drawn) <= 1
        drawn.append(log.drawn[0] if log.drawn else np.nan)
        n += 1
        if d:
            break
    out.update(actions=actions[:n], none=none[:n], ik=np.array(ik), motor=np.array(motor), advanced=np.array(advanced),
               drawn=np.array(drawn), n_steps=n)
    return out


def main():
    out = {}
    for env_name, cls in (("button", KukaButtonGymEnv), ("moving", KukaMovingButtonGymEnv)):
        for seed in SEEDS:
            for joints in (False, True):
                for random_target in (False, True):
                    for force_down in ((True,) if joints else (False, True)):
                        tag = "{}|{}|s{}|rt{}|fd{}".format(env_name, "joints" if joints else "continuous", seed, int(random_target),
                                                         int(force_down))
                        for k, v in case(cls, seed, joints, random_target, force_down).items():
                            out[tag + "|" + k] = v
    path = os.path.join(HERE, "kuka_none_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
