"""GPU: the reference's `None` action in the CONTINUOUS Kuka action modes (kuka_button_gym_env.py:293-299), carried as a row of NaNs
(include/srlhip.h): no noise draw, Cartesian -> zero increment, joints -> targets held at joint_positions[:7]; the moving button, the
counter, reward and termination go on as for the discrete `None` (-1).  Pinned to the reference's own wrapper source
(tests/golden/kuka_none_reference.npz), to the RNG_HOST harness (draw accounting), to the discrete `None`, and across every path that
takes a caller's actions."""
import os
import time
import types

import numpy as np
import pytest
import torch

from srlhip import _lib

pytestmark = pytest.mark.gpu

KUKA_IDS = {"KukaButtonGymEnv-v0": _lib.ENV_KUKA_BUTTON, "KukaMovingButtonGymEnv-v0": _lib.ENV_KUKA_MOVING,
            "Kuka2ButtonGymEnv-v0": _lib.ENV_KUKA_2BUTTON, "KukaRandButtonGymEnv-v0": _lib.ENV_KUKA_RAND}
NOISE_STD_CONTINUOUS, NOISE_STD_JOINTS = 0.0001, 0.002        # kuka_button_gym_env.py:32-33


def make(kind=_lib.ENV_KUKA_BUTTON, n=1, **kw):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.is_discrete, cfg.rng_mode = n, 0, _lib.RNG_MT19937
    for k, v in kw.items():
        setattr(cfg, k, v)
    return _lib.Handle(cfg)


def none_actions(T, n, adim, seed, frac=0.3):
    """uniform actions with ~frac `None` rows: every env's first step, and a run of six per env"""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-1, 1, size=(T, n, adim)).astype(np.float32)
    none = rs.rand(T, n) < frac
    none[0] = True
    for i in range(n):
        s = rs.randint(5, T - 10)
        none[s:s + 6, i] = True
    a[none] = np.nan
    return a, none


# ---- 1. pinned to the reference ------------------------------------------------------------------------------------------------------
def test_ee_target_matches_reference_none_steps(golden_dir):
    g = np.load(os.path.join(golden_dir, "kuka_none_reference.npz"))
    tags = sorted({k.rsplit("|", 1)[0] for k in g.files if "|continuous|" in k})
    assert len(tags) == 2 * 3 * 4
    for tag in tags:
        env, _, s, rt, fd = tag.split("|")
        h = make(_lib.ENV_KUKA_BUTTON if env == "button" else _lib.ENV_KUKA_MOVING, 1, auto_reset=0, seed0=int(s[1:]),
                 random_target=int(rt == "rt1"), force_down=int(fd == "fd1"))
        h.reset()
        assert np.array_equal(h.get_state(_lib.F_KUKA_EE_TARGET)[:, 0], g[tag + "|reset_ik"][-1]), tag
        acts, ik = g[tag + "|actions"].astype(np.float32), g[tag + "|ik"]
        compared = 0
        for t in range(len(acts)):
            _, _, d = h.step(acts[t].reshape(1, 3))
            assert np.array_equal(h.get_state(_lib.F_KUKA_EE_TARGET)[:, 0], ik[t]), (tag, t)
            compared += 1
            if d[0]:
                break
        assert compared > 150, tag
        h.close()


# ---- 2. draw accounting --------------------------------------------------------------------------------------------------------------
# The lumped forms launch the RNG_HOST arms of the lumped-gripper kernels, which nothing else does: the lane-per-env kernel (one and two
# buttons: reset and the single-step launch), the lane-group kernel of the baked model, and the one of a runtime model table (reset and
# rollout; the table installed is the baked model's own) — n = 5, T = 3: a tail group of the wavefront shadows env 4.
LUMPED_FORMS = [pytest.param(j, f, id="{}-{}".format(j, f), marks=pytest.mark.lumped_kuka)
                for f in ("lumped_lane", "lumped_group", "lumped_table") for j in (0, 1)] + \
               [pytest.param(0, "lumped_two", id="0-lumped_two", marks=pytest.mark.lumped_kuka)]


@pytest.mark.parametrize("joints,form", [pytest.param(0, "full", id="0"), pytest.param(1, "full", id="1")] + LUMPED_FORMS)
def test_none_rows_draw_nothing(joints, form, monkeypatch):
    from oracle import gym_seeding
    adim = 7 if joints else 3
    kind, kw, lead = _lib.ENV_KUKA_BUTTON, {}, 0
    if form == "full":
        n, T = 64, 520
        acts, none = none_actions(T, n, adim, 31 + joints)
    else:
        n, T = 5, 3
        acts = np.random.RandomState(31 + joints).uniform(-1, 1, size=(T, n, adim)).astype(np.float32)
        none = np.zeros((T, n), bool)
        none[0] = True
        none[1, 2] = True
        acts[none] = np.nan
        kw = dict(kuka_model=_lib.KUKA_MODEL_LUMPED)
        monkeypatch.setenv("SRLHIP_KUKA_KERNEL", "lane" if form in ("lumped_lane", "lumped_two") else "group")
        if form == "lumped_two":
            kind, lead = _lib.ENV_KUKA_2BUTTON, 2          # kuka_2button_gym_env.py:55-70: two uniform draws in front of the init actions
    a = make(kind, n=n, auto_reset=0, seed0=200, action_joints=joints, **kw)
    b = make(kind, n=n, auto_reset=0, rng_mode=_lib.RNG_HOST, action_joints=joints, **kw)
    if form == "lumped_table":
        from oracle import kuka_clib
        from srlhip import kuka_model
        for h in (a, b):
            h.set_kuka_model(kuka_model.to_table(kuka_clib.get_model()))
    if form != "full":
        assert a.kuka_kernel() == b.kuka_kernel() == ("lane" if form in ("lumped_lane", "lumped_two") else "group")
    rngs = [gym_seeding.np_random(200 + i)[0] for i in range(n)]
    rand = np.zeros((n, b.reset_rand_count))
    assert b.reset_rand_count == lead + 5
    for i, r in enumerate(rngs):
        rand[i, :lead] = [r.uniform(-1, 1) for _ in range(lead)]
        rand[i, lead:lead + 5] = [float(r.normal((7,) if joints else (3,))[0]) for _ in range(5)]
    assert np.array_equal(a.reset(), b.reset(host_rand=rand))
    std = NOISE_STD_JOINTS if joints else NOISE_STD_CONTINUOUS
    for t in range(T):
        noise = np.array([0.0 if none[t, i] else r.normal(0.0, scale=std) for i, r in enumerate(rngs)])
        oa, ra, da = a.step(acts[t])
        ob, rb, db = b.step(np.where(none[t][:, None], np.float32(0), acts[t]), host_noise=noise)
        assert np.array_equal(oa, ob) and np.array_equal(ra, rb) and np.array_equal(da, db), t
        if t % 50 == 0 or t == T - 1:
            # the IK target is the wrapper's own arithmetic on the drawn noise: bit for bit (a draw out of place moves it by ~1e-4);
            # the joint state comes out of two instantiations of the stepper (MT19937 / RNG_HOST): the documented 1e-11 bar on the
            # joints, and that bar over one physics step (dt = 1/240 s) on their velocities
            assert np.array_equal(a.get_state(_lib.F_KUKA_EE_TARGET), b.get_state(_lib.F_KUKA_EE_TARGET)), t
            assert np.abs(a.get_state(_lib.F_KUKA_Q) - b.get_state(_lib.F_KUKA_Q)).max() <= 1e-11, t
            assert np.abs(a.get_state(_lib.F_KUKA_QD) - b.get_state(_lib.F_KUKA_QD)).max() <= 240 * 1e-11, t
    a.close(); b.close()


# ---- 3. cross-mode: the continuous `None` is the discrete one ------------------------------------------------------------------------
def test_continuous_none_equals_discrete_none():
    n, T = 32, 300
    c = make(n=n, auto_reset=0, seed0=7)
    d = make(n=n, auto_reset=0, seed0=7, is_discrete=1)
    c.reset(); d.reset()
    # the two action modes start from different reset states (their init actions differ): hand the continuous one's over
    for f in (_lib.F_KUKA_BUTTON_XY, _lib.F_KUKA_BUTTON_Q, _lib.F_KUKA_BUTTON_POS, _lib.F_KUKA_EE_TARGET, _lib.F_KUKA_QD,
              _lib.F_KUKA_GRIPPER_QD, _lib.F_KUKA_GRIPPER_Q, _lib.F_KUKA_Q):
        d.set_state(f, c.get_state(f))
    nan = np.full((n, 3), np.nan, np.float32)
    for t in range(T):
        oc, rc, dc = c.step(nan)
        od, rd, dd = d.step(np.full(n, -1, np.int32))
        assert np.array_equal(oc, od) and np.array_equal(rc, rd) and np.array_equal(dc, dd), t
    for f in (_lib.F_KUKA_Q, _lib.F_KUKA_QD, _lib.F_KUKA_EE_TARGET, _lib.F_KUKA_COUNTERS):
        assert np.array_equal(c.get_state(f), d.get_state(f)), f
    c.close(); d.close()


# ---- 4. every path -------------------------------------------------------------------------------------------------------------------
def run_steps(h, acts, mode):
    obs, rew, done = [], [], []
    for t in range(len(acts)):
        if mode == "async":
            h.step_async(acts[t])
            o, r, d = h.step_wait()
        else:
            o, r, d = h.step(acts[t])
        obs.append(o.copy()); rew.append(r.copy()); done.append(d.copy())
        if mode == "persist" and t == len(acts) // 2:
            time.sleep(0.02)                                   # > park_us: the resident kernel parks, the next step restarts it
    return {"obs": np.array(obs), "reward": np.array(rew), "done": np.array(done)}


def same(a, b, what):
    for k in ("obs", "reward", "done"):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("env_id", sorted(KUKA_IDS))
def test_every_path_agrees(env_id):
    from srlhip.device_env import DeviceVecEnv
    from srlhip.vec_env import HipVecEnv
    kind, n, T, seed = KUKA_IDS[env_id], 64, 160, 11
    acts, _ = none_actions(T, n, 3, 5)
    h = make(kind, n, seed0=seed)
    h.reset()
    ref = run_steps(h, acts, "step")
    q_ref = h.get_state(_lib.F_KUKA_Q)
    h.close()
    h = make(kind, n, seed0=seed)
    h.reset()
    same(ref, run_steps(h, acts, "async"), "step_async")
    h.close()
    h = make(kind, n, seed0=seed)
    h.reset()
    out = h.rollout(T, actions=acts)
    same(ref, out, "rollout")
    assert np.array_equal(h.get_state(_lib.F_KUKA_Q), q_ref)
    h.close()
    if kind in (_lib.ENV_KUKA_BUTTON, _lib.ENV_KUKA_MOVING):
        h = make(kind, n, seed0=seed)
        h.reset()
        h.set_persistent(True, 500)
        same(ref, run_steps(h, acts, "persist"), "persistent")
        h.set_persistent(False)
        assert np.array_equal(h.get_state(_lib.F_KUKA_Q), q_ref)
        h.close()
    dev = DeviceVecEnv(env_id, n, seed=seed, env_kwargs={"srl_model": "ground_truth", "is_discrete": False}, rng_mode="mt19937")
    dev.reset()
    got = {"obs": [], "reward": [], "done": []}
    for t in range(T):
        o, r, d = dev.step(torch.from_numpy(acts[t]).to(dev.device))
        got["obs"].append(o.cpu().numpy()); got["reward"].append(r.cpu().numpy()); got["done"].append(d.cpu().numpy())
    same(ref, {k: np.array(v) for k, v in got.items()}, "device pointers")
    dev.close()
    env = HipVecEnv(env_id, n, seed=seed, env_kwargs={"srl_model": "ground_truth", "is_discrete": False}, device_ids=[0, 0, 0, 0],
                    rng_mode="mt19937")
    env.reset()
    for t in range(T):
        o, r, d, _ = env.step(acts[t])
        assert np.array_equal(o, ref["obs"][t]) and np.array_equal(r, ref["reward"][t]) and np.array_equal(d, ref["done"][t] & 1 != 0), t
    env.close()


@pytest.mark.parametrize("env_kind", [_lib.ENV_KUKA_BUTTON, _lib.ENV_KUKA_MOVING])
def test_occ_kernel_agrees(env_kind, monkeypatch):
    n, T = 128, 300
    acts, _ = none_actions(T, n, 3, 8)
    outs, qs = [], []
    for occ in ("0", "1"):
        monkeypatch.setenv("SRLHIP_KUKA_OCC", occ)
        h = make(env_kind, n, seed0=3)
        h.reset()
        outs.append(h.rollout(T, actions=acts))
        qs.append(h.get_state(_lib.F_KUKA_Q))
        h.close()
    assert np.array_equal(outs[0]["done"], outs[1]["done"]) and np.array_equal(outs[0]["reward"], outs[1]["reward"])
    assert np.abs(qs[0] - qs[1]).max() <= 1e-11


# The short forms launch the lane-group instantiations that no other test does — actions drawn on the device (GIVEN = false), and the
# kernels of a runtime model table (CM = true; the table installed is the baked model's own, so the lane kernel stays the reference) —
# on n = 5, T = 3: one full wavefront plus a tail group that shadows env 4.
@pytest.mark.lumped_kuka
@pytest.mark.parametrize("joints,form", [pytest.param(0, "given", id="0"), pytest.param(1, "given", id="1")] +
                         [pytest.param(j, f, id="{}-{}".format(j, f)) for j in (0, 1) for f in ("drawn", "table_given", "table_drawn")])
def test_lumped_lane_and_group_kernels_agree(joints, form, monkeypatch):
    from srlhip import kuka_model
    n, T, adim = (128, 300, 7 if joints else 3) if form == "given" else (5, 3, 7 if joints else 3)
    acts = none_actions(T, n, adim, 9)[0] if form == "given" else np.random.RandomState(9).uniform(-1, 1, size=(T, n, adim)).astype(np.float32)
    outs, qs = [], []
    for kernel in ("lane", "group"):
        monkeypatch.setenv("SRLHIP_KUKA_KERNEL", kernel)
        h = make(n=n, seed0=4, action_joints=joints, kuka_model=_lib.KUKA_MODEL_LUMPED)
        if kernel == "group" and form.startswith("table"):
            from oracle import kuka_clib
            h.set_kuka_model(kuka_model.to_table(kuka_clib.get_model()))
        assert h.kuka_kernel() == kernel
        h.reset()
        outs.append(h.rollout(T, actions=None if form.endswith("drawn") else acts))
        qs.append(h.get_state(_lib.F_KUKA_Q))
        h.close()
    assert np.array_equal(outs[0]["done"], outs[1]["done"]) and np.array_equal(outs[0]["reward"], outs[1]["reward"])
    if form.endswith("drawn"):
        assert np.array_equal(outs[0]["actions"], outs[1]["actions"])
    assert np.abs(qs[0] - qs[1]).max() <= 1e-11


# ---- 5. boundary ---------------------------------------------------------------------------------------------------------------------
def test_boundary():
    from srlhip.envs import KukaButtonGymEnv
    from srlhip.vec_env import HipVecEnv
    h = make(n=4)
    h.reset()
    a = np.zeros((4, 3), np.float32)
    a[1] = np.nan
    h.step(a)                                                  # an all-NaN row is `None`
    h.rollout(2, actions=np.stack([a, a]))
    for bad in (np.nan, np.inf, -np.inf):
        b = a.copy()
        b[2, 1] = bad
        with pytest.raises(_lib.SrlHipError):
            h.step(b)
        with pytest.raises(_lib.SrlHipError):
            h.rollout(2, actions=np.stack([b, b]))
    b = a.copy()
    b[1, 2] = 0.5                                              # partly NaN
    with pytest.raises(_lib.SrlHipError):
        h.step(b)
    h.close()
    m = _lib.default_config(_lib.ENV_MOBILE)
    m.num_envs, m.is_discrete = 4, 0
    hm = _lib.Handle(m)
    hm.reset()
    with pytest.raises(_lib.SrlHipError):
        hm.step(np.full((4, 2), np.nan, np.float32))           # MobileRobot: no continuous `None` in the reference
    hm.close()
    with HipVecEnvCtx("MobileRobotGymEnv-v0") as env:
        with pytest.raises(NotImplementedError):
            env.step([None, [0.1, 0.2], [0.0, 0.0], [1.0, -1.0]])
    for joints in (False, True):
        dim = 7 if joints else 3
        with HipVecEnvCtx("KukaButtonGymEnv-v0", action_joints=joints, device_ids=[0, 0]) as env:
            env.step([None, np.ones(dim) * 0.5, None, np.zeros(dim)])
            env.step(np.full((4, dim), np.nan, np.float32))
            part = np.zeros((4, dim), np.float32)
            part[3, 0] = np.nan
            steps0 = [sh.h.get_state(_lib.F_EP_LENGTH).copy() for sh in env._shards]
            with pytest.raises(_lib.SrlHipError):
                env.step(part)                                 # refused before any shard launched
            assert all(np.array_equal(s, sh.h.get_state(_lib.F_EP_LENGTH)) for s, sh in zip(steps0, env._shards))
        f = KukaButtonGymEnv(is_discrete=False, action_joints=joints, srl_model="ground_truth")
        f.saver = types.SimpleNamespace(actions=[], step=lambda img, action, r, d, gt: f.saver.actions.append(action),
                                        reset=lambda *a: None)
        f.render = lambda mode="rgb_array": None
        f.reset()
        first = np.full(dim, 0.25, np.float32)
        f.step(first)
        ee = f._h.get_state(_lib.F_KUKA_EE_TARGET).copy()
        f.step(None)
        assert f.saver.actions[-1] is first                    # the saver records the previous action
        if not joints:
            assert np.array_equal(f._h.get_state(_lib.F_KUKA_EE_TARGET), ee)
        f.close()


class HipVecEnvCtx(object):
    def __init__(self, env_id, action_joints=False, device_ids=None):
        from srlhip.vec_env import HipVecEnv
        self.env = HipVecEnv(env_id, 4, seed=1, env_kwargs={"srl_model": "ground_truth", "is_discrete": False,
                                                              "action_joints": action_joints}, device_ids=device_ids)

    def __enter__(self):
        self.env.reset()
        return self.env

    def __exit__(self, *a):
        self.env.close()


# ---- 6. learners ---------------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def check_learner(model, args, members):
    state = {"r": None, "prev": None, "iters": 0, "bad": 0, "nan_rows": 0, "live_rows": 0}

    def cb(l, g):
        if l["r"] is not state["r"]:                           # a new iteration: nobody finished yet
            state["iters"] += 1
            if state["iters"] > 2:
                raise _Stop()
            state["r"], state["prev"] = l["r"], torch.zeros(members, dtype=torch.bool, device=l["r"].device)
        a = l["actions"]
        all_nan, any_nan = torch.isnan(a).all(1), torch.isnan(a).any(1)
        prev = state["prev"]
        state["bad"] += int(((all_nan != prev) | (any_nan != prev)).sum())
        state["nan_rows"] += int(prev.sum())
        state["live_rows"] += int((~prev).sum())
        state["prev"] = l["done"].clone()

    with pytest.raises(_Stop):
        model.train(args, callback=cb, env_kwargs={"srl_model": "ground_truth", "is_discrete": False, "max_distance": 0.28})
    assert state["iters"] == 3 and state["bad"] == 0 and state["nan_rows"] > 0 and state["live_rows"] > 0, state


def test_ars_sends_none_rows_for_finished_directions():
    from rl_baselines.evolution_strategies.ars import ARSModel
    args = types.SimpleNamespace(env="KukaButtonGymEnv-v0", seed=0, num_population=4, top_population=2, step_size=0.05,
                                 exploration_noise=3.0, max_step_amplitude=10, deterministic=True, algo_type="v2", num_stack=1,
                                 srl_model="ground_truth", continuous_actions=True, num_timesteps=10 ** 7)
    check_learner(ARSModel(), args, 8)


def test_cma_es_sends_none_rows_for_finished_members(tmp_path):
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    args = types.SimpleNamespace(env="KukaButtonGymEnv-v0", seed=0, num_population=8, mu=0.0, sigma=2.0, cuda=True,
                                 deterministic=True, num_stack=1, srl_model="ground_truth", continuous_actions=True,
                                 num_timesteps=10 ** 7, log_dir=str(tmp_path))
    check_learner(CMAESModel(), args, 8)
