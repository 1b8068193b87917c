"""The front end's refusals and grow-only buffers on the device (csrc/api.hip over csrc/api_rules.hpp): a refused call answers with the
code and message the host program printed for that rule and leaves the handle as it was — its next step equals, bit for bit, the step
of a twin that never saw the refused calls; and a staging buffer that is regrown and then reused smaller hands back what a fresh
handle's does."""
import ctypes

import numpy as np
import pytest

import api_rules_lines
from srlhip import _lib

pytestmark = pytest.mark.gpu
N, T = 5, 3
EINVAL, ENOTSUP = -22, -95


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    api_rules_lines.build()
    return api_rules_lines.verdicts(api_rules_lines.run("api_rules_hostcheck", tmp_path_factory.mktemp("rules")))


def make(kind, discrete=1, **kw):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.seed0, cfg.is_discrete, cfg.rng_mode = N, 11, discrete, _lib.RNG_PHILOX
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = _lib.Handle(cfg)
    h.reset()
    return h


def actions_for(h, seed, lead=()):
    rs = np.random.RandomState(seed)
    if h.cfg.is_discrete:
        return rs.randint(h.num_actions, size=lead + (N,)).astype(np.int32)
    return rs.uniform(-1, 1, size=lead + (N, h.action_dim)).astype(np.float32)


def refused(h, rc, want_code, want_msg):
    assert rc == want_code, (rc, h.last_error())
    assert h.last_error() == want_msg


def policy_struct(cls, **fields):
    pol = cls()
    pol.struct_size, pol.clip_obs = ctypes.sizeof(cls), 10.0
    for k, v in fields.items():
        setattr(pol, k, v)
    return pol


@pytest.mark.parametrize("kind,discrete", [(_lib.ENV_MOBILE, 1), (_lib.ENV_MOBILE, 0), (_lib.ENV_KUKA_BUTTON, 1), (_lib.ENV_KUKA_BUTTON, 0)])
def test_refused_calls_leave_the_handle_as_it_was(printed, kind, discrete):
    h, twin = make(kind, discrete), make(kind, discrete)
    lib, hh = h._lib, h._h
    kuka = kind == _lib.ENV_KUKA_BUTTON
    a = actions_for(h, 1)
    obs, rew, done = h.new_obs(), np.zeros(N, np.float32), np.zeros(N, np.uint8)
    step = lambda act, noise=None: lib.srlhip_step(hh, _lib._ptr(act), _lib._ptr(noise), _lib._ptr(obs), _lib._ptr(rew), _lib._ptr(done))
    # the action plane
    if discrete:
        for value in (-2, h.num_actions):
            bad = a.copy()
            bad[3] = value
            refused(h, step(bad), EINVAL, "step: discrete action out of range (valid: -1 = no-op, 0 .. num_actions - 1)")
    else:
        for col, value in ((0, np.nan), (h.action_dim - 1, np.inf)):
            bad = a.copy()
            bad[2, col] = value
            refused(h, step(bad), EINVAL, "step: non-finite continuous action (a Kuka env's `None` is a row of NaNs)")
            refused(h, lib.srlhip_rollout(hh, 1, _lib._ptr(bad[None].copy()), None, None, None, None), EINVAL,
                    "rollout: non-finite continuous action (a Kuka env's `None` is a row of NaNs)")
        if not kuka:                                   # MobileRobot has no `None` row
            refused(h, step(np.full_like(a, np.nan)), EINVAL, "step: non-finite continuous action (a Kuka env's `None` is a row of NaNs)")
    noise = np.zeros(N)
    noise[4] = np.inf
    refused(h, step(a, noise), EINVAL, "step: non-finite host_noise")
    refused(h, lib.srlhip_step_wait(hh, _lib._ptr(obs), _lib._ptr(rew), _lib._ptr(done)), EINVAL, "step_wait: no srlhip_step_async is pending")
    # the policy structs: every tail is the host program's, behind the entry point's name
    D, A = h.obs_dim, h.num_actions if discrete else h.action_dim
    w64, w32 = np.zeros((N, D, A)), np.zeros((N, 4 * D + 4 + A * 4 + A), np.float32)
    mean, std = np.zeros(D), np.ones(D)
    planes = (None, None, None, None)
    tail = lambda key: printed[key]
    lin = lambda **f: policy_struct(_lib.LinearPolicy, **dict(dict(per_env=1, weights=w64.ctypes.data), **f))
    mlp = lambda **f: policy_struct(_lib.MlpPolicy, **dict(dict(per_env=1, hidden=4, params=w32.ctypes.data), **f))
    calls = [
        ("rollout_policy", lib.srlhip_rollout_policy, None, "policy-abi linear null"),
        ("rollout_policy", lib.srlhip_rollout_policy, lin(struct_size=40), "policy-abi linear 40"),
        ("rollout_policy", lib.srlhip_rollout_policy, lin(weights=None), "policy-pointers weights 0 0 0 0"),
        ("rollout_policy", lib.srlhip_rollout_policy, lin(normalize=1, obs_std=std.ctypes.data), "policy-pointers weights 1 1 0 1"),
        ("rollout_mlp_policy", lib.srlhip_rollout_mlp_policy, None, "policy-abi mlp null"),
        ("rollout_mlp_policy", lib.srlhip_rollout_mlp_policy, mlp(struct_size=48), "policy-abi mlp 48"),
        ("rollout_mlp_policy", lib.srlhip_rollout_mlp_policy, mlp(hidden=0, reserved=1), "policy-shape mlp 0 1"),
        ("rollout_mlp_policy", lib.srlhip_rollout_mlp_policy, mlp(hidden=129), "policy-shape mlp 129 0"),
        ("rollout_mlp_policy_sampled", lib.srlhip_rollout_mlp_policy_sampled, mlp(reserved=1), "policy-shape mlp 100 1"),
        ("rollout_mlp_policy_sampled", lib.srlhip_rollout_mlp_policy_sampled, mlp(params=None), "policy-pointers params 0 0 0 0"),
        ("rollout_mlp_policy", lib.srlhip_rollout_mlp_policy, mlp(normalize=1, obs_mean=mean.ctypes.data), "policy-pointers params 1 1 1 0"),
    ]
    if not discrete:                                   # the one by-name refusal a default handle can meet
        calls.append(("rollout_mlp_policy_sampled", lib.srlhip_rollout_mlp_policy_sampled, mlp(), "policy-config 1 1 0 {} 1 0 1".format(kind)))
    for name, fn, pol, key in calls:
        code, msg = tail(key)
        assert code != 0, key
        refused(h, fn(hh, T, None if pol is None else ctypes.byref(pol), *planes), code, name + ": " + msg)
    # ... and the values, checked on host-pointer handles only
    bad_w, bad_std = w64.copy(), std.copy()
    bad_w[1, 0, 0], bad_std[0] = np.nan, 0.0
    code, msg = tail("policy-values weights 0 1 0 0")
    refused(h, lib.srlhip_rollout_policy(hh, T, ctypes.byref(lin(weights=bad_w.ctypes.data)), *planes), code, "rollout_policy: " + msg)
    code, msg = tail("policy-values weights 1 0 0 3")
    refused(h, lib.srlhip_rollout_policy(hh, T, ctypes.byref(lin(normalize=1, obs_mean=mean.ctypes.data, obs_std=bad_std.ctypes.data)), *planes), code,
            "rollout_policy: " + msg)
    # srlhip_policy_act on a host-pointer handle: its struct checks fire first, then the handle is refused
    act_out = np.zeros(N * 8, np.float32)
    policy_act = lambda l, m, o=obs: lib.srlhip_policy_act(hh, None if l is None else ctypes.byref(l), None if m is None else ctypes.byref(m), 0, _lib._ptr(o), D,
                                                         None, None, _lib._ptr(act_out), None)
    for l, m, key in ((None, None, "act-which 0 0"), (lin(), mlp(), "act-which 1 1"), (None, mlp(hidden=0), "policy-shape mlp 0 0"),
                      (lin(weights=None), None, "policy-pointers weights 0 0 0 0"), (lin(), None, "act-planes 1 1 0 0 0 0 {}".format(discrete))):
        code, msg = tail(key)
        assert code != 0, key
        refused(h, policy_act(l, m), code, "policy_act: " + msg)
    # a bad model table
    lumped, tree = api_rules_lines.default_tables()
    tree[0] = 11.0                                     # nd
    if kuka:
        code, msg = tail("tree nd-11")
        refused(h, lib.srlhip_set_kuka_tree_model(hh, _lib._ptr(tree)), code, msg)
    else:
        refused(h, lib.srlhip_set_kuka_tree_model(hh, _lib._ptr(tree)), EINVAL, "set_kuka_tree_model: not a Kuka handle")
        refused(h, lib.srlhip_set_kuka_model(hh, _lib._ptr(lumped)), EINVAL, "set_kuka_model: not a Kuka handle")
    # one step: the twin never saw any of the above
    got, want = h.step(a), twin.step(a)
    for g, w, name in zip(got, want, ("obs", "reward", "done")):
        assert g.tobytes() == w.tobytes(), name
    for g, w in zip(h.episode_stats(), twin.episode_stats()):
        assert np.array_equal(g, w)
    h.close()
    twin.close()


@pytest.mark.parametrize("kind", [_lib.ENV_MOBILE, _lib.ENV_KUKA_BUTTON])
def test_regrown_staging_buffers_hand_back_what_a_fresh_handle_does(kind):
    """rollout with T = 2, 5, 2 and the 8 x 8 renders between them share the staging buffers: each regrows on the way up and is reused,
    larger than needed, on the way down"""
    seeds = 11 + np.arange(N)

    def restart(h):
        h.seed(seeds)
        h.reset()

    def fresh(call):
        f = make(kind, img_h=8, img_w=8)
        restart(f)
        out = call(f)
        f.close()
        return out

    h = make(kind, img_h=8, img_w=8)
    for t, cap in ((2, 1024), (5, 4096), (2, 1024)):
        a = actions_for(h, t, (t,))
        for call in (lambda x: x.rollout(t, actions=a), lambda x: x.rollout(t), lambda x: {"img": x.render()},
                     lambda x: {"jpeg": np.frombuffer(b"".join(s or b"overflow" for s in x.render_jpeg(cap_per_stream=cap)), np.uint8)}):
            restart(h)
            got, want = call(h), fresh(call)
            assert sorted(got) == sorted(want)
            for k in got:
                assert got[k].tobytes() == want[k].tobytes(), (t, k)
    h.close()
