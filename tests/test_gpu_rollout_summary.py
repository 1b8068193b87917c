"""GPU checks of srlhip_rollout_policy_summary: the four fused policy rollouts returning per-env return, live-step count and the
moments of the live observations instead of the [T][N] planes.

The truth is tests/rollout_summary_ref.py (sequential float64 loops, the contract of include/srlhip.h) applied to the planes the
corresponding PLANE call returns on a twin handle with the same seed and arguments; those plane calls are held to the CPU oracle by
test_gpu_policy_rollout.py / test_gpu_mlp_policy_rollout.py and their sampled siblings.  Every equality is bit for bit.  After the
call both handles make one further plane call (3 steps, all planes compared: env state, env RNG and action-stream counters) and
their state fields are compared.

Shapes.  MobileRobot n = 130: a partial wavefront, and more than one workgroup of the MLP kernel (16 lanes per env, 256-lane blocks);
T = 300 passes the 251-step limit (first < T, an auto-reset inside the call), T = 40 leaves first = T.  Kuka n = 7: two wavefronts
of four envs, the second partly filled; T = 1010 passes KukaButton's 1001-step limit, T = 64 leaves envs without a done.
Kuka2Button's limit is 1500 steps, so T = 1010 does not end its episodes by the step limit: that case asserts what its planes show,
and a third length, T = 1510, is added for it so that it too is checked with a done in every env."""
import ctypes

import numpy as np
import pytest

from srlhip import _lib
import rollout_summary_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("ret", "length", "obs_sum", "obs_sqsum")
MOBILE_FIELDS = ("F_POS_X", "F_POS_Y", "F_TARGET_X", "F_TARGET_Y", "F_TARGET2_X", "F_TARGET2_Y", "F_STEP_COUNT", "F_CUR_TARGET",
                 "F_EP_RETURN", "F_EP_LENGTH", "F_LAST_REWARD", "F_LAST_RETURN", "F_LAST_LENGTH", "F_N_FINISHED")
KUKA_FIELDS = ("F_KUKA_Q", "F_KUKA_QD", "F_KUKA_GRIPPER_Q", "F_KUKA_COUNTERS", "F_EP_RETURN", "F_EP_LENGTH", "F_LAST_RETURN",
               "F_LAST_LENGTH", "F_N_FINISHED", "F_LAST_REWARD")
RNG = {"PHILOX": _lib.RNG_PHILOX, "MT19937": _lib.RNG_MT19937}


def make(kind, n, rng_mode, seed0=0, **kw):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.rng_mode, cfg.auto_reset, cfg.seed0 = n, rng_mode, 1, seed0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return _lib.Handle(cfg)


def policy_kwargs(h, hidden, seed, normalize, freeze, sample):
    """the keyword arguments of Handle.rollout_policy_summary for a random per-env policy; hidden == 0: the linear one"""
    rs = np.random.RandomState(seed)
    kw = dict(per_env=True, freeze_after_done=bool(freeze), sample=bool(sample))
    if hidden:
        kw.update(params=(0.5 * rs.standard_normal((h.num_envs, h.mlp_param_count(hidden)))).astype(np.float32), hidden=hidden)
    else:
        kw.update(weights=rs.standard_normal(h.policy_shape(True)))
    if normalize:
        kw.update(obs_mean=rs.uniform(-0.3, 0.3, h.obs_dim), obs_std=rs.uniform(0.5, 2.0, h.obs_dim), clip_obs=1.5)
    return kw


def plane_call(h, T, kw):
    kw = dict(kw)
    if "params" in kw:
        return h.rollout_mlp_policy(T, kw.pop("params"), kw.pop("hidden"), **kw)
    return h.rollout_policy(T, kw.pop("weights"), **kw)


def check_against_twin(hs, T, kw, fields, calls=1):
    """hs = (summary handle, twin), both freshly made with the same seed.  `calls` summary calls against as many plane calls; the
    last pair is compared.  Returns the reference of the last call."""
    a, b = hs
    assert np.array_equal(a.reset(), b.reset())
    for _ in range(calls):
        out = a.rollout_policy_summary(T, **kw)
        planes = plane_call(b, T, kw)
    want = ref.summary_from_planes(planes["obs"], planes["reward"], planes["done"])
    for k in KEYS:
        assert ref.bits_equal(out[k], want[k]), (k, out[k][:4], want[k][:4])
    after_a, after_b = plane_call(a, 3, kw), plane_call(b, 3, kw)
    for k in after_a:
        assert ref.bits_equal(after_a[k], after_b[k]), "one further call: " + k
    for f in fields:
        assert ref.bits_equal(a.get_state(getattr(_lib, f)), b.get_state(getattr(_lib, f))), f
    return want


def mobile_cases():
    cases = []
    i = 0
    for kind in (0, 1, 2, 3):
        for disc in (1, 0):
            if not disc and kind in (1, 2):              # no continuous policy kernel for the 1D and two-target envs
                continue
            for hidden in (0, 5, 100):
                for sample in ((0, 1) if disc else (0,)):
                    # every kernel (kind, action type, policy family, selection) meets both RNG modes at both lengths; normalize and
                    # freeze change once per kernel, out of step with each other, so each RNG x T pair of a policy family sees both values
                    for rng in ("PHILOX", "MT19937"):
                        for T in (300, 40):
                            cases.append((kind, disc, rng, hidden, sample, i % 2, (i // 2 + (rng == "MT19937")) % 2, T))
                    i += 1
    return cases


MOBILE_CASES = mobile_cases()


@pytest.mark.parametrize("kind,disc,rng,hidden,sample,normalize,freeze,T", MOBILE_CASES,
                         ids=["k{}-d{}-{}-h{}-s{}-n{}-f{}-T{}".format(*c) for c in MOBILE_CASES])
def test_mobile_summary_equals_the_reference_on_the_twins_planes(kind, disc, rng, hidden, sample, normalize, freeze, T):
    n = 130
    hs = [make(kind, n, RNG[rng], seed0=11, is_discrete=disc, random_target=1) for _ in range(2)]
    kw = policy_kwargs(hs[0], hidden, 100 + kind, normalize, freeze, sample)
    want = check_against_twin(hs, T, kw, MOBILE_FIELDS)
    if T == 300:
        assert (want["first"] < T).all(), "every env passes its 251-step limit"
    else:
        assert (want["first"] == T).sum() > n // 2, "most envs report no done in 40 steps"
        assert (want["length"][want["first"] == T] == T).all()
    for h in hs:
        h.close()


KUKA_CASES = []
for _env, _disc, _joints, _forms in (("KUKA_BUTTON", 1, 0, ((0, 0), (100, 0), (0, 1), (100, 1))), ("KUKA_BUTTON", 0, 0, ((0, 0), (100, 0))),
                                     ("KUKA_BUTTON", 0, 1, ((0, 0), (100, 0))), ("KUKA_2BUTTON", 1, 0, ((0, 0), (100, 0), (0, 1), (100, 1)))):
    for _hidden, _sample in _forms:
        for _rng in ("PHILOX", "MT19937"):              # every instantiation meets both RNG modes at every length
            for _T in (1010, 64) + ((1510,) if _env == "KUKA_2BUTTON" else ()):
                _i = len(KUKA_CASES)
                KUKA_CASES.append((_env, _disc, _joints, _rng, _hidden, _sample, (_i // 2) % 2, (_i // 3) % 2, _T))


@pytest.mark.parametrize("env,disc,joints,rng,hidden,sample,normalize,freeze,T", KUKA_CASES,
                         ids=["{}-d{}-j{}-{}-h{}-s{}-n{}-f{}-T{}".format(*c) for c in KUKA_CASES])
def test_kuka_summary_equals_the_reference_on_the_twins_planes(env, disc, joints, rng, hidden, sample, normalize, freeze, T):
    n = 7
    hs = [make(getattr(_lib, "ENV_" + env), n, RNG[rng], seed0=3, is_discrete=disc, action_joints=joints) for _ in range(2)]
    kw = policy_kwargs(hs[0], hidden, 40 + disc + 2 * joints, normalize, freeze, sample)
    want = check_against_twin(hs, T, kw, KUKA_FIELDS)
    limit = 1501 if env == "KUKA_2BUTTON" else 1001
    if T >= limit:
        assert (want["first"] < T).all(), "the step limit guarantees a done in every env"
    elif T == 64:
        assert (want["first"] == T).any(), "at least one env has no done"
    for h in hs:
        h.close()


def test_two_calls_in_a_row_are_two_plane_calls_and_the_second_summary_is_the_second_calls_alone():
    for kind, T in ((0, 150), (_lib.ENV_KUKA_BUTTON, 40)):
        mobile = kind == 0
        hs = [make(kind, 130 if mobile else 7, _lib.RNG_PHILOX, seed0=5) for _ in range(2)]
        kw = policy_kwargs(hs[0], 0, 9, 0, 0, 0)
        want = check_against_twin(hs, T, kw, MOBILE_FIELDS if mobile else KUKA_FIELDS, calls=2)
        if mobile:
            assert (want["first"] < T).all() and (want["first"] > 50).all()      # the second call meets the 251st step of the episode
        for h in hs:
            h.close()


def test_device_surface_graph_replay_wrappers_and_normalize_statistics():
    import torch
    from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize, first_done_masks
    n, seed, T = 130, 9, 300
    env = DeviceVecEnv("MobileRobotGymEnv-v0", n, seed=seed, rng_mode="philox")
    mirror = make(0, n, _lib.RNG_PHILOX, seed0=seed)
    W = np.random.RandomState(77).standard_normal(env.h.policy_shape(True))
    Wd = torch.as_tensor(W, device=env.device)

    def same(out, want, tag):
        for k in KEYS:
            assert ref.bits_equal(out[k].cpu().numpy(), want[k]), tag + " " + k

    with torch.cuda.stream(env.torch_stream):
        env.reset()
        out = env.rollout_policy_summary(T, Wd, freeze_after_done=True)
    env.torch_stream.synchronize()
    mirror.reset()
    direct = mirror.rollout_policy_summary(T, weights=W, freeze_after_done=True)
    same(out, direct, "on stream")
    # graph capture of one call on the device-pointer handle: the replay gives the bits of a direct call
    bufs = {"ret": torch.zeros(n, dtype=torch.float64, device=env.device), "length": torch.zeros(n, dtype=torch.int32, device=env.device),
            "obs_sum": torch.zeros((n, 2), dtype=torch.float64, device=env.device), "obs_sqsum": torch.zeros((n, 2), dtype=torch.float64, device=env.device)}
    env.reset(); mirror.reset()
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_policy_summary(T, weights=Wd.data_ptr(), freeze_after_done=True, out=tuple(bufs[k].data_ptr() for k in KEYS))
    g = h.graph_end()
    h.graph_launch(g)
    h.sync()
    same(bufs, mirror.rollout_policy_summary(T, weights=W, freeze_after_done=True), "graph")
    h.graph_destroy(g)
    # the MLP form, the trivial frame stack; a real stack refuses
    P = (0.5 * np.random.RandomState(3).standard_normal((n, env.h.mlp_param_count(5)))).astype(np.float32)
    env.reset(); mirror.reset()
    same(DeviceVecFrameStack(env, 1).rollout_mlp_policy_summary(40, torch.as_tensor(P, device=env.device), 5),
         mirror.rollout_policy_summary(40, params=P, hidden=5), "stack of 1, MLP")
    for name, args in (("rollout_policy_summary", (4, Wd)), ("rollout_mlp_policy_summary", (4, torch.as_tensor(P, device=env.device), 5))):
        with pytest.raises(NotImplementedError):
            getattr(DeviceVecFrameStack(env, 4), name)(*args)
    # DeviceVecNormalize, training: one update from the sums against a twin updated through the planes path
    twins = [DeviceVecEnv("MobileRobotGymEnv-v0", n, seed=seed, rng_mode="philox") for _ in range(2)]      # fresh: the same episode twice
    norms = [DeviceVecNormalize(e, training=True, norm_reward=False) for e in twins]
    for e in twins:
        e.reset()
    s = norms[0].rollout_policy_summary(T, Wd, freeze_after_done=True)
    planes = norms[1].rollout_policy(T, Wd, freeze_after_done=True)
    want = ref.summary_from_planes(planes["obs"].cpu().numpy(), planes["reward"].cpu().numpy(), planes["done"].cpu().numpy())
    same(s, want, "normalised")
    a, b = norms[0].obs_rms, norms[1].obs_rms
    live = (~first_done_masks(planes["done"])[1]).cpu().numpy()
    x = planes["obs"].cpu().numpy().astype(np.float64)[live]              # [rows][D]
    rows = x.shape[0]
    assert float(a.count) == float(b.count) == 1e-4 + rows
    mean_a, mean_b, var_a, var_b = (t.cpu().numpy() for t in (a.mean, b.mean, a.var, b.var))
    mean_err, var_err = np.abs(mean_a - mean_b), np.abs(var_a - var_b)
    mean_bound, var_bound = rows * 2.0 ** -52 * np.abs(x).max(0), 4 * rows * 2.0 ** -52 * (x * x).mean(0)
    print("obs_rms after one summary update vs the planes path: |mean diff| {} (bound {}), |var diff| {} (bound {})".format(mean_err, mean_bound, var_err, var_bound))
    assert (mean_err <= mean_bound).all() and (var_err <= var_bound).all()
    env.close(); mirror.close()
    for e in twins:
        e.close()


def test_kuka_device_pointer_handle_direct_and_under_graph_capture():
    """KukaButton on a device-pointer handle (the header kernel writes the four output pointers into the policy header): the tensor
    surface with the linear policy, then a captured and replayed call with the sampled MLP, against a host-pointer mirror."""
    import torch
    from srlhip.device_env import DeviceVecEnv
    n, seed, T, H = 7, 4, 64, 5
    env = DeviceVecEnv("KukaButtonGymEnv-v0", n, seed=seed, rng_mode="philox")
    mirror = make(_lib.ENV_KUKA_BUTTON, n, _lib.RNG_PHILOX, seed0=seed)
    rs = np.random.RandomState(21)
    W = rs.standard_normal(env.h.policy_shape(True))
    P = (0.5 * rs.standard_normal((n, env.h.mlp_param_count(H)))).astype(np.float32)
    Wd, Pd = torch.as_tensor(W, device=env.device), torch.as_tensor(P, device=env.device)
    with torch.cuda.stream(env.torch_stream):
        env.reset()
        out = env.rollout_policy_summary(T, Wd, freeze_after_done=True)
    env.torch_stream.synchronize()
    mirror.reset()
    want = mirror.rollout_policy_summary(T, weights=W, freeze_after_done=True)
    for k in KEYS:
        assert ref.bits_equal(out[k].cpu().numpy(), want[k]), "direct " + k
    bufs = {"ret": torch.zeros(n, dtype=torch.float64, device=env.device), "length": torch.zeros(n, dtype=torch.int32, device=env.device),
            "obs_sum": torch.zeros((n, 3), dtype=torch.float64, device=env.device), "obs_sqsum": torch.zeros((n, 3), dtype=torch.float64, device=env.device)}
    torch.cuda.synchronize()
    h = env.h
    h.graph_begin()
    h.rollout_policy_summary(T, params=Pd.data_ptr(), hidden=H, sample=True, out=tuple(bufs[k].data_ptr() for k in KEYS))
    g = h.graph_end()
    h.graph_launch(g)
    h.sync()
    want = mirror.rollout_policy_summary(T, params=P, hidden=H, sample=True)      # continues from the state the first call left
    for k in KEYS:
        assert ref.bits_equal(bufs[k].cpu().numpy(), want[k]), "graph " + k
    h.graph_destroy(g)
    env.close(); mirror.close()


def _lin(W, **kw):
    p = _lib.LinearPolicy()
    p.struct_size, p.per_env, p.weights, p.clip_obs = ctypes.sizeof(_lib.LinearPolicy), 1, W.ctypes.data, 10.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _mlp(W, hidden, **kw):
    p = _lib.MlpPolicy()
    p.struct_size, p.per_env, p.hidden, p.params, p.clip_obs = ctypes.sizeof(_lib.MlpPolicy), 1, hidden, W.ctypes.data, 10.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class _Out(object):
    def __init__(self, n, D):
        self.arrays = {"ret": np.zeros(n), "length": np.zeros(n, np.int32), "obs_sum": np.zeros((n, D)), "obs_sqsum": np.zeros((n, D))}

    def struct(self, **kw):
        s = _lib.RolloutSummary()
        s.struct_size, s.reserved = ctypes.sizeof(_lib.RolloutSummary), 0
        for k, a in self.arrays.items():
            setattr(s, k, a.ctypes.data)
        for k, v in kw.items():
            setattr(s, k, v)
        return s


def _call(h, T, lin, mlp, sample, out):
    return h._lib.srlhip_rollout_policy_summary(h._h, T, None if lin is None else ctypes.byref(lin), None if mlp is None else ctypes.byref(mlp), sample,
                                                None if out is None else ctypes.byref(out))


REFUSALS = [           # test_gpu_policy_rollout.py's table, restated for this entry
    ("joints", _lib.ENV_KUKA_BUTTON, dict(obs_mode=_lib.OBS_JOINTS), "joints"),
    ("joints_position", _lib.ENV_KUKA_BUTTON, dict(obs_mode=_lib.OBS_JOINTS_POSITION), "joints_position"),
    ("raw_pixels", _lib.ENV_MOBILE, dict(obs_mode=_lib.OBS_RAW_PIXELS, img_h=16, img_w=16), "raw_pixels"),
    ("rand_button", _lib.ENV_KUKA_RAND, dict(), "KukaRandButton"),
    ("lumped", _lib.ENV_KUKA_BUTTON, dict(kuka_model=_lib.KUKA_MODEL_LUMPED), "lumped"),
    ("rng_host", _lib.ENV_MOBILE, dict(rng_mode=_lib.RNG_HOST, auto_reset=0), "RNG_HOST"),
    ("no_auto_reset", _lib.ENV_MOBILE, dict(auto_reset=0), "auto_reset"),
]


@pytest.mark.parametrize("name,kind,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_what_they_refuse_and_leave_the_handle_usable(name, kind, kw, word):
    n = 5
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.rng_mode, cfg.seed0 = n, _lib.RNG_PHILOX, 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = _lib.Handle(cfg)
    host_rand = np.full((n, h.reset_rand_count), 0.5) if cfg.rng_mode == _lib.RNG_HOST else None
    before = h.reset(host_rand=host_rand)
    W = np.zeros((n, 32, 8))                          # larger than any policy shape: never read
    out = _Out(n, 32)
    assert _call(h, 4, _lin(W), None, 0, out.struct()) == -95
    assert word in h.last_error(), h.last_error()
    assert h.last_error().startswith("rollout_policy_summary:"), h.last_error()
    again = h.reset(host_rand=host_rand)              # the refusal left the handle usable
    assert again.shape == before.shape
    if cfg.rng_mode != _lib.RNG_HOST:
        o, r, d = h.step(np.zeros(n, np.int32))
        assert d.shape == (n,) and np.isfinite(r).all()
    h.close()


def test_sample_is_discrete_only_and_kuka2button_has_no_joint_space_mlp():
    n = 5
    for kind, kw, lin, word in ((_lib.ENV_MOBILE, dict(is_discrete=0), True, "discrete"), (_lib.ENV_KUKA_BUTTON, dict(is_discrete=0), True, "discrete"),
                                (_lib.ENV_KUKA_BUTTON, dict(is_discrete=0), False, "discrete"), (_lib.ENV_KUKA_2BUTTON, dict(is_discrete=0, action_joints=1), False, "Kuka2Button")):
        h = make(kind, n, _lib.RNG_PHILOX, seed0=2, **kw)
        before = h.reset()
        W64, W32, out = np.zeros((n, 32, 8)), np.zeros((n, 4096), np.float32), _Out(n, 3)
        sample = 0 if word == "Kuka2Button" else 1
        assert _call(h, 4, _lin(W64) if lin else None, None if lin else _mlp(W32, 100), sample, out.struct()) == -95, h.last_error()
        assert word in h.last_error() and h.last_error().startswith("rollout_policy_summary:"), h.last_error()
        assert h.reset().shape == before.shape
        h.close()


def test_einval_cases_leave_the_handle_as_it_was():
    n = 7
    h = make(0, n, _lib.RNG_PHILOX, seed0=1)
    h.reset()
    W = np.random.RandomState(2).standard_normal(h.policy_shape(True))
    P = np.zeros((n, h.mlp_param_count(5)), np.float32)
    out = _Out(n, 2)
    ok = np.array([0.1, 0.2]), np.array([1.0, 2.0])
    bad_calls = [
        ("both policies", (4, _lin(W), _mlp(P, 5), 0, out.struct()), "exactly one"),
        ("neither policy", (4, None, None, 0, out.struct()), "exactly one"),
        ("null out", (4, _lin(W), None, 0, None), "out"),
        ("null ret", (4, _lin(W), None, 0, out.struct(ret=None)), "ret"),
        ("obs_sum alone", (4, _lin(W), None, 0, out.struct(obs_sqsum=None)), "obs_sqsum"),
        ("obs_sqsum alone", (4, _lin(W), None, 0, out.struct(obs_sum=None)), "obs_sum"),
        ("struct_size", (4, _lin(W), None, 0, out.struct(struct_size=32)), "struct_size"),
        ("reserved", (4, _lin(W), None, 0, out.struct(reserved=1)), "reserved"),
        ("policy struct_size", (4, _lin(W, struct_size=8), None, 0, out.struct()), "struct_size"),
        ("mlp reserved", (4, None, _mlp(P, 5, reserved=1), 0, out.struct()), "reserved"),
        ("hidden", (4, None, _mlp(P, 129), 0, out.struct()), "hidden"),
        ("T", (0, _lin(W), None, 0, out.struct()), "T"),
        ("null weights", (4, _lin(W, weights=None), None, 0, out.struct()), "weights"),
        ("mean without std", (4, _lin(W, normalize=1, obs_mean=ok[0].ctypes.data), None, 0, out.struct()), "obs_mean"),
    ]
    for tag, args, word in bad_calls:
        assert _call(h, *args) == -22, tag
        assert word in h.last_error() and h.last_error().startswith("rollout_policy_summary:"), (tag, h.last_error())
    # the value checks of the plane calls on a host-pointer handle
    for bad in (np.array([1.0, 0.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])):
        assert _call(h, 4, _lin(W, normalize=1, obs_mean=ok[0].ctypes.data, obs_std=bad.ctypes.data), None, 0, out.struct()) == -22, bad
        assert "obs_std" in h.last_error()
    Wb = W.copy(); Wb[3, 1, 2] = np.nan
    assert _call(h, 4, _lin(Wb), None, 0, out.struct()) == -22 and "weights" in h.last_error()
    Pb = P.copy(); Pb[2, 3] = np.inf
    assert _call(h, 4, None, _mlp(Pb, 5), 0, out.struct()) == -22 and "params" in h.last_error()
    # a pending step
    h.step_async(np.zeros(n, np.int32))
    assert _call(h, 4, _lin(W), None, 0, out.struct()) == -22 and "pending" in h.last_error()
    h.step_wait()
    # length and the moments are optional; the handle equals one that saw none of the above
    g = make(0, n, _lib.RNG_PHILOX, seed0=1)
    g.reset(); g.step(np.zeros(n, np.int32))
    assert _call(h, 300, _lin(W), None, 0, out.struct(length=None, obs_sum=None, obs_sqsum=None)) == 0, h.last_error()
    want = g.rollout_policy_summary(300, weights=W, moments=False)
    assert ref.bits_equal(out.arrays["ret"], want["ret"]) and not out.arrays["length"].any() and not out.arrays["obs_sum"].any()
    assert "obs_sum" not in want
    h.close(); g.close()


def test_a_resident_persistent_kernel_parks_around_the_call():
    n = 64
    hs = [make(0, n, _lib.RNG_PHILOX, seed0=6, random_target=1) for _ in range(2)]
    W = np.random.RandomState(11).standard_normal(hs[0].policy_shape(True))
    acts = np.random.RandomState(3).randint(4, size=(6, n)).astype(np.int32)
    hs[0].set_persistent(True)
    res = []
    for h in hs:
        r = [h.reset()]
        r += [np.concatenate([np.ravel(x) for x in h.step(acts[t])]) for t in range(3)]
        s = h.rollout_policy_summary(40, weights=W)
        r += [s[k] for k in KEYS]
        r += [np.concatenate([np.ravel(x) for x in h.step(acts[t])]) for t in range(3, 6)]
        res.append(r)
    for x, y in zip(*res):
        assert ref.bits_equal(x, y)
    for h in hs:
        h.close()


# ---- the learners ---------------------------------------------------------------------------------------------------------------------
def _ars_args(returns, algo_type="v1", num_timesteps=20000, seed=5):
    import argparse
    P = 8
    return argparse.Namespace(env="MobileRobotGymEnv-v0", num_population=P, top_population=2, step_size=0.02, exploration_noise=0.02,
                              algo_type=algo_type, max_step_amplitude=10, deterministic=True, continuous_actions=False, fused_rollout=True,
                              fused_returns=returns, num_timesteps=num_timesteps, seed=seed, srl_model="ground_truth", num_stack=1, num_cpu=2 * P,
                              log_dir=None)


def test_ars_v1_fused_returns_equals_fused_rollout_bit_for_bit():
    """--algo-type v1 (no normalisation), unshaped rewards, three updates (P x 251 live rows = 2008 steps each against num_updates = 20000 // P * 2 = 5000)."""
    from rl_baselines.evolution_strategies.ars import ARSModel
    planes, summary = ARSModel().train(_ars_args(False)), ARSModel().train(_ars_args(True))
    assert len(planes.history) == 3 and np.abs(planes.M).max() > 0
    assert ref.bits_equal(summary.M, planes.M) and summary.history == planes.history


def test_ars_v2_fused_returns_agrees_over_one_update():
    """With v2's normalisation the statistics come from the launch's sums (sum / n, sqsum / n - mean^2) instead of the two-pass
    variance of the planes: one update — its evaluation runs on the INITIAL statistics in both paths, so the returns are the same
    numbers, and the history agrees to 1e-9 relative."""
    from rl_baselines.evolution_strategies.ars import ARSModel
    planes, summary = ARSModel().train(_ars_args(False, "v2", 2008)), ARSModel().train(_ars_args(True, "v2", 2008))
    assert len(planes.history) == 1 and len(summary.history) == 1
    a, b = np.asarray(summary.history, np.float64), np.asarray(planes.history, np.float64)
    assert np.isfinite(a).all() and np.isfinite(summary.M).all()
    assert np.all(np.abs(a - b) <= 1e-9 * np.abs(b)), (a, b)


def test_cma_es_fused_returns_equals_fused_rollout_over_three_generations():
    """CMA-ES always wraps its env in DeviceVecNormalize; "the same setting" as ARS v1 is that wrapper with its statistics frozen
    (training = False), so that both paths hand the kernel the same numbers: equal best member, history and step count."""
    import argparse
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    P = 16

    class Frozen(CMAESModel):
        calls, steps = 0, 0

        @classmethod
        def makeEnv(cls, args, env_kwargs=None, load_path_normalise=None):
            env = super(Frozen, cls).makeEnv(args, env_kwargs, load_path_normalise)
            env.training = False
            return env

        def evaluate_fused(self, env_, population, T_):
            r, live = CMAESModel.evaluate_fused(self, env_, population, T_)
            self.calls += 1
            self.steps += int(live.sum())
            return r, live + (10 ** 9 if self.calls == 3 else 0)       # the third generation ends the run

    def run(returns):
        a = argparse.Namespace(env="MobileRobotGymEnv-v0", num_population=P, mu=0.0, sigma=0.14, deterministic=True, continuous_actions=False,
                               fused_rollout=True, fused_returns=returns, num_timesteps=10 ** 8, seed=5, srl_model="ground_truth", num_stack=1, log_dir=None)
        return Frozen().train(a)

    planes, summary = run(False), run(True)
    assert planes.calls == 3 and summary.calls == 3 and summary.steps == planes.steps and planes.steps >= 3 * P
    assert ref.bits_equal(np.asarray(summary.best_model), np.asarray(planes.best_model))
    assert np.array_equal(np.asarray(summary.history), np.asarray(planes.history))
