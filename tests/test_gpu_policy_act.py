"""srlhip_policy_act on the GPU: the kernels of csrc/policy_act.hip against the order-exact numpy restatement of the contract
(tests/policy_act_ref.py) bit for bit, the call's bookkeeping (frozen plane, action-stream counters, graph replay), and the closed loop
policy_act -> step against the three fused rollouts from the same seed."""

import numpy as np
import pytest

import mlp_policy_ref as ref
import mlp_sample_ref as msr
import policy_act_ref as par
import policy_exact as pe

pytestmark = pytest.mark.gpu

DS, HS = (1, 3, 17, 200), (1, 16, 17, 100, 128)
# handle kinds by the action space they give: A = 2, 4, 6 discrete; 2, 3, 7 continuous
SPACES = {("d", 2): ("ENV_MOBILE_1D", 1, 0), ("d", 4): ("ENV_MOBILE", 1, 0), ("d", 6): ("ENV_KUKA_BUTTON", 1, 0),
          ("c", 2): ("ENV_MOBILE", 0, 0), ("c", 3): ("ENV_KUKA_BUTTON", 0, 0), ("c", 7): ("ENV_KUKA_BUTTON", 0, 1)}


def torch_():
    import torch
    return torch


def make_handle(space, n, rng="PHILOX", seed=17, obs_mode=None, io_device=1):
    from srlhip import _lib
    kind, discrete, joints = SPACES[space]
    cfg = _lib.default_config(getattr(_lib, kind))
    cfg.num_envs, cfg.seed0, cfg.is_discrete, cfg.action_joints = n, seed, discrete, joints
    cfg.rng_mode, cfg.auto_reset, cfg.io_device = getattr(_lib, "RNG_" + rng), 1, io_device
    if obs_mode is not None:
        cfg.obs_mode, cfg.img_h, cfg.img_w = obs_mode, 64, 64
    return _lib.Handle(cfg)


def dev(a):
    torch = torch_()
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Call(object):
    """one srlhip_policy_act call on device copies of numpy inputs -> numpy outputs"""

    def __init__(self, h, space, D):
        self.h, self.discrete, self.D = h, space[0] == "d", D
        self.A, self.none_nan = space[1], SPACES[space][0].startswith("ENV_KUKA")

    def __call__(self, obs, params, hidden=0, per_env=True, mean=None, std=None, clip=10.0, freeze=False, done_prev=None, frozen=None,
                 sample=False, rows=None):
        torch = torch_()
        n, A = self.h.num_envs, self.A
        keep = [dev(obs.astype(np.float32)), dev(params.astype(np.float32) if hidden else params.astype(np.float64))]
        act = torch.full((n,) if self.discrete else (n, A), -7, dtype=torch.int32 if self.discrete else torch.float32, device="cuda")
        score = torch.zeros((n, A), dtype=torch.float64, device="cuda")
        kw = dict(per_env=per_env, freeze_after_done=freeze, clip_obs=clip, sample=sample, score_out=score.data_ptr())
        if mean is not None:
            keep += [dev(mean.astype(np.float64)), dev(std.astype(np.float64))]
            kw.update(obs_mean=keep[-2].data_ptr(), obs_std=keep[-1].data_ptr())
        fz = None
        if frozen is not None:
            fz = dev(frozen.astype(np.uint8))
            kw["frozen"] = fz.data_ptr()
        if done_prev is not None:
            keep.append(dev(done_prev.astype(np.uint8)))
            kw["done_prev"] = keep[-1].data_ptr()
        kw.update(dict(params=keep[1].data_ptr(), hidden=hidden) if hidden else dict(weights=keep[1].data_ptr()))
        self.h.policy_act(keep[0].data_ptr(), self.D, act.data_ptr(), **kw)
        self.h.sync()
        return dict(action=act.cpu().numpy(), score=score.cpu().numpy(), frozen=None if fz is None else fz.cpu().numpy())


def gaussian(seed, N, D, H, A, per_env):
    rng = np.random.RandomState(seed)
    obs = rng.standard_normal((N, D)).astype(np.float32)
    obs[rng.random_sample((N, D)) < 0.1] = np.float32(-0.0)
    lead = (N,) if per_env else ()
    params = ref.random_params(seed + 1, lead + (ref.param_count(D, H, A),)) if H else 0.5 * rng.standard_normal(lead + (D, A))
    if H:
        ref.split(params, D, H, A)[3][..., 0] = -0.0
    if per_env and N > 1:
        params[1] = -0.0 if not H else 0.0
    return obs, params, 0.1 * rng.standard_normal(D), 0.5 + rng.random_sample(D), 1.25


@pytest.mark.parametrize("N", [1, 5, 67, 130])
@pytest.mark.parametrize("space", sorted(SPACES))
def test_kernel_equals_the_reference(space, N):
    h = make_handle(space, N)
    discrete, A = space[0] == "d", space[1]
    try:
        for D in DS:
            call = Call(h, space, D)
            for H in (0,) + HS:
                for per_env in (1, 0):
                    obs, params, mean, std, clip = gaussian(N * 1000 + D * 7 + H, N, D, H, A, per_env)
                    rng = np.random.RandomState(D + H)
                    done_prev, frozen = rng.randint(0, 4, size=N).astype(np.uint8), (rng.random_sample(N) < 0.3).astype(np.uint8)
                    got = call(obs, params, H, per_env, mean, std, clip, True, done_prev, frozen)
                    kw = dict(params=params, hidden=H) if H else dict(weights=params)
                    want = par.act(obs, D, A, discrete, per_env=per_env, mean=mean, std=std, clip=clip, freeze=True, done_prev=done_prev,
                                   frozen=frozen, none_nan=call.none_nan, **kw)
                    where = (space, N, D, H, per_env)
                    assert np.array_equal(pe.bits(got["score"]), pe.bits(want["score"])), where
                    assert np.array_equal(pe.bits(got["action"]), pe.bits(want["action"])), where
                    assert np.array_equal(got["frozen"], want["frozen"]), where
    finally:
        h.close()


@pytest.mark.parametrize("rng", ["PHILOX", "MT19937"])
@pytest.mark.parametrize("space", [("d", 4), ("d", 6)])
def test_sampled_scores_bitwise_actions_by_the_interval_rule_and_counters(space, rng):
    """sampled calls: scores bit-equal, the action equal or inside the interval rule (share capped), the draws those of blocks
    c0, c0 + 1, ... of every env's stream — frozen envs included — on both rng modes"""
    N, D, H, A, K = 67, 17, 17, space[1], 4
    h = make_handle(space, N, rng=rng)
    try:
        call = Call(h, space, D)
        obs, params, mean, std, clip = gaussian(5, N, D, H, A, 1)
        frozen = (np.arange(N) % 5 == 0).astype(np.uint8)
        seeds = 17 + np.arange(N)
        u = msr.draws(seeds, 0, K)                             # the counters start at 0 after create
        needed = live_total = 0
        for k in range(K):
            got = call(obs, params, H, 1, mean, std, clip, True, None, frozen, sample=True)
            want = par.act(obs, D, A, True, params=params, hidden=H, mean=mean, std=std, clip=clip, freeze=True, frozen=frozen, u=u[k])
            assert np.array_equal(pe.bits(got["score"]), pe.bits(want["score"]))
            live = want["live"]
            assert (got["action"][~live] == -1).all()
            differ = live & (got["action"] != want["action"])
            assert par.interval_ok(want["score"], u[k], got["action"])[live].all()
            needed, live_total = needed + int(differ.sum()), live_total + int(live.sum())
        print("sampled {} {}: {} of {} live actions needed the interval rule".format(space, rng, needed, live_total))
        assert needed <= pe.MAX_SHARE * live_total
        # the synthetic agent continues on the same counters: after K sampled calls its draws are those of a twin handle that has drawn
        # as many as the header says K blocks are (MobileRobot discrete: the counter counts actions; Kuka discrete: blocks)
        torch = torch_()
        twin = make_handle(space, N, rng=rng)
        planes = [torch.zeros((1, N), dtype=torch.int32, device="cuda") for _ in range(2)]
        warm = torch.zeros((K, N), dtype=torch.int32, device="cuda")
        scratch = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
        for hh in (h, twin):
            hh.reset(obs_out=scratch.data_ptr())
        twin.rollout(K, out=(None, None, None, warm.data_ptr()))
        for hh, p in ((h, planes[0]), (twin, planes[1])):
            hh.rollout(1, out=(None, None, None, p.data_ptr()))
            hh.sync()
        assert np.array_equal(planes[0].cpu().numpy(), planes[1].cpu().numpy())
        twin.close()
    finally:
        h.close()


def test_captured_call_replayed_equals_eager_calls():
    space, N, D, H, A, K = ("d", 4), 67, 17, 16, 4, 3
    torch = torch_()
    obs, params, mean, std, clip = gaussian(11, N, D, H, A, 1)
    d_obs, d_par = dev(obs), dev(params)
    rows = {}
    for mode in ("eager", "graph"):
        h = make_handle(space, N)
        act = torch.zeros((N,), dtype=torch.int32, device="cuda")
        kw = dict(params=d_par.data_ptr(), hidden=H, sample=True)
        got = []
        if mode == "eager":
            for _ in range(K + 1):
                h.policy_act(d_obs.data_ptr(), D, act.data_ptr(), **kw)
                h.sync()
                got.append(act.cpu().numpy().copy())
        else:
            h.policy_act(d_obs.data_ptr(), D, act.data_ptr(), **kw)          # eager first, as every captured sequence
            h.sync()
            got.append(act.cpu().numpy().copy())
            h.graph_begin()
            h.policy_act(d_obs.data_ptr(), D, act.data_ptr(), **kw)
            g = h.graph_end()
            for _ in range(K):
                h.graph_launch(g)
                h.sync()
                got.append(act.cpu().numpy().copy())
            h.graph_destroy(g)
        rows[mode] = np.stack(got)
        h.close()
    assert np.array_equal(rows["eager"], rows["graph"])
    assert (rows["eager"][1:] != rows["eager"][:-1]).any()        # fresh numbers at every call


def test_result_does_not_depend_on_the_batch_around_an_env():
    space, D, H, A = ("d", 6), 17, 100, 6
    obs, params, mean, std, clip = gaussian(21, 67, D, H, A, 1)
    obs[1], params[1] = obs[2], params[3]                         # (gaussian's zero block: make row 1 ordinary)
    base = None
    for N, at in ((1, 0), (5, 0), (67, 0), (67, 40), (5, 3)):
        h = make_handle(space, N)
        o, p = np.roll(obs, at, 0)[:N], np.roll(params, at, 0)[:N]      # rows 0 and 1 of the originals sit at `at`, `at + 1`
        got = Call(h, space, D)(o, p, H, 1, mean, std, clip)
        h.close()
        row = (pe.bits(got["score"][at]).tolist(), int(got["action"][at]))
        base = base or row
        assert row == base, (N, at)
    lin = 0.5 * np.random.RandomState(3).standard_normal((67, D, A))
    base = None
    for N, at in ((1, 0), (5, 0), (67, 0), (67, 40)):
        h = make_handle(space, N)
        got = Call(h, space, D)(np.roll(obs, at, 0)[:N], np.roll(lin, at, 0)[:N], 0, 1, mean, std, clip)
        h.close()
        row = (pe.bits(got["score"][at]).tolist(), int(got["action"][at]))
        base = base or row
        assert row == base, (N, at)


@pytest.mark.parametrize("space", [("d", 4), ("c", 2), ("c", 3)])
def test_done_prev_and_frozen_semantics(space):
    N, D, H, A = 5, 3, 16, space[1]
    h = make_handle(space, N)
    try:
        call = Call(h, space, D)
        obs, params, mean, std, clip = gaussian(31, N, D, H, A, 1)
        params[1] = params[2]                                   # (gaussian's all-zero block would score a zero row: not a `None`)
        done_prev, frozen = np.array([0, 1, 2, 3, 0], np.uint8), np.array([0, 0, 0, 0, 1], np.uint8)

        def none(a):
            if space[0] == "d":
                return a == -1
            return np.isnan(a).all(-1) if call.none_nan else ((a == 0).all(-1) & ~np.signbit(a).any(-1))
        got = call(obs, params, H, 1, freeze=True, done_prev=done_prev, frozen=frozen)
        assert got["frozen"].tolist() == [0, 1, 0, 1, 1] and none(got["action"]).tolist() == [False, True, False, True, True]
        if space == ("c", 3):
            assert (pe.bits(got["action"][1]) == 0x7fc00000).all()
        again = call(obs, params, H, 1, freeze=True, done_prev=np.zeros(N, np.uint8), frozen=got["frozen"])      # a frozen env stays frozen
        assert again["frozen"].tolist() == [0, 1, 0, 1, 1] and none(again["action"]).tolist() == [False, True, False, True, True]
        first = call(obs, params, H, 1, freeze=True, done_prev=None, frozen=frozen)                                # NULL done_prev
        assert first["frozen"].tolist() == [0, 0, 0, 0, 1] and none(first["action"]).tolist() == [False] * 4 + [True]
        off = call(obs, params, H, 1, freeze=False, done_prev=done_prev, frozen=frozen)                            # ignores both planes
        assert off["frozen"].tolist() == frozen.tolist() and not none(off["action"]).any()
    finally:
        h.close()


# ---- closed loop against the fused kernels -----------------------------------------------------------------------------------------------
def closed_loop(space, rng, N, T, params, hidden, norm, sample=False):
    """-> (planes of one fused call, planes of T x (policy_act -> step)) from the same seed"""
    torch = torch_()
    D = 2 if SPACES[space][0] == "ENV_MOBILE" else (1 if SPACES[space][0] == "ENV_MOBILE_1D" else 3)
    A, discrete = space[1], space[0] == "d"
    mean, std, clip = norm
    d_par = dev(params.astype(np.float32) if hidden else params.astype(np.float64))
    d_mean, d_std = (None, None) if mean is None else (dev(mean), dev(std))
    stats = dict(obs_mean=None if mean is None else d_mean.data_ptr(), obs_std=None if mean is None else d_std.data_ptr(), clip_obs=clip)

    def planes():
        return {"obs": torch.zeros((T, N, D), dtype=torch.float32, device="cuda"), "reward": torch.zeros((T, N), dtype=torch.float32, device="cuda"),
                "done": torch.zeros((T, N), dtype=torch.uint8, device="cuda"),
                "actions": torch.zeros((T, N) if discrete else (T, N, A), dtype=torch.int32 if discrete else torch.float32, device="cuda")}
    out = []
    for fused in (True, False):
        h = make_handle(space, N, rng=rng)
        p = planes()
        obs0 = torch.zeros((N, D), dtype=torch.float32, device="cuda")
        h.reset(obs_out=obs0.data_ptr())
        ptrs = tuple(p[k].data_ptr() for k in ("obs", "reward", "done", "actions"))
        if fused:
            if hidden:
                h.rollout_mlp_policy(T, d_par.data_ptr(), hidden, per_env=True, freeze_after_done=True, out=ptrs, sample=sample, **stats)
            else:
                h.rollout_policy(T, d_par.data_ptr(), per_env=True, freeze_after_done=True, out=ptrs, **stats)
        else:
            frozen = torch.zeros((N,), dtype=torch.uint8, device="cuda")
            pol = dict(params=d_par.data_ptr(), hidden=hidden) if hidden else dict(weights=d_par.data_ptr())
            for t in range(T):
                src = obs0 if t == 0 else p["obs"][t - 1]
                h.policy_act(src.data_ptr(), D, p["actions"][t].data_ptr(), per_env=True, freeze_after_done=True, sample=sample,
                             done_prev=p["done"][t - 1].data_ptr() if t else None, frozen=frozen.data_ptr(), **pol, **stats)
                h.step(p["actions"][t].data_ptr(), out=(p["obs"][t].data_ptr(), p["reward"][t].data_ptr(), p["done"][t].data_ptr()))
        h.sync()
        out.append({k: v.cpu().numpy() for k, v in p.items()})
        h.close()
    return out


def assert_planes_equal(a, b):
    for k in ("actions", "obs", "reward", "done"):
        assert np.array_equal(pe.bits(a[k]) if a[k].dtype != np.uint8 else a[k], pe.bits(b[k]) if b[k].dtype != np.uint8 else b[k]), k


@pytest.mark.parametrize("space,rng,what", [(("d", 4), "PHILOX", "linear"), (("d", 4), "PHILOX", "mlp"), (("d", 4), "PHILOX", "sampled"),
                                            (("d", 4), "MT19937", "sampled"), (("c", 2), "MT19937", "linear"), (("c", 2), "MT19937", "mlp")])
def test_closed_loop_equals_the_fused_rollout_mobile(space, rng, what):
    N, T, D, A = 7, 253, 2, space[1]
    norm = pe.MOBILE_NORM if rng == "PHILOX" else (None, None, 10.0)
    if what == "linear":
        params, hidden = pe.dyadic_params(100, D, A, N, tie_groups=pe.tie_patterns(A)), 0
    else:
        params, hidden = pe.dyadic_params(203, D, A, N, hidden=17, tie_groups=pe.tie_patterns(A) + [None], dead=0.25, all_dead_every=6), 17
    fused, loop = closed_loop(space, rng, N, T, params, hidden, norm, sample=what == "sampled")
    assert fused["done"].any() and (fused["actions"][-1] == (-1 if space[0] == "d" else 0)).all()      # crosses the episode end and the freeze
    assert_planes_equal(fused, loop)


@pytest.mark.parametrize("case", [c for c in pe.KUKA if c[0] == "KUKA_BUTTON" and c[4] == 5] + [pe.KUKA[6]], ids=str)
def test_closed_loop_equals_the_fused_rollout_kuka(case):
    """policy_exact's KukaButton cases as they are (dyadic parameters: the fused Kuka kernels' freedom to fuse a product with its sum
    is empty on them)"""
    env, discrete, joints, rng, n, H, per_env, normalize, seed = case
    space = ("d", 6) if discrete else ("c", 7 if joints else 3)
    params = pe.kuka_params(case)[:5]
    norm = pe.norm_of(normalize, pe.KUKA_NORM, 3)
    fused, loop = closed_loop(space, rng, 5, 24, params, H, norm)
    assert_planes_equal(fused, loop)
    if discrete and H:
        fused, loop = closed_loop(space, rng, 5, 24, params, H, norm, sample=True)
        assert_planes_equal(fused, loop)


def test_refusals_by_message():
    from srlhip import _lib
    torch = torch_()
    N, D, H = 5, 3, 16
    h = make_handle(("d", 4), N)
    obs, act = torch.zeros((N, D), device="cuda"), torch.zeros((N,), dtype=torch.int32, device="cuda")
    par32, par64 = torch.zeros((N, 4096), device="cuda"), torch.zeros((N, D, 4), dtype=torch.float64, device="cuda")
    frozen = torch.zeros((N,), dtype=torch.uint8, device="cuda")

    def refuse(code, text, *a, **kw):
        with pytest.raises(_lib.SrlHipError, match=text) as err:
            h.policy_act(*a, **kw)
        assert "({})".format(code) in str(err.value)
    refuse(-22, "hidden must be in 1..128", obs.data_ptr(), D, act.data_ptr(), params=par32.data_ptr(), hidden=129)
    refuse(-22, "hidden must be in 1..128", obs.data_ptr(), D, act.data_ptr(), params=par32.data_ptr(), hidden=0)
    refuse(-22, "obs_dim must be in 1..1024", obs.data_ptr(), 1025, act.data_ptr(), params=par32.data_ptr(), hidden=H)
    refuse(-22, "obs_dim must be in 1..1024", obs.data_ptr(), 0, act.data_ptr(), weights=par64.data_ptr())
    refuse(-22, "only an MLP policy's actions are sampled", obs.data_ptr(), D, act.data_ptr(), weights=par64.data_ptr(), sample=True)
    refuse(-22, "needs the frozen plane", obs.data_ptr(), D, act.data_ptr(), weights=par64.data_ptr(), freeze_after_done=True)
    pol = _lib.MlpPolicy()
    pol.struct_size, pol.hidden, pol.params = 8, H, par32.data_ptr()
    import ctypes
    rc = h._lib.srlhip_policy_act(h._h, None, ctypes.byref(pol), 0, obs.data_ptr(), D, None, None, act.data_ptr(), None)
    assert rc == -22 and "struct_size mismatch" in h.last_error()
    rc = h._lib.srlhip_policy_act(h._h, None, None, 0, obs.data_ptr(), D, None, None, act.data_ptr(), None)
    assert rc == -22 and "exactly one" in h.last_error()
    h.policy_act(obs.data_ptr(), D, act.data_ptr(), params=par32.data_ptr(), hidden=H, frozen=frozen.data_ptr(), freeze_after_done=True)
    h.close()
    h = make_handle(("c", 2), N)
    actf = torch.zeros((N, 2), device="cuda")
    refuse(-95, "discrete", obs.data_ptr(), D, actf.data_ptr(), params=par32.data_ptr(), hidden=H, sample=True)
    h.close()
    h = make_handle(("d", 4), N, io_device=0)
    h.reset()
    refuse(-95, "device-pointer handles only", obs.data_ptr(), D, act.data_ptr(), params=par32.data_ptr(), hidden=H)
    h.step_async(np.zeros(N, np.int32))
    refuse(-22, "srlhip_step_async is pending", obs.data_ptr(), D, act.data_ptr(), params=par32.data_ptr(), hidden=H)
    h.step_wait()
    h.close()


def test_works_on_a_pixel_handle():
    """any observation mode: the call never looks at the env state"""
    from srlhip import _lib
    space, N, D, H, A = ("d", 6), 5, 20, 100, 6
    h = make_handle(space, N, obs_mode=_lib.OBS_RAW_PIXELS)
    obs, params, mean, std, clip = gaussian(41, N, D, H, A, 1)
    got = Call(h, space, D)(obs, params, H, 1, mean, std, clip)
    want = par.act(obs, D, A, True, params=params, hidden=H, mean=mean, std=std, clip=clip)
    h.close()
    assert np.array_equal(pe.bits(got["score"]), pe.bits(want["score"])) and np.array_equal(got["action"], want["action"])
