"""srlhip_policy_act without a GPU: the numpy restatement of its contract (tests/policy_act_ref.py) against the plain numpy forward and
against the library's own per-env text (csrc/policy_act.hpp) run as the stand-alone host program policy_hostcheck, plus the argument
rules of the learners that use it."""
import argparse
import os
import subprocess

import numpy as np
import pytest

import mlp_policy_ref as ref
import policy_act_ref as par
import policy_exact as pe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "robotics-rl-srl_amd", "csrc")
PROGRAMS = ("policy_hostcheck", "policy_hostcheck_san")        # plain, and under the address / undefined-behaviour sanitizers

NS, DS, HS = (1, 5), (1, 3, 17, 200), (1, 16, 17, 100, 128)
A_DISCRETE, A_CONTINUOUS = (2, 4, 6), (2, 3, 7)


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-s", "-C", CSRC, "policyhostcheck"], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    return [os.path.join(CSRC, "build", p) for p in PROGRAMS]


def bits(a):
    return pe.bits(np.ascontiguousarray(a))


def make_case(seed, N, D, H, A, discrete, per_env, normalize=True, freeze=True, has_done=True, none_nan=False, sample=False):
    """Gaussian parameters, observations with a few exact zeros and negative zeros, statistics whose clip bites"""
    rng = np.random.RandomState(seed)
    obs = rng.standard_normal((N, D)).astype(np.float32)
    obs[rng.random_sample((N, D)) < 0.1] = np.float32(-0.0)
    lead = (N,) if per_env else ()
    if H:
        params = ref.random_params(seed + 1, lead + (ref.param_count(D, H, A),))
        w1, b1, w2, b2 = ref.split(params, D, H, A)
        b2[..., 0] = -0.0                                  # a bias of -0.0 in front of lane 0's sum
        if N > 1 and per_env:
            params[1] = 0.0                                # every score +0.0: the tie goes to index 0
            params[1, ::3] = -0.0
    else:
        params = 0.5 * rng.standard_normal(lead + (D, A))
        if N > 1 and per_env:
            params[1] = -0.0                               # every product -0.0: the zero score keeps the sign of the sum
    mean, std, clip = 0.1 * rng.standard_normal(D), 0.5 + rng.random_sample(D), 1.25
    if not H and N > 1 and per_env:
        obs[1] = (mean + std * (0.25 + 0.5 * rng.random_sample(D))).astype(np.float32)        # x > 0 with and without the statistics
    done_prev = rng.randint(0, 4, size=N).astype(np.uint8)                   # bit 1 alone must not freeze
    frozen = (rng.random_sample(N) < 0.3).astype(np.uint8)
    u = rng.random_sample(N)
    return dict(N=N, D=D, H=H, A=A, discrete=discrete, per_env=per_env, normalize=normalize, freeze=freeze, has_done=has_done,
                none_nan=none_nan, sample=sample, obs=obs, params=params, mean=mean, std=std, clip=clip, done_prev=done_prev,
                frozen=frozen, u=u)


def run_program(prog, c, tmp_path):
    head = np.array([c["N"], c["D"], c["H"], c["A"], c["per_env"], c["normalize"], c["freeze"], c["discrete"], c["sample"], c["none_nan"],
                     c["has_done"], 0], np.int32)
    blob = b"".join([head.tobytes(), np.float64(c["clip"]).tobytes(), c["obs"].astype(np.float32).tobytes(),
                     (c["params"].astype(np.float32) if c["H"] else c["params"].astype(np.float64)).tobytes(),
                     c["mean"].astype(np.float64).tobytes(), c["std"].astype(np.float64).tobytes(), c["done_prev"].tobytes(),
                     c["frozen"].tobytes(), c["u"].astype(np.float64).tobytes()])
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(blob)
    done = subprocess.run([prog, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode()
    raw = open(dst, "rb").read()
    N, A, o = c["N"], c["A"], 0
    score = np.frombuffer(raw, np.float64, N * A, o).reshape(N, A); o += 8 * N * A
    w = np.frombuffer(raw, np.float64, N * A, o).reshape(N, A); o += 8 * N * A
    if c["discrete"]:
        action = np.frombuffer(raw, np.int32, N, o); o += 4 * N
    else:
        action = np.frombuffer(raw, np.float32, N * A, o).reshape(N, A); o += 4 * N * A
    frozen = np.frombuffer(raw, np.uint8, N, o); o += N
    assert o == len(raw)
    return dict(score=score, w=w, action=action, frozen=frozen)


def reference(c):
    kw = dict(weights=c["params"]) if not c["H"] else dict(params=c["params"], hidden=c["H"])
    return par.act(c["obs"], c["D"], c["A"], c["discrete"], per_env=c["per_env"], mean=c["mean"] if c["normalize"] else None,
                   std=c["std"] if c["normalize"] else None, clip=c["clip"], freeze=c["freeze"],
                   done_prev=c["done_prev"] if c["has_done"] else None, frozen=c["frozen"], none_nan=c["none_nan"],
                   u=c["u"] if c["sample"] else None, **kw)


def check(prog, c, tmp_path):
    got, want = run_program(prog, c, tmp_path), reference(c)
    assert np.array_equal(bits(got["score"]), bits(want["score"])), (c["N"], c["D"], c["H"], c["A"])
    assert np.array_equal(got["frozen"], want["frozen"])
    if c["sample"]:
        # the exp is libm's here and numpy's in the reference: the weights agree to 2 ulp, and GIVEN the program's own weights the
        # pick is the reference's bit for bit
        assert np.all(np.abs(got["w"] - want["w"]) <= 2 * np.spacing(want["w"]))
        picked = par.none_rows(par.pick(got["w"], c["u"]), ~want["live"], True, False)
        assert np.array_equal(got["action"], picked)
    else:
        assert np.array_equal(bits(got["action"]), bits(want["action"]))
    return want


def test_clip_bites_and_zero_signs_are_covered():
    c = make_case(7, 5, 17, 17, 4, True, True)
    x = par.inputs(c["obs"], c["mean"], c["std"], c["clip"])
    assert (x == np.float32(c["clip"])).any() and (x == np.float32(-c["clip"])).any() and (np.abs(x) < c["clip"]).any()
    lin = make_case(8, 5, 3, 0, 4, True, True, normalize=False)
    s = par.linear_scores(par.inputs(lin["obs"]), lin["params"])
    assert (s[1] == 0).all() and np.signbit(s[1]).any()          # a zero of the linear policy keeps its sign ...
    m = make_case(9, 5, 3, 16, 4, True, True)
    sm = par.mlp_scores(par.inputs(m["obs"], m["mean"], m["std"], m["clip"]), m["params"], 16, 4)
    assert (sm[1] == 0).all() and not np.signbit(sm[1]).any()    # ... the MLP's is +0.0 whatever the signs of the terms


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("H", HS)
def test_reference_within_the_rounding_bound_of_the_plain_forward(D, H):
    """the header's bound, generalised to D: (2 D + H + 16) 2^-53 S"""
    for A in (2, 7):
        c = make_case(100 + D + H, 5, D, H, A, False, True)
        x = par.inputs(c["obs"], c["mean"], c["std"], c["clip"])
        plain, S = ref.forward(c["params"], x, D, H, A)
        got = par.mlp_scores(x, c["params"], H, A)
        assert np.all(np.abs(got - plain) <= par.tol_factor(D, H) * S)
    assert par.tol_factor(1024, 128) < 2.0 ** -41 and par.tol_factor(3, 128) < 2.0 ** -45


@pytest.mark.parametrize("D,H,A", [(3, 1, 6), (3, 17, 6), (3, 128, 7), (2, 16, 4), (17, 100, 3), (200, 100, 6)])
def test_reference_is_the_plain_sum_on_dyadic_parameters(D, H, A):
    """policy_exact's parameters on dyadic observations: wherever every sum passes order_free, the order-exact reference IS the plain
    numpy sum, bit for bit"""
    rng = np.random.RandomState(D * 1000 + H)
    n = 12
    params = pe.dyadic_params(400 + H, D, A, n, hidden=H, tie_groups=pe.tie_patterns(A) + [None], dead=0.25, all_dead_every=6, zero_every=11,
                              neg_zero_b2_every=5)
    obs = (rng.randint(-64, 65, size=(n, D)) / 64.0).astype(np.float32)
    score, exact, _ = pe.expected(obs[None], params, True, hidden=H)
    got = par.mlp_scores(obs, params, H, A)
    ex = exact[0]
    assert ex.mean() > 0.9
    assert np.array_equal(bits(got[ex]), bits(score[0][ex]))
    W = pe.dyadic_params(500 + D, D, A, n, tie_groups=pe.tie_patterns(A))
    lscore, lexact, _ = pe.expected(obs[None], W, True)
    lgot = par.linear_scores(obs, W)
    assert np.array_equal(bits(lgot[lexact[0]]), bits(lscore[0][lexact[0]]))


@pytest.mark.parametrize("which", range(len(PROGRAMS)), ids=PROGRAMS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DS)
def test_hostcheck_equals_the_reference(programs, tmp_path, which, N, D):
    prog = programs[which]
    seed = 1000 * N + D
    for H in HS:
        for per_env in (1, 0):
            for A in A_DISCRETE:
                check(prog, make_case(seed + H + A, N, D, H, A, True, per_env), tmp_path)
            for A in A_CONTINUOUS:
                check(prog, make_case(seed + H + A + 50, N, D, H, A, False, per_env, none_nan=A != 2), tmp_path)
        check(prog, make_case(seed + H, N, D, H, 6, True, 1, sample=True), tmp_path)
        check(prog, make_case(seed + H, N, D, H, 4, True, 1, normalize=False, freeze=False), tmp_path)
    for per_env in (1, 0):
        for A in A_DISCRETE:
            check(prog, make_case(seed + A, N, D, 0, A, True, per_env), tmp_path)
        for A in A_CONTINUOUS:
            check(prog, make_case(seed + A + 50, N, D, 0, A, False, per_env, none_nan=A != 2, has_done=A != 3), tmp_path)


def test_frozen_bookkeeping(programs, tmp_path):
    c = make_case(3, 5, 3, 16, 4, True, 1)
    c["done_prev"] = np.array([0, 1, 2, 3, 0], np.uint8)
    c["frozen"] = np.array([0, 0, 0, 0, 1], np.uint8)
    want = check(programs[0], c, tmp_path)
    assert want["frozen"].tolist() == [0, 1, 0, 1, 1] and (want["action"] == -1).tolist() == [False, True, False, True, True]
    c["has_done"] = 0                                       # NULL done_prev: only who was frozen stays frozen
    assert check(programs[0], c, tmp_path)["frozen"].tolist() == [0, 0, 0, 0, 1]
    c["freeze"], c["has_done"] = 0, 1                       # freeze_after_done = 0 ignores both planes
    want = check(programs[0], c, tmp_path)
    assert want["frozen"].tolist() == [0, 0, 0, 0, 1] and (want["action"] >= 0).all()


# ---- the learners' argument rules ---------------------------------------------------------------------------------------------------------
def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", fused_rollout=True, deterministic=True, continuous_actions=False, num_stack=1,
                srl_model="ground_truth", fused_sampling=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_fused_arguments_accept_a_learned_srl_model():
    from rl_baselines.evolution_strategies.ars import ARSModel
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    for name in ("autoencoder", "robotic_priors", "pca"):
        ARSModel.check_fused_arguments(_args(srl_model=name))
        CMAESModel.check_fused_arguments(_args(srl_model=name))
        CMAESModel.check_fused_arguments(_args(srl_model=name, deterministic=False, fused_sampling=True))
    ARSModel.check_fused_arguments(_args())
    for name in ("raw_pixels", "joints", "joints_position"):
        for model, extra in ((ARSModel, {}), (CMAESModel, {}), (CMAESModel, dict(deterministic=False, fused_sampling=True))):
            with pytest.raises(ValueError, match="srl-model ground_truth"):
                model.check_fused_arguments(_args(srl_model=name, **extra))
    with pytest.raises(ValueError, match="deterministic"):
        ARSModel.check_fused_arguments(_args(srl_model="autoencoder", deterministic=False))
