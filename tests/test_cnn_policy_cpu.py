"""srlhip_cnn_policy_act without a GPU: the float64 restatement (tests/cnn_policy_ref.py) against the reference's own module
(tests/golden/cnn_policy_reference.npz), the library's per-env text (csrc/cnn_policy.hpp) run as the stand-alone host program
cnn_policy_hostcheck — plain and under the address / undefined-behaviour sanitizers — against the restatement, the shape arithmetic
against torch's own output shapes, and every refusal of the header comment."""
import os
import subprocess

import numpy as np
import pytest

import cnn_policy_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cnn_policy_reference.npz")


@pytest.fixture(scope="module")
def programs():
    ref.build_programs()
    return ref.PROGRAMS


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("tag", ["224", "64"])
def test_restatement_equals_the_reference_module(golden, tag):
    """float64 against the recorded .double() outputs: rounding-level agreement, 64 x 2^-53 F max|term| (the two sum the same F products
    per score behind three layers whose own rounding is amplified by at most the layers' gains: 64 is that allowance)"""
    frames, params, want = golden["frames_" + tag], golden["params_" + tag], golden["scores64_" + tag]
    A = want.shape[1]
    H, W, C = frames.shape[1:]
    for e in range(len(frames)):
        got = ref.forward64(params[e], frames[e], A)
        fcw = ref.split(params[e], C, H, W, A)[9].astype(np.float64)
        F = fcw.shape[1]
        bound = 64 * 2.0 ** -53 * F * max(1.0, np.abs(fcw).max() * 8.0)      # |x_f| stays below 8 behind a batch-norm with |gamma| < 2.5
        assert np.abs(got - want[e]).max() <= bound, (np.abs(got - want[e]).max(), bound)
        # and the float32 module as CMA-ES drives it is the float32 yardstick's neighbour
        assert ref.rel_err(golden["scores_" + tag][e], got) < 1e-4
        p = np.exp(got - got.max())
        assert np.abs(golden["proba_" + tag][e] - p / p.sum()).max() < 1e-4


def test_param_count_and_shapes_match_torch(programs):
    import torch
    lines = subprocess.check_output([os.path.join(ref.CSRC, "build", programs[0]), "shapes"]).decode().splitlines()
    seen = set()
    for line in lines:
        t = line.split()
        C, H, W, A, ok = (int(v) for v in (t[1], t[2], t[3], t[4], t[6]))
        planes = [int(v) for v in t[8:20]]
        assert ok == int(43 <= H <= 224 and 43 <= W <= 224), line
        if not ok:
            continue
        seen.add(H)
        x = torch.zeros((1, C, H, W))
        want, cin = [], C
        for co, k, pad in ref.LAYERS:
            x = torch.nn.functional.conv2d(x, torch.zeros((co, cin, k, k)), stride=2, padding=pad)
            want += [x.shape[2], x.shape[3]]
            x = torch.nn.functional.max_pool2d(x, 2)
            want += [x.shape[2], x.shape[3]]
            cin = co
        assert planes == want, line
        F = int(x.numel())
        assert int(t[21]) == F and int(t[23]) == ref.param_count(C, H, W, A) == 200 * C + 16 + 1152 + 32 + 4608 + 64 + A * F + A, line
    assert seen == set(range(43, 225))
    assert ref.param_count(3, 224, 224, 6) == 8206 and ref.shape(3, 224, 224)[2] == 288
    assert ref.shape(3, 42, 42)[2] == 0 and ref.shape(3, 43, 43)[1][2] == (1, 1) and ref.shape(3, 43, 43)[0][2] == (2, 2)


def test_refusals_are_the_header_comments(programs):
    for program in programs:
        got = dict(line.split(": ", 1) for line in subprocess.check_output([os.path.join(ref.CSRC, "build", program), "refusals"]).decode().splitlines())
        EINVAL, ENOTSUP = "-22", "-95"
        for key in ("null policy", "struct_size", "reserved", "null params", "null images", "null act_out", "freeze without frozen"):
            assert got[key].startswith(EINVAL + " "), (key, got[key])
        for key, word in (("host-pointer handle", "io_device"), ("ground_truth", "raw_pixels"), ("img_h 42", "43..224"), ("img_w 225", "43..224"),
                          ("sample continuous", "discrete")):
            assert got[key].startswith(ENOTSUP + " ") and word in got[key], (key, got[key])
        for key in ("policy", "planes", "43 x 224", "continuous"):
            assert got[key] == "0 accepted", (key, got[key])


CASES = ref.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_program_against_float64(programs, tmp_path, case):
    _, frames, params, A, per_env = case
    s64 = ref.forward64_batch(params, frames, A, per_env)
    rng = np.random.RandomState(3)
    u = rng.random_sample(len(frames))
    first = None
    for program in programs:
        det = ref.run_program(program, tmp_path, frames, params, A, per_env=per_env)
        err = ref.rel_err(det["score"], s64)
        print(case[0], program, "score error", err, "tolerance", ref.SCORE_TOL)
        assert err <= ref.SCORE_TOL
        assert np.array_equal(det["act"], det["score"].astype(np.float64).argmax(axis=1))       # numpy's argmax: the first maximum
        smp = ref.run_program(program, tmp_path, frames, params, A, per_env=per_env, sample=True, u=u)
        assert np.array_equal(smp["score"], det["score"])
        for e in range(len(frames)):
            assert ref.sample_accepts(smp["score"][e], u[e], int(smp["act"][e]), 0.0), (e, smp["act"][e])
        cont = ref.run_program(program, tmp_path, frames, params, A, per_env=per_env, discrete=False)
        assert np.array_equal(cont["act"], det["score"])
        if first is None:
            first = det
        assert np.array_equal(first["score"], det["score"])                                    # the sanitised build computes the same bits


def test_freeze_and_constant_frame(programs, tmp_path):
    frames, params, done_prev, frozen = ref.constant_case()
    n, A = 5, 6
    for program in programs:
        r = ref.run_program(program, tmp_path, frames, params, A, freeze=True, done_prev=done_prev, frozen=frozen)
        assert r["frozen"].tolist() == [0, 1, 1, 1, 0]
        live = r["frozen"] == 0
        assert np.array_equal(r["act"][~live], [-1, -1, -1]) and np.array_equal(r["act"][live], r["score"][live].astype(np.float64).argmax(axis=1))
        c = ref.run_program(program, tmp_path, frames, params, A, freeze=True, discrete=False, done_prev=done_prev, frozen=frozen)
        assert np.isnan(c["act"][~live]).all() and np.array_equal(c["act"][live], r["score"][live])
        z = ref.run_program(program, tmp_path, frames, params, A, freeze=True, discrete=False, none_nan=False, done_prev=done_prev, frozen=frozen)
        assert (z["act"][~live] == 0).all()
        s64 = ref.forward64_batch(params, frames, A)
        keep = np.arange(n) != 2
        assert ref.rel_err(r["score"][keep], s64[keep]) <= ref.SCORE_TOL
        err_c = ref.rel_err(r["score"][2], s64[2])
        print(program, "constant frame: score error", err_c, "tolerance", ref.SCORE_TOL_CONSTANT)
        assert err_c <= ref.SCORE_TOL_CONSTANT


def test_yardstick_constants():
    """E32 and E32_CONSTANT of tests/cnn_policy_ref.py are what the float32 PyTorch CPU forward gives on these inputs: the pinned constants
    may not be smaller than half the measurement nor larger than twice it"""
    e32 = 0.0
    for _, frames, params, A, per_env in CASES:
        for e in range(len(frames)):
            p = params[e] if per_env else params
            e32 = max(e32, ref.rel_err(ref.forward32_torch(p, frames[e], A), ref.forward64(p, frames[e], A)))
    frames, params = ref.constant_case()[:2]
    e32_c = ref.rel_err(ref.forward32_torch(params[2], frames[2], 6), ref.forward64(params[2], frames[2], 6))
    print("E32 measured", e32, "pinned", ref.E32, "| constant frame measured", e32_c, "pinned", ref.E32_CONSTANT)
    assert 0.5 * e32 <= ref.E32 <= 2.0 * e32
    assert 0.5 * e32_c <= ref.E32_CONSTANT <= 2.0 * e32_c
