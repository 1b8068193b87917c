"""srlhip_pca_* without a GPU: the rules over their table, the library's host twin (srlhip_pca_project_host: the kernel's own text,
csrc/pca_project.hpp) against the numpy restatement bit for bit and against an exactly rounded reference within the derived bound
(tests/pca_ref.py), the stand-alone host program — plain and under the address / undefined-behaviour sanitizers — against the library,
and SRLPCA on the CPU, which stays the torch formulation."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pca_ref as ref

sys.path.insert(0, os.path.join(ref.REPO, "robotics-rl-srl_amd"))
from srlhip import _lib  # noqa: E402

# F: 192 = 8 x 8 x 3 (below one chunk), 720 (ragged against any power-of-two chunk), 12288 = 64 x 64 x 3 (24 chunks)
SHAPES = [(F, S, whiten) for F in (192, 720, 12288) for S in (1, 5, 32) for whiten in (False, True)]
IDS = ["F%d S%d %s" % (F, S, "whitened" if wh else "plain") for F, S, wh in SHAPES]
N = 3


def _case(F, S, whiten):
    rng = np.random.RandomState(7 * F + 13 * S + int(whiten))
    w, b = ref.fold(ref.make_model(rng, F, S, whiten))
    return ref.make_frames(rng, N, F), w, b


@pytest.fixture(scope="module")
def twins():
    """(frames, w, b, the library's float64 states), once per shape"""
    out = {}
    for shape in SHAPES:
        frames, w, b = _case(*shape)
        out[shape] = (frames, w, b, _lib.pca_project_host(w, b, frames))
    return out


@pytest.fixture(scope="module")
def programs():
    ref.build_programs()
    return ref.PROGRAMS


def test_supported_over_the_table():
    for F in (0, 1, 12288, 301056):
        for S in (0, 1, 64, 65):
            assert _lib.pca_supported(F, S) == (F >= 1 and 1 <= S <= ref.MAX_DIM), (F, S)
    lib = _lib.load()
    w, b, x, out = np.zeros((4, 65)), np.zeros(65), np.zeros((1, 4), np.uint8), np.zeros((1, 65))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.srlhip_pca_project_host(4, 65, ptr(w), ptr(b), ptr(x), 1, ptr(out), 0) == -95
    assert lib.srlhip_pca_project_host(0, 1, ptr(w), ptr(b), ptr(x), 1, ptr(out), 0) == -95
    assert lib.srlhip_pca_project_host(4, 2, ptr(w), ptr(b), ptr(x), -1, ptr(out), 0) == -22
    assert lib.srlhip_pca_project_host(4, 2, ptr(w), ptr(b), None, 1, ptr(out), 0) == -22
    assert lib.srlhip_pca_project_host(4, 2, ptr(w), ptr(b), ptr(x), 1, ptr(out), 2) == -22
    assert lib.srlhip_pca_project_host(4, 2, ptr(w), ptr(b), None, 0, None, 0) == 0          # n = 0: a successful call


def test_create_without_a_gpu_fails_with_a_message():
    import torch
    lib = _lib.load()
    h = ctypes.c_void_p()
    w, b = np.zeros((4, 65)), np.zeros(65)
    assert lib.srlhip_pca_create(0, 4, 65, w.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)) == -95
    assert b"state_dim" in lib.srlhip_pca_last_error(None) and not h.value
    assert lib.srlhip_pca_create(0, 4, 2, None, None, ctypes.byref(h)) == -22
    if torch.cuda.is_available():
        return                                             # (with a GPU the create below succeeds: tests/test_gpu_pca.py)
    with pytest.raises(_lib.SrlHipError) as e:
        _lib.PcaProjector(0, np.zeros((4, 2)), np.zeros(2))
    assert "srlhip_pca_create failed (-5)" in str(e.value) and "hip" in str(e.value)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_twin_within_the_derived_bound_of_the_exact_reference(twins, shape):
    frames, w, b, got = twins[shape]
    want, T = ref.exact(frames, w, b)
    err, bnd = np.abs(got - want), ref.bound(w.shape[0], T)
    print("max |twin - exact| / bound", float((err / np.maximum(bnd, 1e-300)).max()))
    assert (err <= bnd).all()
    assert (T > 0).all()
    # the float32 states are the float64 ones rounded once
    assert ref.same_bits(_lib.pca_project_host(w, b, frames, states_f32=True), got.astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_twin_equals_the_numpy_restatement_bit_for_bit(twins, shape):
    frames, w, b, got = twins[shape]
    assert ref.same_bits(got, ref.project(frames, w, b))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_host_programs_give_the_library_bits(programs, twins, tmp_path, shape):
    frames, w, b, got = twins[shape]
    for program in programs:                               # the second one is the sanitised build: it must run clean and give the same bits
        assert ref.same_bits(ref.run_program(program, tmp_path, frames, w, b), got)
        assert ref.same_bits(ref.run_program(program, tmp_path, frames, w, b, states_f32=True), got.astype(np.float32))


def test_host_programs_on_ragged_batches(programs, tmp_path):
    """F of one feature, one below / at / above a chunk boundary, n = 0 and n = 1"""
    rng = np.random.RandomState(3)
    for F, S, n in ((1, 1, 1), (511, 3, 2), (512, 64, 1), (513, 7, 5), (1025, 2, 0)):
        w, b = ref.fold(ref.make_model(rng, F, S, True))
        frames = ref.make_frames(rng, n, F)
        want = _lib.pca_project_host(w, b, frames)
        assert ref.same_bits(want, ref.project(frames, w, b)) if n else want.shape == (0, S)
        for program in programs:
            assert ref.same_bits(ref.run_program(program, tmp_path, frames, w, b), want)


def test_rules_of_the_host_programs(programs):
    for program in programs:
        lines = subprocess.check_output([os.path.join(ref.CSRC, "build", program), "rules"]).decode().splitlines()
        shape = {tuple(int(v) for v in ln.split(":")[0].split()[1:]): ln.split(": ", 1)[1] for ln in lines if ln.startswith("shape ")}
        assert len(shape) == 16
        for (F, S), verdict in shape.items():
            ok = F >= 1 and 1 <= S <= ref.MAX_DIM
            assert verdict == "0 accepted" if ok else verdict.startswith("-95 pca: "), (F, S, verdict)
            assert bool(_lib.pca_supported(F, S)) == ok
        fwd = [ln.split(": ", 1)[1] for ln in lines if ln.startswith("forward ")]
        assert [v.split(" ")[0] for v in fwd] == ["-22", "0", "-22", "-22", "-22", "0"]
        launch = [ln for ln in lines if ln.startswith("launch ")]
        for ln in launch:
            t = ln.replace(":", "").split()
            F, S, n, nc, SP, tile, tiles, slab = (int(t[i]) for i in (2, 4, 6, 8, 10, 12, 14, 16))
            assert nc == ref.chunks(F) and SP >= S and SP in (8, 16, 32, 64) and SP < 2 * max(S, 5)
            assert tiles == -(-n // tile)
            # one launch covers every tile of a one-chunk frame; otherwise as many as keep its chunk sums within 512 MiB, at least one
            assert slab == (tiles if nc == 1 else min(tiles, max(1, (512 << 20) // (nc * tile * SP * 8)))), ln


def test_srlpca_on_the_cpu_is_the_torch_formulation():
    import torch
    from state_representation.models import SRLPCA
    rng = np.random.RandomState(11)
    pca = ref.make_model(rng, 192, 5, True)
    frames = ref.make_frames(rng, 4, 192).reshape(4, 8, 8, 3)
    w, b = ref.fold(pca)
    for backend in ("auto", "torch"):
        m = SRLPCA(5, cuda=False, backend=backend)
        m.set_model(pca)
        assert m.hip is None and m.backend == "gemm" and m.state_dtype == torch.float64
        got = m.getStates(frames)
        assert got.dtype == torch.float64 and tuple(got.shape) == (4, 5) and got.device.type == "cpu"
        assert np.array_equal(got.numpy(), torch.addmm(torch.from_numpy(b), torch.from_numpy(frames.reshape(4, -1)).to(torch.float64), torch.from_numpy(w)).numpy())
        assert np.allclose(m.getState(frames[0]), got[0].numpy(), rtol=1e-12, atol=1e-10)      # (torch's GEMM is not batch-invariant)
        assert m.replicate("cpu").hip is None
    with pytest.raises(RuntimeError):
        SRLPCA(5, cuda=False, backend="hip")
    with pytest.raises(ValueError):
        SRLPCA(5, backend="rocblas")
