"""srlhip_knn's contract restated in numpy (csrc/knn.hpp: the distance's terms AND their order, the total order of the neighbours, the
error term), the case generators and shape lists the CPU and GPU tests share, and the case-file format of csrc/knn_hostcheck.cpp.

DISTANCE.  diff_s = x[i][s] - x[j][s], d = fma(diff_s, diff_s, d) for s ascending from +0.0, fma being libm's correctly rounded one (the
kernel's v_fma_f64).  `exact=True` replaces the fma by d + diff * diff for inputs on which no operation rounds (multiples of 2^-8 below
2^10 in magnitude: a difference has at most 19 significant bits, its square 38, a sum of 64 of them 44) — asserted, not assumed; it is what
keeps the larger "grid" case cheap; `fast=True` is fma_square below, the same bits as libm's fma without a call per element (the larger
"random" case; the CPU tests hold it against the libm route).
NEIGHBOURS.  np.lexsort((j, d)) per query with the query's own index removed; a NaN or +inf distance never enters, such slots are
(-1, +inf).
ERR.  e = fma(t, t, e), t = gt[idx][g] - gt[i][g], neighbours outer, g inner, slots of -1 skipped, / k."""
import ctypes
import ctypes.util
import functools
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "robotics-rl-srl_amd", "csrc")
PROGRAMS = ("knn_hostcheck", "knn_hostcheck_san")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(_libm.fma, 3, 1)

CONTENTS = ("random", "grid", "equal", "f32", "wide")
NS, SS, KS, GS = (2, 3, 33, 63, 64, 65, 130), (1, 2, 3, 33, 64), (1, 5, 32), (1, 3, 14)


def shapes():
    """(N, S, k, G): every N, S, k and G of the lists appears, each N with every admissible k; S and G cycle"""
    out, c = [], 0
    for N in NS:
        for k in KS:
            if k <= N - 1:
                out.append((N, SS[c % len(SS)], k, GS[c % len(GS)]))
                c += 1
    for S in SS:
        out.append((65, S, 5, GS[c % len(GS)]))
        c += 1
    return out


def make_states(content, N, S, seed=0):
    rng = np.random.RandomState(seed + 1000 * N + S)
    if content == "random":
        return rng.randn(N, S)
    if content == "grid":
        return rng.randint(0, 3, size=(N, S)).astype(np.float64)
    if content == "equal":
        return np.tile(rng.randn(1, S), (N, 1))
    if content == "f32":
        return rng.randn(N, S).astype(np.float32)
    if content == "wide":
        # magnitudes 1e-150 .. 1e150 mixed: squares underflow; one value in fifty is of magnitude 1e160, whose square overflows, so that
        # rows with fewer than k finite distances exist (test_knn_cpu.py checks that they do)
        return rng.randn(N, S) * 10.0 ** rng.choice([-150, -3, 0, 3, 150, 160], size=(N, S), p=[0.245, 0.245, 0.245, 0.1225, 0.1225, 0.02])
    raise ValueError(content)


def make_ground_truth(N, G, seed=0):
    return np.random.RandomState(seed + 7 * N + G).randn(N, G)


def query_lists(N, seed=0):
    """None (every row); a strict subset, ascending; a list with a repeated index in descending order"""
    rng = np.random.RandomState(seed + N)
    sub = np.sort(rng.choice(N, max(1, N // 2), replace=False)).astype(np.int32)
    rep = np.sort(rng.choice(N, min(N, 5), replace=False))[::-1].astype(np.int32)
    rep = np.concatenate([rep[:1], rep]).astype(np.int32)
    return [None, sub, rep]


def fma_square(diff, d):
    """fma(diff, diff, d) elementwise without a libm call per element: p + e = diff^2 exactly (Dekker's product on Veltkamp's split), s + t =
    p + d exactly (two-sum), and round(s + (t + e)) is the fused result wherever the rounding of t + e cannot carry the sum across a
    rounding boundary of s; the elements where it might (t + e within 1e-9 ulp of a half or quarter ulp of s), and those outside the
    range in which the splits are exact, go through libm."""
    p = diff * diff
    c = 134217729.0 * diff
    hi = c - (c - diff)
    lo = diff - hi
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    s = p + d
    bb = s - p
    t = (p - (s - bb)) + (d - bb)
    rem = t + e
    r = s + rem
    u = np.spacing(np.abs(s))
    doubt = (np.abs(np.abs(rem) - 0.5 * u) <= 1e-9 * u) | (np.abs(np.abs(rem) - 0.25 * u) <= 1e-9 * u)
    a = np.abs(diff)
    doubt |= ~np.isfinite(r) | ((a != 0.0) & ((a < 1e-100) | (a > 1e100))) | (np.abs(d) > 1e200)
    if doubt.any():
        r[doubt] = _fma(diff[doubt], diff[doubt], d[doubt]).astype(np.float64)
    return r


def distances(x, rows, exact=False, fast=False):
    """float64 [len(rows)][N] in the contract's order"""
    x = np.asarray(x).astype(np.float64)
    if exact:
        assert np.array_equal(x * 256.0, np.round(x * 256.0)) and np.abs(x).max() < 1024.0 and x.shape[1] <= 64
    d = np.zeros((len(rows), len(x)))
    for s in range(x.shape[1]):
        diff = x[rows, s][:, None] - x[None, :, s]
        d = d + diff * diff if exact else fma_square(diff, d) if fast else _fma(diff, diff, d).astype(np.float64)
    return d


def neighbours(x, k, queries=None, ground_truth=None, exact=False, fast=False):
    """-> (idx int32 [Q][k], dist float64 [Q][k][, err float64 [Q]])"""
    N = len(x)
    rows = np.arange(N) if queries is None else np.asarray(queries, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = distances(x, rows, exact, fast)
    idx, dist = np.full((len(rows), k), -1, np.int32), np.full((len(rows), k), np.inf)
    for q, i in enumerate(rows):
        j = np.arange(N)
        keep = (j != i) & (d[q] < np.inf)              # NaN and +inf never enter
        j, dq = j[keep], d[q][keep]
        order = np.lexsort((j, dq))[:k]
        idx[q, :len(order)], dist[q, :len(order)] = j[order], dq[order]
    if ground_truth is None:
        return idx, dist
    gt = np.asarray(ground_truth, dtype=np.float64)
    err = np.zeros(len(rows))
    for q, i in enumerate(rows):
        e = 0.0
        for n in range(k):
            if idx[q, n] < 0:
                continue
            for g in range(gt.shape[1]):
                t = gt[idx[q, n], g] - gt[i, g]
                e = _libm.fma(t, t, e)
        err[q] = e / float(k)
    return idx, dist, err


@functools.lru_cache(maxsize=None)
def case(content, N, S, k, G, which):
    """-> (states, ground truth, queries, (idx, dist, err)) of query list `which` of query_lists(N): computed once per process, shared by
    the CPU and the GPU tests, never written to.  The distances come from fma_square, which test_knn_cpu.py holds against libm's fma."""
    x, gt = make_states(content, N, S), make_ground_truth(N, G)
    queries = query_lists(N)[which]
    want = neighbours(x, k, queries, gt, fast=True)
    for a in (x, gt) + want + (() if queries is None else (queries,)):
        a.setflags(write=False)
    return x, gt, queries, want


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def build_programs():
    subprocess.check_call(["make", "-s", "-C", CSRC, "knnhostcheck"])
    return [os.path.join(CSRC, "build", p) for p in PROGRAMS]


def write_case(path, x, k, queries=None, ground_truth=None):
    x = np.ascontiguousarray(x)
    f32 = x.dtype == np.float32
    N, S = x.shape
    Q = 0 if queries is None else len(queries)
    G = 0 if ground_truth is None else ground_truth.shape[1]
    with open(path, "wb") as f:
        f.write(np.array([N, S, k, Q, G, int(f32)], np.int64).tobytes())
        f.write(x.astype(np.float32 if f32 else np.float64).tobytes())
        if Q:
            f.write(np.ascontiguousarray(queries, dtype=np.int32).tobytes())
        if G:
            f.write(np.ascontiguousarray(ground_truth, dtype=np.float64).tobytes())


def read_result(path, rows, k, has_gt):
    raw = open(path, "rb").read()
    idx = np.frombuffer(raw, np.int32, rows * k).reshape(rows, k)
    dist = np.frombuffer(raw, np.float64, rows * k, offset=4 * rows * k).reshape(rows, k)
    err = np.frombuffer(raw, np.float64, rows, offset=12 * rows * k) if has_gt else None
    return idx, dist, err
