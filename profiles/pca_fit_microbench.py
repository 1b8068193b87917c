"""srlhip_pca_gram (csrc/pca_gram.hip) against the torch formulation of the same exact product — `X.to(float64) @ X.T`, exact too because
every sum stays below 2^53 — in the same process, at 4096 frames of 64x64x3 and of 224x224x3; and the whole fit_pca
(state_representation/pca_fit.py) against the same steps done in torch (float64 copy, centring, Gram product, numpy eigh, back-projection).

    python profiles/pca_fit_microbench.py [--reps 10] [--points 4096x64,4096x224] [--state-dim 32] [--no-fit]

Timing of the launches: device events around `reps` back-to-back calls on one stream after 3 warm-up calls, the median of 5 such
batches; no clock is pinned, so the figures are at whatever clock the chip holds under this load.  The fits are wall-clock times of one
call after one warm-up call, synchronised at both ends (they contain the same host-side eigh).  The torch path's peak extra memory is
torch.cuda.max_memory_allocated over its calls less what was allocated before them.  The share of the int8 matrix peak is against
2 x the dense BF16 spec figure of 2.5 Pop/s = 5 Pop/s, counting the 2 N^2 F operations of the full product although only the upper
triangle of tiles is computed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "robotics-rl-srl_amd"), REPO]
from srlhip import _lib  # noqa: E402
from state_representation import pca_fit  # noqa: E402

I8_PEAK = 5.0e15


def timed(fn, reps):
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def wall(fn):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def torch_fit(x, k):
    """fit_pca's steps in torch: the float64 copy, the centred Gram product on the device, eigh in numpy, the back-projection"""
    N = x.shape[0]
    X = x.to(torch.float64)
    mean = X.mean(dim=0)
    X -= mean
    C = (X @ X.T).cpu().numpy()
    lam, U = pca_fit.top_pairs(C, k)
    W = torch.from_numpy(np.ascontiguousarray(U / np.sqrt(lam)[None, :])).to(x.device)
    comp = (X.T @ W).T.contiguous()
    return comp.cpu().numpy(), mean.cpu().numpy(), lam / (N - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", default="4096x64,4096x224")
    ap.add_argument("--state-dim", type=int, default=32)
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for point in args.points.split(","):
        n, side = (int(v) for v in point.split("x"))
        F = side * side * 3
        frames = torch.randint(0, 256, (n, F), dtype=torch.uint8, device=dev)
        gram = torch.empty((n, n), dtype=torch.int64, device=dev)
        rowsum = torch.empty((n,), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        row = {"n": n, "side": side, "F": F}
        for split in (0, 1):
            hip = lambda: _lib.pca_gram(0, frames.data_ptr(), n, F, gram.data_ptr(), rowsum.data_ptr(), split=split, stream=stream)      # noqa: E731
            for _ in range(3):
                hip()
            torch.cuda.synchronize()
            ms = timed(hip, args.reps)
            row["hip_ms_split%d" % split] = round(ms, 4)
            row["i8_peak_share_split%d" % split] = round(2.0 * n * n * F / (ms * 1e-3) / I8_PEAK, 4)
        ref = lambda: frames.to(torch.float64) @ frames.to(torch.float64).T                      # noqa: E731
        conv = lambda: frames.to(torch.float64)                                                   # noqa: E731
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(2):
            got = ref()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - base
        row["exact_match"] = bool((got.to(torch.int64) == gram).all())
        del got
        row["torch_ms"] = round(timed(ref, max(1, args.reps // 3)), 4)
        row["torch_convert_ms"] = round(timed(conv, max(1, args.reps // 3)), 4)
        row["torch_peak_extra_MB"] = round(extra / 1e6, 1)
        row["speedup"] = round(row["torch_ms"] / row["hip_ms_split0"], 2)
        tiles = (n + 31) // 32
        row["frame_bytes_MB"] = round(n * F / 1e6, 1)
        row["operand_bytes_loaded_MB"] = round((tiles * tiles) * 32 * F / 1e6, 1)      # a diagonal tile loads one operand, every other two
        row["plane_bytes_MB"] = round(n * n * 8 / 1e6, 1)
        torch.cuda.empty_cache()
        if not args.no_fit:
            k = args.state_dim
            ms, model = wall(lambda: pca_fit.fit_pca(frames, k, backend="hip"))
            row["fit_hip_ms"] = round(ms, 1)
            ms, (comp, mean, var) = wall(lambda: torch_fit(frames, k))
            row["fit_torch_ms"] = round(ms, 1)
            row["fit_variance_max_rel_diff"] = float(np.abs(var / model.explained_variance_ - 1).max())
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
