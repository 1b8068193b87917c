"""srlhip_knn (csrc/knn.hip) against the torch formulation of the same search — `torch.cdist` in float64, the query's own column set to
+inf, `topk(k, largest=False)` — in the same process, at N = Q = 4096 and at N = 65536, Q = 4096, for S = 8 and 32, k = 5, split 0 and 1.

    python profiles/knn_microbench.py [--reps 10] [--points 4096x4096,65536x4096] [--dims 8,32] [--k 5]

Timing: device events around `reps` back-to-back calls on one stream after 3 warm-up calls, the median of 5 such batches; no clock is
pinned, so the figures are at whatever clock the chip holds under this load.  The torch path's peak extra memory is
torch.cuda.max_memory_allocated over its calls less what was allocated before them (the [Q][N] float64 plane and topk's scratch).  torch's
cdist expands the square (a matrix product) for these sizes, so its distances differ from the contract's in the last bits and its
neighbours may differ where distances are nearly equal: `neighbours_equal_share` is the share of (query, slot) pairs on which the two
agree, reported, not asserted.  f64_peak_share counts 3 S flops per pair (a subtraction and a fused multiply-add per dimension) against the 78.6 Tflop/s vector float64 spec figure."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "robotics-rl-srl_amd"), REPO]
from srlhip import _lib  # noqa: E402

F64_PEAK = 78.6e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", default="4096x4096,65536x4096")
    ap.add_argument("--dims", default="8,32")
    ap.add_argument("--k", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    k = args.k
    for point in args.points.split(","):
        n, q = (int(v) for v in point.split("x"))
        for s in (int(v) for v in args.dims.split(",")):
            gen = torch.Generator(device=dev).manual_seed(n + s)
            x = torch.randn((n, s), dtype=torch.float64, device=dev, generator=gen)
            gt = torch.randn((n, 3), dtype=torch.float64, device=dev, generator=gen)
            queries = torch.sort(torch.randperm(n, device=dev, generator=gen)[:q])[0].to(torch.int32)
            idx = torch.empty((q, k), dtype=torch.int32, device=dev)
            dist = torch.empty((q, k), dtype=torch.float64, device=dev)
            err = torch.empty((q,), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            row = {"n": n, "q": q, "s": s, "k": k}
            for split in (0, 1):
                work = torch.empty(_lib.knn_workspace_bytes(n, s, k, q, split) // 8 + 1, dtype=torch.int64, device=dev)
                hip = lambda: _lib.knn(0, x.data_ptr(), False, n, s, queries.data_ptr(), q, k, gt.data_ptr(), 3, idx.data_ptr(),      # noqa: E731
                                       dist.data_ptr(), err.data_ptr(), work.data_ptr(), split=split, stream=stream)
                for _ in range(3):
                    hip()
                torch.cuda.synchronize()
                ms = timed(hip, args.reps if split == 0 else max(1, args.reps // 3))
                row["hip_ms_split%d" % split] = round(ms, 4)
                row["workspace_MB_split%d" % split] = round(_lib.knn_workspace_bytes(n, s, k, q, split) / 1e6, 2)
            row["f64_peak_share_split0"] = round(3.0 * s * n * q / (row["hip_ms_split0"] * 1e-3) / F64_PEAK, 4)
            ql = queries.long()
            rows = torch.arange(q, device=dev)

            def ref():
                d = torch.cdist(x[ql], x)
                d[rows, ql] = float("inf")
                return torch.topk(d, k, dim=1, largest=False)

            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            for _ in range(2):
                got = ref()
            torch.cuda.synchronize()
            extra = torch.cuda.max_memory_allocated(dev) - base
            row["neighbours_equal_share"] = round(float((got.indices.to(torch.int32) == idx).double().mean()), 6)
            del got
            row["torch_ms"] = round(timed(ref, max(1, args.reps // 3)), 4)
            row["torch_peak_extra_MB"] = round(extra / 1e6, 1)
            row["speedup"] = round(row["torch_ms"] / row["hip_ms_split0"], 2)
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
