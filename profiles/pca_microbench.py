"""srlhip_pca_forward (csrc/pca_project.hip) against the torch formulation SRLPCA keeps as backend="torch" — `images.to(float64)` followed
by addmm (rocBLAS dgemm) — in the same process, at 4096 frames of 64x64x3 and of 224x224x3, S = 32 and S = 5, float64 states.

    python profiles/pca_microbench.py [--reps 20] [--points 4096x64,4096x224] [--dims 32,5]

Timing: device events around `reps` back-to-back calls on one stream after 3 warm-up calls, the median of 5 such batches.  The torch
path's peak extra memory is torch.cuda.max_memory_allocated over its calls less what was allocated before them."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "robotics-rl-srl_amd"), REPO]
from srlhip import _lib  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", default="4096x64,4096x224")
    ap.add_argument("--dims", default="32,5")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for point in args.points.split(","):
        n, side = (int(v) for v in point.split("x"))
        F = side * side * 3
        frames = torch.randint(0, 256, (n, F), dtype=torch.uint8, device=dev)
        for S in (int(v) for v in args.dims.split(",")):
            rng = np.random.RandomState(S)
            q, _ = np.linalg.qr(rng.standard_normal((F, S)))
            w = q / np.sqrt(rng.uniform(0.5, 400.0, size=S))[None, :]
            b = -((128.0 + 20.0 * rng.standard_normal(F)) @ w)
            proj = _lib.PcaProjector(0, w, b)
            out = torch.empty((n, S), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            hip = lambda: proj.forward(frames.data_ptr(), n, out.data_ptr(), stream=stream)      # noqa: E731
            for _ in range(3):
                hip()
            torch.cuda.synchronize()
            hip_ms = timed(hip, args.reps)
            wd, bd = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
            ref = lambda: torch.addmm(bd, frames.to(torch.float64), wd)                          # noqa: E731
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            for _ in range(3):
                got = ref()
            torch.cuda.synchronize()
            extra = torch.cuda.max_memory_allocated(dev) - base
            torch_ms = timed(ref, args.reps)
            err = float((got - out).abs().max())
            print(json.dumps({"n": n, "side": side, "F": F, "S": S, "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
                              "speedup": round(torch_ms / hip_ms, 2), "torch_peak_extra_MB": round(extra / 1e6, 1),
                              "hip_gflops_f64": round(2.0 * n * F * S / hip_ms / 1e6, 1), "max_abs_diff": err}), flush=True)
            proj.close()
            del got, wd, bd
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
