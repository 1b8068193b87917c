"""One training step of the linear SRL encoder (csrc/linear_srl.hip: srlhip_linear_srl_forward + srlhip_linear_srl_step) against the
"torch" backend's step of the same arithmetic — a float64 copy of the frames normalised per channel, addmm for the states, the matmul
xn^T G for the gradient, torch.optim.Adam on V — in the same process, at batch 256, S = 32, for 64 x 64 x 3 and 224 x 224 x 3 frames, and
at a small shape (8 x 8 x 3, batch 16, S = 4) where launch overhead is everything.  G is a fixed tensor on both sides: the loss heads are
the same torch code for both and are left out.

    python profiles/linear_srl_microbench.py [--reps 20] [--shapes 64x64x3:256:32,224x224x3:256:32,8x8x3:16:4]

Timing: device events around `reps` back-to-back steps on one stream after 3 warm-up steps, the median of 5 such batches; no clock is
pinned, so the figures are at whatever clock the chip holds under this load.  Peak extra memory is torch.cuda.max_memory_allocated over
the steps less what was allocated before them (hip: the states and the forward's workspace; torch: the float64 frames, the [F][S]
gradient and Adam's temporaries).  step_bytes_min = 6 F S 8 + n F is what the step kernel must move (V, m, v read and written once, the
frames read once); step_bytes_model adds what this kernel moves on top by construction (the frames once per column group, G once per
workgroup); step_GBps is step_bytes_min over the step kernel's own time."""
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


def peak_extra(fn, dev):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="64x64x3:256:32,224x224x3:256:32,8x8x3:16:4")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for spec in args.shapes.split(","):
        shape, n, S = spec.split(":")
        H, W, C = (int(v) for v in shape.split("x"))
        n, S, F = int(n), int(S), H * W * C
        gen = torch.Generator(device=dev).manual_seed(F + S)
        x = torch.randint(0, 256, (n, F), dtype=torch.uint8, device=dev, generator=gen)
        G = torch.randn((n, S), dtype=torch.float64, device=dev, generator=gen) / n
        V0 = torch.randn((F, S), dtype=torch.float64, device=dev, generator=gen) / np.sqrt(F)
        c = torch.zeros((S,), dtype=torch.float64, device=dev)
        scale, offset = _lib.linear_srl_tables(C)
        V, m, v = V0.clone(), torch.zeros_like(V0), torch.zeros_like(V0)
        work = torch.empty((_lib.linear_srl_workspace_bytes(F, S, n) // 8,), dtype=torch.float64, device=dev)
        adam = _lib.adam_at(10)

        def hip_forward():
            states = torch.empty((n, S), dtype=torch.float64, device=dev)
            _lib.linear_srl_forward(0, x.data_ptr(), n, F, S, scale, offset, V.data_ptr(), c.data_ptr(), states.data_ptr(), work.data_ptr(), stream=stream)
            return states

        def hip_step():
            _lib.linear_srl_step(0, x.data_ptr(), n, F, S, scale, offset, G.data_ptr(), V.data_ptr(), m.data_ptr(), v.data_ptr(), adam, stream=stream)

        def hip_both():
            hip_forward()
            hip_step()

        ch = torch.arange(F, device=dev) % C
        scale_f, offset_f = torch.from_numpy(scale).to(dev)[ch], torch.from_numpy(offset).to(dev)[ch]
        Vp = torch.nn.Parameter(V0.clone())
        opt = torch.optim.Adam([Vp], lr=1e-3)

        def torch_both():
            opt.zero_grad(set_to_none=True)
            states = torch.addmm(c, x.to(torch.float64) * scale_f - offset_f, Vp)
            states.backward(G)
            opt.step()

        row = {"frame": shape, "n": n, "S": S, "F": F}
        for fn in (hip_both, torch_both):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        row["hip_forward_ms"] = round(timed(hip_forward, args.reps), 4)
        row["hip_step_ms"] = round(timed(hip_step, args.reps), 4)
        row["hip_ms"] = round(timed(hip_both, args.reps), 4)
        row["torch_ms"] = round(timed(torch_both, max(1, args.reps // 2)), 4)
        row["speedup"] = round(row["torch_ms"] / row["hip_ms"], 2)
        row["hip_peak_extra_MB"] = round((peak_extra(hip_both, dev) + work.numel() * 8) / 1e6, 2)
        row["torch_peak_extra_MB"] = round(peak_extra(torch_both, dev) / 1e6, 2)
        groups, blocks = -(-S // (8 if S <= 8 else 16 if S <= 16 else 32)), -(-F // 128)
        row["step_bytes_min_MB"] = round((6 * F * S * 8 + n * F) / 1e6, 2)
        row["step_bytes_model_MB"] = round((6 * F * S * 8 + groups * n * F + blocks * n * S * 8) / 1e6, 2)
        row["step_GBps"] = round((6 * F * S * 8 + n * F) / (row["hip_step_ms"] * 1e-3) / 1e9, 1)
        print(json.dumps(row), flush=True)
        del V, m, v, Vp, opt, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
