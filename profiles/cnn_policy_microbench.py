"""srlhip_cnn_policy_act at 4096 envs, 64x64 and 224x224 (C = 3, A = 6, per-env parameters), against its two floors — the frame bytes
at HBM rate and the fp32 work at the vector peak — and against the same forward written with torch on the device: one grouped
convolution per layer (groups = N, the only way torch expresses N different networks) with per-group statistics.

    python profiles/cnn_policy_microbench.py [--envs 4096] [--reps 20]

Timing: device events around `reps` back-to-back launches on the handle's stream after a warm-up, the median of 5 such batches; the
frames are random bytes, rewritten once (the result does not depend on them)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "robotics-rl-srl_amd"), REPO]
from srlhip.pixel_env import RawPixelVecEnv  # noqa: E402

HBM_BYTES_PER_S, FP32_FLOPS = 8.0e12, 157.3e12      # MI355X: peak HBM3E bandwidth, peak vector fp32


def timed(fn, stream, reps):
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            for _ in range(reps):
                fn()
            b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def torch_forward(frames, blocks, n):
    """frames uint8 [n][H][W][C], blocks: per-env parameter blocks [n][...] -> scores [n][A]: conv2d(groups=n) on a [1][n C][H][W] tensor"""
    x = (frames.permute(0, 3, 1, 2).to(torch.float32) / 255.0).reshape(1, -1, frames.shape[1], frames.shape[2])
    for l, pad in enumerate((2, 1, 1)):
        w, g, b = blocks[3 * l:3 * l + 3]
        x = F.conv2d(x, w.reshape((-1,) + tuple(w.shape[2:])), stride=2, padding=pad, groups=n)
        x = x.reshape(n, w.shape[1], x.shape[2], x.shape[3])
        mean, var = x.mean(dim=(2, 3), keepdim=True), x.var(dim=(2, 3), unbiased=False, keepdim=True)
        x = F.max_pool2d(torch.relu((x - mean) * torch.rsqrt(var + 1e-5) * g.unsqueeze(-1).unsqueeze(-1) + b.unsqueeze(-1).unsqueeze(-1)), 2)
        x = x.reshape(1, -1, x.shape[2], x.shape[3])
    x = x.reshape(n, -1)
    return torch.bmm(blocks[9], x.unsqueeze(-1)).squeeze(-1) + blocks[10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n = args.envs
    for side in (64, 224):
        env = RawPixelVecEnv("KukaButtonGymEnv-v0", n, seed=1, img_shape=(side, side))
        P, A = env.cnn_param_count(), env.h.num_actions
        gen = torch.Generator(device="cuda").manual_seed(side)
        params = (0.1 * torch.randn((n, P), device="cuda", generator=gen)).contiguous()
        env.images.copy_(torch.randint(0, 256, env.images.shape, device="cuda", generator=gen, dtype=torch.uint8))
        torch.cuda.synchronize()
        call = lambda: env.h.cnn_policy_act(env.images.data_ptr(), env.actions.data_ptr(), params.data_ptr(), per_env=True)      # noqa: E731
        for _ in range(3):
            call()
        env.h.sync()
        ms = timed(call, env.torch_stream, args.reps)
        shapes = [(8, 3, 5, 5), (8,), (8,), (16, 8, 3, 3), (16,), (16,), (32, 16, 3, 3), (32,), (32,)]
        f_in = (P - sum(int(np.prod(s)) for s in shapes) - A) // A
        shapes += [(A, f_in), (A,)]
        blocks, o = [], 0
        for s in shapes:
            k = int(np.prod(s))
            blocks.append(params[:, o:o + k].reshape((n,) + s).contiguous())
            o += k
        torch_ms = None
        try:
            for _ in range(2):
                torch_forward(env.images, blocks, n)
            torch.cuda.synchronize()
            torch_ms = timed(lambda: torch_forward(env.images, blocks, n), torch.cuda.current_stream(), max(1, args.reps // 10))
        except RuntimeError as e:                      # the grouped formulation can run out of memory at 224 x 224
            print("torch formulation failed at {0} x {0}: {1}".format(side, str(e).splitlines()[0]))
        c1 = (side - 1) // 2 + 1
        p1 = c1 // 2
        c2 = (p1 - 1) // 2 + 1
        p2 = c2 // 2
        c3 = (p2 - 1) // 2 + 1
        flops = 2.0 * (c1 * c1 * 8 * 75 + c2 * c2 * 16 * 72 + c3 * c3 * 32 * 144)
        bytes_ = side * side * 3 + 4.0 * P
        print(json.dumps({"side": side, "envs": n, "kernel_ms": round(ms, 4), "torch_grouped_ms": None if torch_ms is None else round(torch_ms, 3),
                          "floor_bytes_ms": round(1e3 * n * bytes_ / HBM_BYTES_PER_S, 4), "floor_fp32_ms": round(1e3 * n * flops / FP32_FLOPS, 4),
                          "mflop_per_frame": round(flops / 1e6, 2), "frames_per_s": round(n / ms * 1e3)}))
        env.close()


if __name__ == "__main__":
    main()
