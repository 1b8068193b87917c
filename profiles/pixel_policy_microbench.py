"""srlhip_pixel_policy_act (C = 3, A = 6, paired) at four points — N = 4096 and N = 20 envs, 64x64 and 224x224 frames — against the torch
formulation the per-step ARS path uses without it (ARSModel.batched_actions: W = M +- noise * delta as [P][2][D][A] float64, then a batched
matmul on the flattened float64 frames) and against a floor: a plain device copy of as many bytes as the kernel must read (delta, the
frames, M), timed in the same script.

    python profiles/pixel_policy_microbench.py [--reps 20] [--points 4096x64,4096x224,20x64,20x224]

Timing: device events around `reps` back-to-back launches on the handle's stream after 3 warm-up launches, the median of 5 such batches.
Where the torch formulation does not fit at N envs it is timed at the largest N (halved until it fits) and the line says so."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "robotics-rl-srl_amd"), REPO]
from rl_baselines.evolution_strategies.ars import ARSModel  # noqa: E402
from srlhip.pixel_env import RawPixelVecEnv  # noqa: E402


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


def torch_time(frames, M, delta, noise, reps):
    """batched_actions on the first 2 P envs, P halved until the [P][2][D][A] block fits -> (ms, envs timed)"""
    P = delta.shape[0]
    while P >= 1:
        try:
            obs, d = frames[:2 * P].reshape(2 * P, -1), delta[:P]
            active = torch.ones(2 * P, dtype=torch.bool, device=frames.device)
            fn = lambda: ARSModel.batched_actions(obs, M, d, noise, active, False, True)      # noqa: E731
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            return timed(fn, torch.cuda.current_stream(), reps), 2 * P
        except RuntimeError as e:
            if "out of memory" not in str(e).lower():
                raise
            torch.cuda.empty_cache()
            P //= 2
    return None, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", default="4096x64,4096x224,20x64,20x224")
    args = ap.parse_args()
    for point in args.points.split(","):
        n, side = (int(v) for v in point.split("x"))
        env = RawPixelVecEnv("KukaButtonGymEnv-v0", n, seed=1, img_shape=(side, side))
        A, D = env.h.num_actions, side * side * 3
        gen = torch.Generator(device="cuda").manual_seed(side + n)
        M = torch.randn((D, A), dtype=torch.float64, device="cuda", generator=gen)
        delta = torch.randn((n // 2, D, A), dtype=torch.float64, device="cuda", generator=gen)
        env.images.copy_(torch.randint(0, 256, env.images.shape, device="cuda", generator=gen, dtype=torch.uint8))
        torch.cuda.synchronize()
        call = lambda: env.h.pixel_policy_act(env.images.data_ptr(), env.actions.data_ptr(), M.data_ptr(), delta=delta.data_ptr(), noise=0.02)      # noqa: E731
        for _ in range(3):
            call()
        env.h.sync()
        ms = timed(call, env.torch_stream, args.reps)
        # the floor: one device copy of the bytes the kernel must read
        nbytes = delta.numel() * 8 + env.images.numel() + M.numel() * 8
        src = torch.empty(((nbytes + 15) // 16) * 2, dtype=torch.float64, device="cuda").normal_()
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        torch.cuda.synchronize()
        copy_ms = timed(lambda: dst.copy_(src), torch.cuda.current_stream(), args.reps)
        del src, dst
        torch.cuda.empty_cache()
        torch_ms, torch_envs = torch_time(env.images, M, delta, 0.02, max(2, args.reps // 4))
        # the same actions from both (deterministic; near ties aside the argmax agrees — reported, not asserted here: the tests hold the bits)
        print(json.dumps({"envs": n, "side": side, "kernel_ms": round(ms, 4), "copy_ms": round(copy_ms, 4), "kernel_over_copy": round(ms / copy_ms, 2),
                          "bytes_read": nbytes, "kernel_tb_per_s": round(nbytes / ms / 1e9, 3),
                          "torch_ms": None if torch_ms is None else round(torch_ms, 4), "torch_envs": torch_envs,
                          "torch_ms_scaled_to_envs": None if torch_ms is None else round(torch_ms * n / torch_envs, 4)}), flush=True)
        env.close()
        del M, delta
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
