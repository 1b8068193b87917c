"""The linear policy's sampled forms against what they replace, 4096 envs (an ARS population of 2048), one device.  One JSON line per leg.

    (a) rollout   srlhip_rollout_policy_sampled against srlhip_rollout_policy on the same handle and weights, MobileRobot T = 252 and
                  KukaButton T = 1002 (the episode limit + 1: what ARS --fused-rollout launches), freeze_after_done, HIP events on the
                  handle's stream; every repetition starts from reset().
    (b) ars       one ARS evaluation: reset + ARSModel.evaluate_fused with sampling (--fused-rollout --fused-sampling) against reset + the
                  per-step loop of ARSModel.train — batched_actions / pixel_actions with torch.softmax + torch.multinomial + torch.where,
                  env.step, a done.all() read every 16 steps: the only way to run the default action selection without this entry point,
                  and code this change does not touch.  On ground truth (DeviceVecEnv), on 64 x 64 pixels with --pixel-policy
                  (RawPixelVecEnv) and on a learned state (PixelStateVecEnv, 64 x 64 frames, state_dim 3).  Wall clock around a device
                  synchronisation, the two alternating.
    (c) plane     srlhip_sample_actions alone against the torch.softmax + torch.multinomial + torch.where triple it replaces, A = 6,
                  20 calls per timing, alternating.

Medians of --reps repetitions after --warmup.

    python profiles/policy_sample_microbench.py [--envs 4096] [--reps 20] [--warmup 3] [--legs rollout,ars,plane]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from rl_baselines.evolution_strategies.ars import ARSModel  # noqa: E402
from srlhip.device_env import DeviceVecEnv  # noqa: E402


def emit(out):
    print(json.dumps(out), flush=True)


def rollout_leg(a, env_id, T, rng="philox"):
    n = a.envs
    env = DeviceVecEnv(env_id, n, seed=0, rng_mode=rng)
    dev, h = env.device, env.h
    D, A = h.obs_dim, h.num_actions
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    W = torch.randn((n, D, A), dtype=torch.float64, device=dev, generator=gen).contiguous()
    planes = (torch.empty((T, n, D), dtype=torch.float32, device=dev), torch.empty((T, n), dtype=torch.float32, device=dev),
              torch.empty((T, n), dtype=torch.uint8, device=dev), torch.empty((T, n), dtype=torch.int32, device=dev))
    ptrs = tuple(t.data_ptr() for t in planes)
    legs = (("deterministic", lambda: h.rollout_policy(T, W.data_ptr(), True, True, out=ptrs)),
            ("sampled", lambda: h.rollout_policy(T, W.data_ptr(), True, True, out=ptrs, sample=True)))
    out = {"leg": "rollout", "env": env_id, "rng": rng, "envs": n, "steps": T, "reps": a.reps, "freeze_after_done": True}
    ms = {name: [] for name, _ in legs}
    with torch.cuda.stream(env.torch_stream):
        for i in range(a.warmup + a.reps):
            for name, fn in legs:                          # alternating: both see the same neighbours on the machine
                env.reset()
                h.timing_begin()
                fn()
                t = h.timing_end()
                if i >= a.warmup:
                    ms[name].append(t)
    for name, _ in legs:
        out[name + "_ms"] = statistics.median(ms[name])
        out[name + "_min_max_ms"] = [min(ms[name]), max(ms[name])]
    out["sampled_over_deterministic"] = out["sampled_ms"] / out["deterministic_ms"]
    env.close()
    emit(out)


def ars_leg(a, kind):
    """one evaluation of P = envs / 2 directions, MobileRobotGymEnv-v0, T = 252"""
    import types
    P, T, noise = a.envs // 2, 252, 0.02
    args = types.SimpleNamespace(env="MobileRobotGymEnv-v0", num_cpu=2 * P, seed=0, num_stack=1, algo_type="v1", img_shape=(3, 64, 64),
                                 srl_model={"ground_truth": "ground_truth", "pixels": "raw_pixels", "learned": "autoencoder"}[kind],
                                 pixel_policy=kind == "pixels", state_dim=3)
    torch.manual_seed(0)
    env = ARSModel.makeEnv(args)
    dev = env.device
    pixels = kind == "pixels"
    D, A = int(torch.tensor(env.observation_space.shape).prod()), env.action_space.n
    model = ARSModel()
    model.exploration_noise, model.deterministic, model.continuous_actions = noise, False, False
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    M = torch.zeros((D, A), dtype=torch.float64, device=dev)
    delta = torch.randn((P, D, A), dtype=torch.float64, device=dev, generator=gen)

    def per_step():
        obs = env.reset()
        done = torch.zeros(2 * P, dtype=torch.bool, device=dev)
        r = torch.zeros((P, 2), dtype=torch.float64, device=dev)
        if pixels:
            frozen = torch.zeros(2 * P, dtype=torch.uint8, device=dev)
            scores = torch.zeros((2 * P, A), dtype=torch.float64, device=dev)
        k = 0
        while True:
            if pixels:
                actions = ARSModel.pixel_actions(env, M, delta, noise, done, frozen, scores, False, False, gen)
            else:
                actions = ARSModel.batched_actions(obs, M, delta, noise, ~done, False, False, gen, False)
            obs, reward, new_done = env.step(actions)
            done = done | (new_done != 0)
            r += (reward.to(torch.float64) * (~done).to(torch.float64)).view(P, 2)
            k += 1
            if k % 16 == 0 and bool(done.all()):
                return k

    def fused():
        env.reset()
        model.evaluate_fused(env, M, delta, T)
        return T

    out = {"leg": "ars", "obs": kind, "env": args.env, "population": P, "envs": 2 * P, "steps": T, "reps": a.reps}
    ms = {"per_step": [], "fused": []}
    with torch.cuda.stream(env.torch_stream):
        for i in range(a.warmup + a.reps):
            for name, fn in (("per_step", per_step), ("fused", fused)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[name + "_env_steps"] = fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
    for name in ms:
        out[name + "_ms"] = statistics.median(ms[name])
        out[name + "_min_max_ms"] = [min(ms[name]), max(ms[name])]
    out["per_step_over_fused"] = out["per_step_ms"] / out["fused_ms"]
    env.close()
    emit(out)


def plane_leg(a, A=6, K=20):
    n = a.envs
    env = DeviceVecEnv("KukaButtonGymEnv-v0", n, seed=0, rng_mode="philox")
    dev, h = env.device, env.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    scores = torch.randn((n, A), dtype=torch.float64, device=dev, generator=gen)
    done = torch.zeros(n, dtype=torch.bool, device=dev)
    frozen = torch.zeros(n, dtype=torch.uint8, device=dev)
    act = torch.zeros(n, dtype=torch.int32, device=dev)

    def kernel():
        for _ in range(K):
            h.sample_actions(scores.data_ptr(), act.data_ptr(), frozen=frozen.data_ptr())

    def triple():
        for _ in range(K):
            x = torch.multinomial(torch.softmax(scores, dim=1), 1, generator=gen).squeeze(1)
            torch.where(~done, x, torch.full_like(x, -1)).to(torch.int32).contiguous()

    ms = {"sample_actions": [], "torch_triple": []}
    with torch.cuda.stream(env.torch_stream):
        for i in range(a.warmup + a.reps):
            for name, fn in (("sample_actions", kernel), ("torch_triple", triple)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[name].append(1e6 * (time.perf_counter() - t0) / K)
    out = {"leg": "plane", "envs": n, "A": A, "calls_per_timing": K, "reps": a.reps}
    for name in ms:
        out[name + "_us"] = statistics.median(ms[name])
        out[name + "_min_max_us"] = [min(ms[name]), max(ms[name])]
    out["torch_over_kernel"] = out["torch_triple_us"] / out["sample_actions_us"]
    env.close()
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="rollout,ars,plane")
    a = ap.parse_args()
    assert a.envs % 2 == 0
    legs = a.legs.split(",")
    if "rollout" in legs:
        rollout_leg(a, "MobileRobotGymEnv-v0", 252)
        rollout_leg(a, "KukaButtonGymEnv-v0", 1002)
    if "plane" in legs:
        plane_leg(a)
    if "ars" in legs:
        for kind in ("ground_truth", "pixels", "learned"):
            ars_leg(a, kind)


if __name__ == "__main__":
    main()
