"""What --fused-returns changes: one ARS evaluation and one CMA-ES generation, reset() included, through the planes path
(srlhip_rollout_policy / srlhip_rollout_mlp_policy + the torch reductions over the [T][N] planes) and through the summary path
(srlhip_rollout_policy_summary), MobileRobotGymEnv-v0 and KukaButtonGymEnv-v0, 4096 envs (2048 ARS directions / 4096 CMA-ES members),
T = the episode limit + 1 (252 / 1002: what --fused-rollout launches), deterministic discrete actions.

    ars_planes / ars_summary   reset + ARSModel.evaluate_fused (--algo-type v1: no normalisation), the live-row count read on the host
    cma_planes / cma_summary   reset + CMAESModel.evaluate_fused on CMA-ES's env stack (DeviceVecNormalize, training: the statistics
                               update is part of the generation), H = 100

Timing as policy_rollout_microbench.py's cma_leg: the host clock around a device synchronisation, the two paths alternating so that both
see the same neighbours on the machine, median of --reps after --warmup; min and max are printed too.  One JSON line per leg.

--kuka-planes adds the PLANE calls of the four Kuka policy kernels on their own (they carry the summary path's run-time test and
accumulators): srlhip_rollout_policy / _sampled / srlhip_rollout_mlp_policy / _sampled on KukaButton, --envs envs, --kuka-steps steps,
HIP events on the handle's stream, every repetition from reset().
--planes-only runs the planes legs alone: the form that also runs on a build without the summary entry point (the figures of the
commit before it are taken this way, same machine, same session).

    python profiles/policy_returns_microbench.py [--envs 4096] [--reps 15] [--warmup 3] [--kuka-planes] [--planes-only]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from rl_baselines.evolution_strategies.ars import ARSModel  # noqa: E402
from rl_baselines.evolution_strategies.cma_es import BatchedMLP, CMAESModel  # noqa: E402
from srlhip.device_env import DeviceVecEnv  # noqa: E402

WORKLOADS = (("MobileRobotGymEnv-v0", 252), ("KukaButtonGymEnv-v0", 1002))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kuka-steps", type=int, default=256)
    ap.add_argument("--kuka-planes", action="store_true")
    ap.add_argument("--planes-only", action="store_true")
    a = ap.parse_args()
    assert a.envs % 2 == 0
    for env_id, T in WORKLOADS:
        ars_leg(a, env_id, T)
        cma_leg(a, env_id, T)
    if a.kuka_planes:
        kuka_plane_leg(a)


def alternate(a, legs, extra):
    """legs: [(name, fn)] timed in turn, a.warmup + a.reps rounds; one JSON line per leg"""
    ms = {name: [] for name, _ in legs}
    for i in range(a.warmup + a.reps):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    med = {}
    for name, _ in legs:
        med[name] = statistics.median(ms[name])
        print(json.dumps(dict(extra, leg=name, ms_median=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]), reps=a.reps)), flush=True)
    return med


def ars_leg(a, env_id, T):
    n = a.envs
    env = DeviceVecEnv(env_id, n, seed=0, rng_mode="philox")
    dev = env.device
    D, A = env.h.obs_dim, env.h.num_actions
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    delta = torch.randn((n // 2, D, A), dtype=torch.float64, device=dev, generator=gen)
    M = torch.zeros((D, A), dtype=torch.float64, device=dev)
    model = ARSModel()
    model.exploration_noise, model.deterministic, model.continuous_actions = 1.0, True, False

    def evaluation(returns):
        def fn():
            model.fused_returns = returns
            env.reset()
            model.evaluate_fused(env, M, delta, T)
        return fn

    legs = [("ars_planes", evaluation(False))] + ([] if a.planes_only else [("ars_summary", evaluation(True))])
    with torch.cuda.stream(env.torch_stream):
        med = alternate(a, legs, {"env": env_id, "directions": n // 2, "steps": T})
    if "ars_summary" in med:
        print(json.dumps({"env": env_id, "leg": "ars_planes_over_summary", "ratio": med["ars_planes"] / med["ars_summary"]}), flush=True)
    env.close()


def cma_leg(a, env_id, T, H=100):
    P = a.envs
    env = CMAESModel.makeEnv(types.SimpleNamespace(env=env_id, num_cpu=P, seed=0, srl_model="ground_truth", num_stack=1))
    dev = env.device
    model = CMAESModel()
    model.policy = BatchedMLP(env.observation_space.shape[0], env.action_space.n, H)
    model.deterministic, model.continuous_actions = True, False
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    population = 0.14 * torch.randn((P, model.policy.n_params), dtype=torch.float64, device=dev, generator=gen)

    def generation(returns):
        def fn():
            model.fused_returns = returns
            env.reset()
            model.evaluate_fused(env, population, T)
        return fn

    legs = [("cma_planes", generation(False))] + ([] if a.planes_only else [("cma_summary", generation(True))])
    with torch.cuda.stream(env.torch_stream):
        med = alternate(a, legs, {"env": env_id, "members": P, "steps": T, "hidden": H})
    if "cma_summary" in med:
        print(json.dumps({"env": env_id, "leg": "cma_planes_over_summary", "ratio": med["cma_planes"] / med["cma_summary"]}), flush=True)
    env.close()


def kuka_plane_leg(a, H=100):
    n, T = a.envs, a.kuka_steps
    env = DeviceVecEnv("KukaButtonGymEnv-v0", n, seed=0, rng_mode="philox")
    dev, h = env.device, env.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    W = torch.randn((n, 3, 6), dtype=torch.float64, device=dev, generator=gen)
    P = (0.5 * torch.randn((n, h.mlp_param_count(H)), dtype=torch.float64, device=dev, generator=gen)).to(torch.float32).contiguous()
    planes = (torch.empty((T, n, 3), dtype=torch.float32, device=dev), torch.empty((T, n), dtype=torch.float32, device=dev),
              torch.empty((T, n), dtype=torch.uint8, device=dev), torch.empty((T, n), dtype=torch.int32, device=dev))
    ptrs = tuple(t.data_ptr() for t in planes)
    legs = (("kuka_plane_linear", lambda: h.rollout_policy(T, W.data_ptr(), True, True, out=ptrs)),
            ("kuka_plane_linear_sampled", lambda: h.rollout_policy(T, W.data_ptr(), True, True, out=ptrs, sample=True)),
            ("kuka_plane_mlp", lambda: h.rollout_mlp_policy(T, P.data_ptr(), H, True, True, out=ptrs)),
            ("kuka_plane_mlp_sampled", lambda: h.rollout_mlp_policy(T, P.data_ptr(), H, True, True, out=ptrs, sample=True)))
    with torch.cuda.stream(env.torch_stream):
        for name, fn in legs:
            ms = []
            for i in range(a.warmup + a.reps):
                env.reset()
                h.timing_begin()
                fn()
                t = h.timing_end()
                if i >= a.warmup:
                    ms.append(t)
            print(json.dumps({"env": "KukaButtonGymEnv-v0", "leg": name, "envs": n, "steps": T, "ms_median": statistics.median(ms), "ms_min": min(ms),
                              "ms_max": max(ms), "us_per_step": 1e3 * statistics.median(ms) / T, "reps": a.reps}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
