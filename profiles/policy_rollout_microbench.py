"""Fused policy rollout against its two neighbours, KukaButtonGymEnv-v0 and MobileRobotGymEnv-v0, 4096 envs, one device, HIP events on
the handle's stream.  The script sets SRLHIP_KUKA_SPEC=0 itself (the library reads it once per process) so that the Kuka GIVEN rollout
is the generic instantiation, like the policy one:

    given     srlhip_rollout with a caller-supplied [T][N] action plane (the baseline: never the policy kernel itself)
    policy    srlhip_rollout_policy over the same T, per-env N(0, 1) weights
    per_step  the ARS inner loop: ARSModel.batched_actions + DeviceVecEnv.step, T times

Each figure is the median of --reps repetitions after --warmup; every repetition starts from reset() so all three run the same
episodes' lengths.  Prints one JSON line per env.  Elapsed time on the stream, not device busy time: the per-step leg includes
its launch and host gaps.

    python profiles/policy_rollout_microbench.py [--envs 4096] [--steps 252] [--reps 15] [--warmup 3]

--mlp times the MLP policy (srlhip_rollout_mlp_policy, H = 100, per-env N(0, 0.5) float32 parameters) instead, at --envs and at 20
envs (the reference's default CMA-ES population):

    mlp       srlhip_rollout_mlp_policy over T steps
    given     srlhip_rollout with the action plane the MLP rollout recorded
    per_step  the CMA-ES inner loop (cma_es.py, unchanged by the fused path): BatchedMLP.forward in float64 + argmax + where +
              DeviceVecEnv.step, T times

--sampled times the sampled MLP rollout (srlhip_rollout_mlp_policy_sampled) beside the deterministic one from the same build, KukaButton
and MobileRobot, --envs envs, the episode limit + 1 as T (1002 / 252: what CMA-ES --fused-rollout launches), H = 100, and one CMA-ES
generation on the per-step path with softmax sampling against evaluate_fused with sampling (wall clock around a device synchronisation,
reset included, at --envs and at 20 members):

    mlp       srlhip_rollout_mlp_policy over T steps (--deterministic-only: this leg alone, e.g. on a build without the sampled entry point)
    sampled   srlhip_rollout_mlp_policy_sampled over T steps
    cma_per_step / cma_fused   one generation: reset + the per-step loop of CMAESModel.train (BatchedMLP.forward, softmax,
              torch.multinomial, DeviceVecEnv.step until every member is done, checked every 16 steps) / reset + evaluate_fused
    pixel (--pixel)   learned SRL states (KukaButton, 64x64 frames, state_dim 200, hidden 100; 4096 and 20 envs), T steps each way,
              alternating: pixel_fused = PixelStateVecEnv.rollout_mlp_policy (T x (srlhip_policy_act, step + rasteriser, encoder), enqueue
              only) / pixel_per_step = PixelStateVecEnv.step + BatchedMLP.forward + argmax in torch on the same stream with a done.all()
              read every 16 steps, as cma_es.py does.  Then policy_act alone at 4096 x (D 200, H 100) next to a device-to-device copy
              of the same parameter bytes, alternating."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

os.environ["SRLHIP_KUKA_SPEC"] = "0"      # before the library's first Kuka launch reads it: the GIVEN baseline must be the generic kernel

import torch  # noqa: E402

from rl_baselines.evolution_strategies.ars import ARSModel  # noqa: E402
from srlhip.device_env import DeviceVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=252)
    ap.add_argument("--kuka-steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mlp", action="store_true")
    ap.add_argument("--sampled", action="store_true")
    ap.add_argument("--deterministic-only", action="store_true")
    ap.add_argument("--no-cma", action="store_true")
    ap.add_argument("--pixel", action="store_true")
    ap.add_argument("--pixel-steps", type=int, default=64)
    a = ap.parse_args()
    assert a.envs % 2 == 0
    if a.pixel:
        for n in (a.envs, 20):
            pixel_leg(a, n, a.pixel_steps)
        act_alone_leg(a, a.envs)
        return
    if a.sampled:
        sampled_leg(a, "MobileRobotGymEnv-v0", 252, 2, 4, "philox", a.envs)
        sampled_leg(a, "KukaButtonGymEnv-v0", 1002, 3, 6, "philox", a.envs)
        if not a.deterministic_only and not a.no_cma:
            for n in (a.envs, 20):
                cma_leg(a, "MobileRobotGymEnv-v0", 252, n)
                cma_leg(a, "KukaButtonGymEnv-v0", 1002, n)
        return
    if a.mlp:
        for n in (a.envs, 20):
            mlp_leg(a, "KukaButtonGymEnv-v0", a.kuka_steps, 3, 6, "philox", n)
            mlp_leg(a, "MobileRobotGymEnv-v0", a.steps, 2, 4, "philox", n)
            mlp_leg(a, "MobileRobotGymEnv-v0", a.steps, 2, 4, "mt19937", n)
        return
    leg(a, "KukaButtonGymEnv-v0", a.kuka_steps, 3, 6, "philox")
    leg(a, "MobileRobotGymEnv-v0", a.steps, 2, 4, "philox")
    # MT19937: the GIVEN rollout is then the sequential mobile_rollout_k too (Philox takes the episode-parallel kernel) — like for like
    leg(a, "MobileRobotGymEnv-v0", a.steps, 2, 4, "mt19937")


def leg(a, env_id, T, D, A, rng):
    n = a.envs
    env = DeviceVecEnv(env_id, n, seed=0, rng_mode=rng)
    dev, h = env.device, env.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    P = n // 2
    delta = torch.randn((P, D, A), dtype=torch.float64, device=dev, generator=gen)
    M = torch.zeros((D, A), dtype=torch.float64, device=dev)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device=dev).view(1, 2, 1, 1)
    W = (M + sign * delta.unsqueeze(1)).reshape(n, D, A).contiguous()
    given = torch.randint(0, A, (T, n), dtype=torch.int32, device=dev, generator=gen)
    planes = (torch.empty((T, n, D), dtype=torch.float32, device=dev), torch.empty((T, n), dtype=torch.float32, device=dev),
              torch.empty((T, n), dtype=torch.uint8, device=dev), torch.empty((T, n), dtype=torch.int32, device=dev))
    ptrs = tuple(t.data_ptr() for t in planes)
    active = torch.ones(n, dtype=torch.bool, device=dev)

    def run_given():
        h.rollout(T, given.data_ptr(), out=ptrs[:3] + (None,))

    def run_policy():
        h.rollout_policy(T, W.data_ptr(), True, False, out=ptrs)

    def run_per_step():
        obs = env.obs
        for _ in range(T):
            act = ARSModel.batched_actions(obs, M, delta, 1.0, active, False, True)
            obs, _, _ = env.step(act)

    out = {"env": env_id, "rng": rng, "envs": n, "steps": T, "reps": a.reps}
    with torch.cuda.stream(env.torch_stream):
        for name, fn in (("given", run_given), ("policy", run_policy), ("per_step", run_per_step)):
            ms = []
            for i in range(a.warmup + a.reps):
                env.reset()
                h.timing_begin()
                fn()
                t = h.timing_end()
                if i >= a.warmup:
                    ms.append(t)
            out[name + "_ms"] = statistics.median(ms)
            out[name + "_us_per_step"] = 1e3 * statistics.median(ms) / T
            out[name + "_min_max_ms"] = [min(ms), max(ms)]
    out["policy_over_given"] = out["policy_ms"] / out["given_ms"]
    out["per_step_over_policy"] = out["per_step_ms"] / out["policy_ms"]
    env.close()
    print(json.dumps(out))


def mlp_leg(a, env_id, T, D, A, rng, n, H=100):
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP
    env = DeviceVecEnv(env_id, n, seed=0, rng_mode=rng)
    dev, h = env.device, env.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    policy = BatchedMLP(D, A, H)
    pop = 0.5 * torch.randn((n, policy.n_params), dtype=torch.float64, device=dev, generator=gen)
    W = pop.to(torch.float32).contiguous()
    planes = (torch.empty((T, n, D), dtype=torch.float32, device=dev), torch.empty((T, n), dtype=torch.float32, device=dev),
              torch.empty((T, n), dtype=torch.uint8, device=dev), torch.empty((T, n), dtype=torch.int32, device=dev))
    ptrs = tuple(t.data_ptr() for t in planes)
    done = torch.zeros(n, dtype=torch.bool, device=dev)

    def run_mlp():
        h.rollout_mlp_policy(T, W.data_ptr(), H, True, False, out=ptrs)

    with torch.cuda.stream(env.torch_stream):
        env.reset()
        run_mlp()
        given = planes[3].clone()                       # the recorded action plane

    def run_given():
        h.rollout(T, given.data_ptr(), out=ptrs[:3] + (None,))

    def run_per_step():
        obs = env.obs
        for _ in range(T):
            act = torch.argmax(policy.forward(pop, obs), dim=1)
            act = torch.where(done, torch.full_like(act, -1), act).to(torch.int32).contiguous()
            obs, _, _ = env.step(act)

    out = {"env": env_id, "rng": rng, "envs": n, "steps": T, "hidden": H, "reps": a.reps}
    with torch.cuda.stream(env.torch_stream):
        for name, fn in (("given", run_given), ("mlp", run_mlp), ("per_step", run_per_step)):
            ms = []
            for i in range(a.warmup + a.reps):
                env.reset()
                h.timing_begin()
                fn()
                t = h.timing_end()
                if i >= a.warmup:
                    ms.append(t)
            out[name + "_ms"] = statistics.median(ms)
            out[name + "_us_per_step"] = 1e3 * statistics.median(ms) / T
            out[name + "_min_max_ms"] = [min(ms), max(ms)]
    out["mlp_over_given"] = out["mlp_ms"] / out["given_ms"]
    out["mlp_over_per_step"] = out["mlp_ms"] / out["per_step_ms"]
    env.close()
    print(json.dumps(out))


def sampled_leg(a, env_id, T, D, A, rng, n, H=100):
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP
    env = DeviceVecEnv(env_id, n, seed=0, rng_mode=rng)
    dev, h = env.device, env.h
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    W = (0.5 * torch.randn((n, BatchedMLP(D, A, H).n_params), dtype=torch.float64, device=dev, generator=gen)).to(torch.float32).contiguous()
    planes = (torch.empty((T, n, D), dtype=torch.float32, device=dev), torch.empty((T, n), dtype=torch.float32, device=dev),
              torch.empty((T, n), dtype=torch.uint8, device=dev), torch.empty((T, n), dtype=torch.int32, device=dev))
    ptrs = tuple(t.data_ptr() for t in planes)
    legs = [("mlp", lambda: h.rollout_mlp_policy(T, W.data_ptr(), H, True, True, out=ptrs))]
    if not a.deterministic_only:
        legs.append(("sampled", lambda: h.rollout_mlp_policy(T, W.data_ptr(), H, True, True, out=ptrs, sample=True)))
    out = {"env": env_id, "rng": rng, "envs": n, "steps": T, "hidden": H, "reps": a.reps, "freeze_after_done": True}
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
            out[name + "_ms"] = statistics.median(ms)
            out[name + "_us_per_step"] = 1e3 * statistics.median(ms) / T
            out[name + "_min_max_ms"] = [min(ms), max(ms)]
    if "sampled_ms" in out:
        out["sampled_over_mlp"] = out["sampled_ms"] / out["mlp_ms"]
    env.close()
    print(json.dumps(out), flush=True)


def cma_leg(a, env_id, T, P, H=100):
    import time
    import types
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP, CMAESModel
    env = CMAESModel.makeEnv(types.SimpleNamespace(env=env_id, num_cpu=P, seed=0, srl_model="ground_truth", num_stack=1))
    dev = env.device
    model = CMAESModel()
    model.policy = BatchedMLP(env.observation_space.shape[0], env.action_space.n, H)
    model.deterministic, model.continuous_actions = False, False
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    population = 0.14 * torch.randn((P, model.policy.n_params), dtype=torch.float64, device=dev, generator=gen)

    def per_step():
        obs = env.reset()
        done = torch.zeros(P, dtype=torch.bool, device=dev)
        r = torch.zeros(P, dtype=torch.float64, device=dev)
        k = 0
        while True:
            scores = model.policy.forward(population, obs)
            act = torch.multinomial(torch.softmax(scores, dim=1), 1, generator=gen).squeeze(1)
            act = torch.where(done, torch.full_like(act, -1), act).to(torch.int32).contiguous()
            obs, reward, new_done = env.step(act)
            done = done | (new_done != 0)
            r += reward.to(torch.float64) * (~done).to(torch.float64)
            k += 1
            if k % 16 == 0 and bool(done.all()):
                return k

    def fused():
        env.reset()
        model.evaluate_fused(env, population, T)
        return T

    out = {"env": env_id, "population": P, "steps": T, "hidden": H, "reps": a.reps}
    with torch.cuda.stream(env.torch_stream):
        for name, fn in (("cma_per_step", per_step), ("cma_fused", fused)):
            ms = []
            for i in range(1 + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[name + "_env_steps"] = fn()
                torch.cuda.synchronize()
                if i >= 1:
                    ms.append(1e3 * (time.perf_counter() - t0))
            out[name + "_ms"] = statistics.median(ms)
            out[name + "_min_max_ms"] = [min(ms), max(ms)]
    out["per_step_over_fused"] = out["cma_per_step_ms"] / out["cma_fused_ms"]
    env.close()
    print(json.dumps(out), flush=True)


def _timed(fn, sync):
    """one call of fn between two host clock reads, the device drained before and after"""
    import time
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def _report(name, n, T, ms, extra=None):
    ms = sorted(ms)
    out = {"leg": name, "envs": n, "steps": T, "ms_median": statistics.median(ms), "ms_min": ms[0], "ms_max": ms[-1], "reps": len(ms)}
    out["us_per_step"] = 1e3 * out["ms_median"] / T
    out["env_steps_per_s"] = n * T / (out["ms_median"] * 1e-3)
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return out


def pixel_leg(a, n, T, D=200, H=100):
    from rl_baselines.evolution_strategies.cma_es import BatchedMLP
    from srlhip.pixel_env import PixelStateVecEnv
    from state_representation.models import SRLNeuralNetwork
    torch.manual_seed(0)
    enc = SRLNeuralNetwork(D, cuda=True, img_shape=(64, 64))
    env = PixelStateVecEnv("KukaButtonGymEnv-v0", n, enc, seed=0, img_shape=(64, 64))
    A = env.h.num_actions
    mlp = BatchedMLP(D, A, H)
    params = (0.1 * torch.randn((n, mlp.n_params), device=env.device)).contiguous()
    sync = torch.cuda.synchronize

    def fused():
        with torch.cuda.stream(env.torch_stream):
            env.rollout_mlp_policy(T, params, H, freeze_after_done=True)

    def per_step():
        with torch.cuda.stream(env.torch_stream):
            done = torch.zeros(n, dtype=torch.bool, device=env.device)
            obs = env._current
            for k in range(1, T + 1):
                acts = torch.argmax(mlp.forward(params, obs), dim=1)
                actions = torch.where(done, torch.full_like(acts, -1), acts).to(torch.int32).contiguous()
                obs, _, new_done = env.step(actions)
                done = done | (new_done != 0)
                if k % 16 == 0:
                    bool(done.all())

    with torch.cuda.stream(env.torch_stream):
        env.reset()
    for _ in range(a.warmup):
        fused(); per_step()
    t_f, t_p = [], []
    for _ in range(a.reps):                                # alternating: both see the same neighbours on the machine
        t_f.append(_timed(fused, sync)); t_p.append(_timed(per_step, sync))
    f = _report("pixel_fused", n, T, t_f)
    p = _report("pixel_per_step", n, T, t_p)
    print(json.dumps({"leg": "pixel_ratio", "envs": n, "per_step_over_fused": p["ms_median"] / f["ms_median"]}), flush=True)
    env.close()


def act_alone_leg(a, n, D=200, H=100):
    from srlhip.pixel_env import PixelStateVecEnv
    from state_representation.models import SRLNeuralNetwork
    enc = SRLNeuralNetwork(D, cuda=True, img_shape=(64, 64))
    env = PixelStateVecEnv("KukaButtonGymEnv-v0", n, enc, seed=0, img_shape=(64, 64))
    P = env.mlp_param_count(H)
    params = (0.1 * torch.randn((n, P), device=env.device)).contiguous()
    twin = torch.empty_like(params)
    obs = torch.randn((n, D), device=env.device)
    act = torch.zeros((n,), dtype=torch.int32, device=env.device)
    K, nbytes = 20, params.numel() * 4
    sync = torch.cuda.synchronize

    def acts():
        for _ in range(K):
            env.h.policy_act(obs.data_ptr(), D, act.data_ptr(), params=params.data_ptr(), hidden=H)

    def copies():
        for _ in range(K):
            env.h.copy_async(twin.data_ptr(), params.data_ptr(), nbytes)

    for _ in range(a.warmup):
        acts(); copies()
    t_a, t_c = [], []
    for _ in range(a.reps):
        t_a.append(_timed(acts, sync) / K); t_c.append(_timed(copies, sync) / K)
    ma, mc = statistics.median(t_a), statistics.median(t_c)
    print(json.dumps({"leg": "policy_act_alone", "envs": n, "D": D, "H": H, "param_bytes": nbytes, "ms_median": ma, "ms_min": min(t_a),
                      "ms_max": max(t_a), "param_GB_per_s": nbytes / (ma * 1e-3) / 1e9, "d2d_copy_ms_median": mc, "d2d_copy_ms_min": min(t_c),
                      "d2d_copy_ms_max": max(t_c), "d2d_copy_read_GB_per_s": nbytes / (mc * 1e-3) / 1e9, "calls_per_timing": K,
                      "reps": a.reps}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
