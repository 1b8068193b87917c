#!/usr/bin/env python
"""bench.py — env-steps/sec of the MI355X-native vectorised env stepper.

Metric (BASELINE.json): env steps/sec (whole node), 4096 envs per GPU,
synthetic random-action rollouts (rl_baselines/random_agent.py:35-42).

One bench "step" = one srlhip_rollout() pass: every env of this rank's shard
advances `inner_steps` VecEnv steps (auto-reset inside, random-agent actions
drawn on the device, observation / reward / done planes streamed to HBM).
value = total env-steps of all ranks / max-over-ranks wall time.

A plain run sets up, warms up, times K steps and prints one JSON line.  --full adds
everything else this file measures: the CPU baselines, the secondary legs of the
default command (other workloads, sizes and the lumped model), the live rocprofv3
PMC passes and the pixel path's per-kernel timings.  --dump-outputs DIR writes what
the timed path returned in its last step as DIR/<name>.npy (float32 / float64; a
fixed, seeded sample of envs when the planes exceed 48 MB).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload kuka|mobile] [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(REPO, "robotics-rl-srl_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
FP64_VALU_PEAK_TFLOPS = 78.6   # MI355X FP64 vector peak (spec)
F16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16/bf16 MFMA peak
F32_MFMA_PEAK_TFLOPS = 157.3   # f32-in / f32-accumulate MFMA = the f32 vector rate
# algorithmic bytes per env-step
ALG_BYTES = {"mobile": 73, "kuka": 213, "kuka_pixels": 24900}
PUBLISHED_REFERENCE_FPS = 250.0   # /root/reference/README.md:9 (8 cores, with 224x224 rendering)
PROFILE_ROUND = 6                 # committed PMC summaries older than this round are NOT read back (profiles/rNN_*: the kernels they measured are gone)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="auto", choices=["auto", "kuka", "mobile", "kuka_pixels"])
    ap.add_argument("--envs-per-gpu", type=int, default=4096)
    ap.add_argument("--inner-steps", type=int, default=None)
    ap.add_argument("--img-size", type=int, default=64,
                    help="kuka_pixels: frame side (64 = BASELINE config 4, fused encoder; 224 = the reference's RENDER size, layered encoder)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--rng", default="philox", choices=["philox", "mt19937"])
    ap.add_argument("--kuka-model", default="full", choices=["full", "lumped"],
                    help="full = the 12-DoF arm + gripper tree of kuka_with_gripper2.sdf (library default); lumped = the rounds 1-2 approximation")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the short BASELINE config 2 (mobile) and config 4 (kuka_pixels) runs nested under \"secondary\"")
    ap.add_argument("--per-step", action="store_true",
                    help="time the per-step VecEnv API (HipVecEnv.step_async / step_wait: the path rl_baselines.train drives) instead of fused "
                         "rollouts; with --device-ids the ONE process shards the envs over those GPUs")
    ap.add_argument("--persistent", action="store_true", help="--per-step: persistent stepping (srlhip_set_persistent: a resident kernel, no launch per step); "
                    "the launching path's figure is reported beside it")
    ap.add_argument("--device-ids", default=None, help="--per-step: GPUs of the sharded HipVecEnv ('all' or e.g. 0,1,2,3; default: device 0)")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="roofline.traffic / issue_util from the committed profiles/ summaries only (no rocprofv3 --pmc child passes)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: CPU baselines, the secondary legs, live rocprofv3 --pmc "
                         "passes, the pixel path's per-kernel timings (--no-cpu-baseline / --no-secondary / --no-live-pmc trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup is not None and args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


DUMP_BUDGET_BYTES = 48 << 20     # --dump-outputs: at most this much in all (a seeded sample of envs beyond it)


def dump_outputs(out_dir, planes, n):
    """Write each plane of `planes` (name -> (torch tensor or ndarray, env axis)) as out_dir/<name>.npy: float64 stays float64,
    everything else becomes float32 (the integer planes are action indices and done flags, exact in float32).  When all planes
    together exceed DUMP_BUDGET_BYTES, a fixed sample of env indices (RandomState(0), sorted) is kept on every plane; env_index.npy
    holds the env indices written either way."""
    os.makedirs(out_dir, exist_ok=True)

    def nbytes(a):
        if torch.is_tensor(a):
            return a.numel() * (8 if a.dtype == torch.float64 else 4)
        a = np.asarray(a)
        return a.size * (8 if a.dtype == np.float64 else 4)
    total = sum(nbytes(a) for a, _ in planes.values())
    if total <= DUMP_BUDGET_BYTES:
        idx = np.arange(n)
    else:
        idx = np.sort(np.random.RandomState(0).choice(n, max(1, DUMP_BUDGET_BYTES * n // total), replace=False))
    for name, (a, axis) in planes.items():
        if torch.is_tensor(a):
            a = a.index_select(axis, torch.from_numpy(idx).to(a.device)).cpu().numpy()
        else:
            a = np.take(np.asarray(a), idx, axis=axis)
        np.save(os.path.join(out_dir, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))
    np.save(os.path.join(out_dir, "env_index.npy"), idx.astype(np.float64))


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start the N ranks ourselves (one process per GPU,
    SURVEY 8e / rl_baselines/utils.py:213-220 "one worker per env" becomes "one rank per shard") by re-executing this file
    under torch.distributed.run on the loopback address; rank 0's single JSON line goes straight to our stdout."""
    import socket
    import subprocess
    n = args.gpus
    if not os.environ.get("SRLHIP_SINGLE_DEVICE"):
        have = torch.cuda.device_count()
        if have < n:
            raise SystemExit("bench.py --gpus {}: only {} GPU(s) visible (set SRLHIP_SINGLE_DEVICE=1 SRLHIP_DIST_BACKEND=gloo "
                             "for a dry run of the N > 1 path on one device)".format(n, have))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


_LIVE_PMC = {}      # workload -> {kernel: {counter: (sum, dispatches)}} measured by child passes of this run


def live_pmc(args, workload):
    """HBM traffic and instruction counters of THIS run's kernels: the same command (short: 1 warm-up + 2 steps) re-run as child
    processes under `rocprofv3 --pmc`, one pass per counter set and no tracing options (MI355X_MICROARCH.md, HBM / rocprofv3
    section), aggregated per kernel like profiles/summarize_pmc.py.  Rank 0 of an N = 1 --full run only; None (-> the committed
    summaries) when rocprofv3 is missing, a pass fails, or we ARE such a child."""
    import csv
    import re
    import shutil
    import subprocess
    import tempfile
    if workload in _LIVE_PMC:
        return _LIVE_PMC[workload]
    _LIVE_PMC[workload] = None
    if not args.full or args.no_live_pmc or os.environ.get("SRLHIP_BENCH_CHILD") or shutil.which("rocprofv3") is None:
        return None
    sets = ["FETCH_SIZE", "WRITE_SIZE"] + (["SQ_WAVES SQ_INSTS_VALU"] if workload == "kuka" else [])
    agg = {}
    env = dict(os.environ, SRLHIP_BENCH_CHILD="1", TMPDIR="/tmp")
    try:
        for pmc in sets:
            out = tempfile.mkdtemp(prefix="srlhip_pmc_", dir="/tmp")
            cmd = ["rocprofv3", "--pmc"] + pmc.split() + ["--output-format", "csv", "-d", out, "-o", "pmc", "--", sys.executable,
                   os.path.abspath(__file__), "--workload", workload, "--no-cpu-baseline", "--no-secondary", "--steps", "2", "--warmup", "1",
                   "--envs-per-gpu", str(args.envs_per_gpu), "--rng", args.rng, "--kuka-model", args.kuka_model]
            if args.inner_steps is not None:
                cmd += ["--inner-steps", str(args.inner_steps)]
            rc = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240).returncode
            found = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith("counter_collection.csv")]
            if rc != 0 or not found:
                shutil.rmtree(out, ignore_errors=True)
                return None
            disp = {}
            for r in csv.DictReader(open(found[0])):
                m = re.search(r"(\w+_k)\b", r["Kernel_Name"])
                name = m.group(1) if m else r["Kernel_Name"].split("<")[0].split("(")[0][-40:]
                k = agg.setdefault(name, {})
                k[r["Counter_Name"]] = k.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                disp.setdefault((name, r["Counter_Name"]), set()).add(r["Dispatch_Id"])
            for (name, c), ids in disp.items():
                agg[name][c] = (agg[name][c], len(ids))
            shutil.rmtree(out, ignore_errors=True)
    except Exception:
        return None
    _LIVE_PMC[workload] = agg
    return agg


def live_traffic(args, workload, kernel):
    """bytes per launch of `kernel` from this run's child PMC passes (helper kernels spread over its launches), or None"""
    agg = live_pmc(args, workload)
    if not agg or kernel not in agg or "FETCH_SIZE" not in agg[kernel] or "WRITE_SIZE" not in agg[kernel]:
        return None
    kernels = [kernel] + (["mobile_sample_actions_k"] if workload == "mobile" else [])
    launches = agg[kernel]["FETCH_SIZE"][1]
    tot = {c: sum(agg[k][c][0] for k in kernels if k in agg and c in agg[k]) / launches for c in ("FETCH_SIZE", "WRITE_SIZE")}
    return (2.0 * tot["FETCH_SIZE"] + tot["WRITE_SIZE"]) * 1024.0


def measured_traffic(kernel, env_steps_per_launch):
    """HBM bytes per launch of `kernel` from the newest committed PMC summaries (profiles/rNN_*_pmc_{FETCH,WRITE}_SIZE.csv,
    collected by profiles/collect.sh in separate --pmc passes of this same command).  FETCH_SIZE / WRITE_SIZE are in KiB;
    FETCH_SIZE is doubled per MI355X_MICROARCH.md §HBM (gfx950 tallies 128-B requests at 64 B).  None if no summary
    matches this launch geometry."""
    import csv
    import glob
    import re
    wl = "kuka" if kernel.startswith("kuka") else "mobile"
    kernels = [kernel] + (["mobile_sample_actions_k"] if wl == "mobile" else [])   # the timed region covers both mobile kernels
    out = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        # only this round's summaries: a silent fall-back to an older round's file would report another kernel's traffic
        files = sorted(glob.glob(os.path.join(REPO, "profiles", "r{:02d}_{}_pmc_{}.csv".format(PROFILE_ROUND, wl, counter))))
        if not files:
            return None
        rows = [row for row in csv.DictReader(open(files[-1])) if row["kernel"] in kernels and row["counter"] == counter]
        launches = [float(row["dispatches"]) for row in rows if row["kernel"] == kernel]
        if not launches:
            return None
        # per launch of `kernel`: its own average plus the other kernels' totals spread over its launches (the standalone
        # action sampler only runs when no plane was drawn ahead: once per bench run)
        out[counter] = sum(float(row["sum"]) for row in rows) / launches[0]
    if len(out) != 2:
        return None
    return (2.0 * out["FETCH_SIZE"] + out["WRITE_SIZE"]) * 1024.0


def cpu_baseline(workload, n_envs, budget_s=12.0, full=True):
    """Oracle ('port') timed on this box's host cores, rank 0, N=1 only."""
    from oracle import clib
    if workload == "mobile":
        # BASELINE config 1: 4 envs behind a SubprocVecEnv-protocol emulation (the way the reference runs N envs)
        from oracle import subproc_baseline
        base = subproc_baseline.mobile_subproc_fps(num_cpu=4, n_steps=2048, warmup=256)
        T = 1024
        t0 = time.perf_counter()
        reps = 0
        while time.perf_counter() - t0 < 3.0:
            clib.mobile_rollout(0, np.arange(n_envs), T, actions=None, rng_mode=clib.RNG_PHILOX)
            reps += 1
        base["c_port_1_thread_env_steps_per_s"] = reps * T * n_envs / (time.perf_counter() - t0)
        return base
    from oracle import kuka_clib
    return kuka_clib.cpu_baseline(10.0, full=full)


def pixel_cpu_baseline(enc, env, budget_s=3.0, phys=None):
    """Config 4 on the host cores ('port'): the C oracles step the physics (OpenMP) and ray-cast 64x64 frames (OpenMP), the
    same CustomCNN runs in float32 under PyTorch on the CPU; each stage timed on a bounded sample and combined per
    env-step (the stages are sequential in the reference: render inside env.step, then the encoder)."""
    from oracle import kuka_clib, raster_clib
    from state_representation.models import SRLNeuralNetwork
    from srlhip import _lib
    if phys is None or not phys.get("value"):
        phys = kuka_clib.cpu_baseline(budget_s, subproc=False)                # env-steps/s, physics only
    n = 1024
    h = env.h
    state = np.concatenate([h.get_state(_lib.F_KUKA_Q).T, h.get_state(_lib.F_KUKA_BUTTON_Q)[0][:, None],
                            h.get_state(_lib.F_KUKA_BUTTON_XY).T], axis=1)[:n]
    gq = h.get_state(_lib.F_KUKA_GRIPPER_Q).T[:n] if h.cfg.kuka_model == _lib.KUKA_MODEL_FULL else None       # full model: fingers drawn from their joints
    kuka_clib.set_full(gq is not None)
    frames = raster_clib.render(4, state, 64, 64, gripper_q=gq)
    t0 = time.perf_counter(); reps = 0
    while time.perf_counter() - t0 < budget_s:
        frames = raster_clib.render(4, state, 64, 64, gripper_q=gq); reps += 1
    raster_rate = reps * n / (time.perf_counter() - t0)
    cpu_enc = SRLNeuralNetwork(enc.state_dim, cuda=False, img_shape=(64, 64), state_dict=enc.model.state_dict(), backend="torch")
    cpu_enc.getStates(frames[:64])
    t0 = time.perf_counter(); reps = 0
    while time.perf_counter() - t0 < budget_s:
        cpu_enc.getStates(frames); reps += 1
    enc_rate = reps * n / (time.perf_counter() - t0)
    value = 1.0 / (1.0 / phys["value"] + 1.0 / raster_rate + 1.0 / enc_rate)
    return {"value": value, "unit": "env-steps/s", "cores": phys["cores"], "kind": "port",
            "sample": "per stage ~{:.0f} s on the host cores: oracle/kuka_oracle.c physics {:.3g} env-steps/s, oracle/raster_oracle.c "
                      "64x64 frames {:.3g}/s ({} frames per pass), PyTorch CPU float32 CustomCNN {:.3g} frames/s; combined as "
                      "sequential stages".format(budget_s, phys["value"], raster_rate, n, enc_rate)}


def bench_pixels(args, rank, local_rank, world, dev, K=None, W=None, cpu=True, phys_baseline=None, dump=None):
    """BASELINE config 4/5: KukaButtonGymEnv raw_pixels 64x64 -> tile rasteriser -> SRL encoder forward
    (fused HIP kernel, csrc/encoder.hip) on the same device.  One bench step = `inner` VecEnv steps of this rank's shard."""
    from srlhip import _lib, sharding
    from srlhip.pixel_env import PixelStateVecEnv
    from state_representation.models import SRLNeuralNetwork
    n, S = args.envs_per_gpu, args.img_size
    inner = args.inner_steps or (256 if S == 64 else 32)       # >= 256 VecEnv steps per bench step at the BASELINE size
    K = K if K is not None else (args.steps if args.steps is not None else 8)
    W = W if W is not None else (args.warmup if args.warmup is not None else 1)
    torch.manual_seed(0)
    enc = SRLNeuralNetwork(3, cuda=True, img_shape=(S, S), device=dev)
    first, _ = sharding.shard_range(world * n, world, rank)
    env = PixelStateVecEnv("KukaButtonGymEnv-v0", n, enc, seed=0, img_shape=(S, S), device_id=local_rank, first_env_id=first)
    env.reset()
    gathered = torch.zeros((world * n,), dtype=torch.float32, device=dev) if world > 1 else None
    ret = torch.zeros((n,), dtype=torch.float32, device=dev)
    last = {}

    def one_step():
        for _ in range(inner):
            states, rew, done = env.step()
        last["states"], last["reward"], last["done"] = states, rew, done
        if world > 1:
            env.h.episode_stats_device(last_return=ret.data_ptr())     # enqueued on the stepper's stream
            torch.cuda.current_stream(dev).wait_stream(env._stream)
            sharding.gather_episode_returns(ret, out=gathered)

    def fence():
        env.h.sync()
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    for _ in range(W):
        one_step()
    fence()
    t0 = time.perf_counter()
    for _ in range(K):
        one_step()
    fence()
    dt_own = time.perf_counter() - t0
    dt_ranks = sharding.per_rank(dt_own, device=dev)
    dt = sharding.max_over_ranks(dt_own, device=dev)
    if dump and rank == 0:
        dump_outputs(dump, {k: (v, 0) for k, v in last.items()}, n)
    value = world * n * inner * K / dt
    step_ms = dt * 1e3 / (K * inner)
    hip_encoder = enc.hip is not None
    line = {"metric": "env steps/sec (whole node), KukaButtonGymEnv {} envs/GPU".format(n), "value": value,
            "unit": "env-steps/s", "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": dt * 1e3 / K,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64 dynamics, f32 raster, f32-accurate split-f16 MFMA encoder" if hip_encoder else "f64 dynamics, f32 raster/encoder",
            "data": "synthetic",
            "config": {"workload": "KukaButtonGymEnv-v0 raw_pixels {}x{}, {} envs per GPU, rasteriser + srl_zoo CustomCNN "
                                   "forward (random init) on the same device, random-agent actions".format(S, S, n),
                       "envs_per_gpu": n, "inner_steps": inner, "parallelism": "env-shard x{}".format(world),
                       "encoder_backend": enc.backend, "ms_per_vecenv_step": step_ms,
                       "x_vs_published_250fps_cpu": value / PUBLISHED_REFERENCE_FPS}}
    if world > 1:      # stragglers: every rank's own time for the K steps (value uses the maximum)
        line["config"]["ms_per_step_ranks"] = {"min": min(dt_ranks) * 1e3 / K, "max": max(dt_ranks) * 1e3 / K, "all": [x * 1e3 / K for x in dt_ranks]}
    if not args.full:       # what follows takes runs of its own
        env.close()
        return line
    # per-kernel shares, each timed alone with HIP events on the stepper's own stream (the stream all three run on)
    # (`reps` launches captured in a HIP graph and replayed between the two events: the figure does not depend on how fast this
    #  process can enqueue — a busy host once made the eagerly-enqueued "alone" time longer than the whole step that contains it)
    env.h.sync()
    reps = 50

    def graph_ms(enqueue):
        enqueue()                                   # lazy allocations happen outside the capture
        env.h.sync()
        env.h.graph_begin()
        for _ in range(reps):
            enqueue()
        g = env.h.graph_end()
        try:
            env.h.graph_launch(g)                   # warm replay
            env.h.sync()
            env.h.timing_begin()
            env.h.graph_launch(g)
            return env.h.timing_end() / reps
        finally:
            env.h.graph_destroy(g)

    raster_ms = graph_ms(lambda: env.h.render(out=env.images.data_ptr()))
    enc_ms = graph_ms(lambda: enc.getStates(env.images, stream=env._stream_ptr, out=env.states)) if hip_encoder else None
    stepper_ms = graph_ms(lambda: env.h.rollout(1, out=(0, env.rewards.data_ptr(), env.dones.data_ptr(), env.actions.data_ptr())))
    raster_gbs = n * S * S * 3 / (raster_ms * 1e-3) / 1e9
    raster_roof = {"bound": "hbm", "kernel": "raster_k", "achieved": raster_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": raster_gbs / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": raster_ms,
                   "alg_bytes_per_env_step": S * S * 3, "env_steps_per_launch": n,
                   "note": "image write only ({} B per env); the rasteriser is ray-cast ALU bound".format(S * S * 3)}
    # CustomCNN map sizes for an S x S frame: conv7/2 p3 -> pool3/2 p1 -> conv3 p1 -> pool3/2 -> conv3/2 p1 -> pool3/2
    c1 = (S + 6 - 7) // 2 + 1; p1 = (c1 + 2 - 3) // 2 + 1; c2 = p1; p2 = (c2 - 3) // 2 + 1; c3 = (p2 + 2 - 3) // 2 + 1; p3 = (c3 - 3) // 2 + 1
    if hip_encoder:
        # dominant kernel of this path: the fused encoder (csrc/encoder.hip).  Algorithmic work = the float32 network's
        # 2*K*N*M flops per frame (conv1 147x64x1024, conv2 576x64x256, conv3 576x64x16, FC); it is executed on the
        # f16 matrix pipe with split operands (2-3 MFMAs per algorithmic one, K padded 147 -> 224 in layer 1), so the
        # peak it is priced against is the dense f16 MFMA peak.
        flops_frame = 2.0 * (147 * 64 * c1 * c1 + 576 * 64 * c2 * c2 + 576 * 64 * c3 * c3 + 64 * p3 * p3 * enc.state_dim)
        mfma_frame = 4 * (8.5 * 56 + 432 + 54) * 32768.0          # executed: 4 waves x MFMAs x 32x32x16x2
        tf = flops_frame * n / (enc_ms * 1e-3) / 1e12
        roofline = {"bound": "mfma", "kernel": "encoder_fwd_k" if S == 64 else "enc_layer_k x3 + enc_fc_k (csrc/encoder_general.hip)", "achieved": tf, "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": tf / F16_MFMA_PEAK_TFLOPS, "traffic": n * S * S * 3 if S == 64 else None, "avg_launch_ms": enc_ms,
                    "alg_flops_per_env_step": flops_frame, "env_steps_per_launch": n,
                    "executed_mfma_tflops": mfma_frame * n / (enc_ms * 1e-3) / 1e12 if S == 64 else None,
                    "f32_mfma_peak_tflops": F32_MFMA_PEAK_TFLOPS,
                    "traffic_source": "algorithmic = measured: one 12 288-byte frame read per env-step (profiles/ PMC FETCH_SIZE x2), "
                                      "state_dim floats written; weights (352 KiB) stay in L2",
                    "note": "float32-accurate results (7e-7 rel. vs torch CPU) from split-f16 MFMAs; vs the f32 MFMA peak "
                            "({} TFLOP/s) the algorithmic rate is {:.2f}x".format(F32_MFMA_PEAK_TFLOPS, tf / F32_MFMA_PEAK_TFLOPS),
                    "raster_k": raster_roof}
    else:
        roofline = raster_roof
    line["config"]["kernel_ms"] = {"raster_k": raster_ms, "encoder_fwd_k": enc_ms, "stepper_single_step_launch": stepper_ms,
                                   "stepper_and_launch_gaps": step_ms - raster_ms - (enc_ms or 0.0),
                                   "how": "each kernel alone: {} launches replayed from one HIP graph between two events on the stepper's stream".format(reps)}
    line["roofline"] = roofline
    if world == 1 and rank == 0 and S == 64:
        # HBM bytes per launch of the two pixel-path kernels, re-measured now: this command as child processes under rocprofv3 --pmc
        # (separate FETCH_SIZE / WRITE_SIZE passes, MI355X_MICROARCH.md's HBM section), FETCH_SIZE x2 + WRITE_SIZE in KiB
        t_r = live_traffic(args, "kuka_pixels", "raster_k")
        t_e = live_traffic(args, "kuka_pixels", "encoder_fwd_k") if hip_encoder else None
        src = "measured in this run: the same command re-run as child processes under rocprofv3 --pmc (FETCH_SIZE x2 + WRITE_SIZE, KiB), bytes per launch"
        if t_r is not None:
            raster_roof["traffic"] = t_r; raster_roof["traffic_source"] = src
            raster_roof["traffic_over_algorithmic"] = t_r / float(n * S * S * 3)
        if t_e is not None and hip_encoder:
            roofline["traffic"] = t_e; roofline["traffic_source"] = src
    if rank == 0 and world == 1 and cpu and not args.no_cpu_baseline and S == 64:
        try:
            line["cpu_baseline"] = pixel_cpu_baseline(enc, env, phys=phys_baseline)
            line["cpu_baseline"]["host"] = "{} logical cores".format(os.cpu_count())
        except Exception as exc:      # the checker must never sink the measurement
            line["cpu_baseline"] = {"value": None, "error": repr(exc)}
    env.close()
    return line


def pmc_issue_util(kernel, avg_launch_s, clock_hz=2.35e9):      # (the PMC pass's GRBM_GUI_ACTIVE says 2.35 GHz under this load)
    """VALU issue utilisation of `kernel`: instructions per wavefront (newest committed PMC summary, SQ_INSTS_VALU / SQ_WAVES)
    x 4 cycles per wave64 float64 instruction / cycles of one launch (live duration x 2.4 GHz).  None without a summary."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r{:02d}_kuka_pmc_SQ_WAVES.csv".format(PROFILE_ROUND))))
    files = [f for f in files if any(row["kernel"] == kernel for row in csv.DictReader(open(f)))]      # a summary that saw THIS kernel
    if not files:
        return None
    c = {}
    for row in csv.DictReader(open(files[-1])):
        if row["kernel"] == kernel:
            c[row["counter"]] = float(row["avg_per_dispatch"])
    if "SQ_INSTS_VALU" not in c or not c.get("SQ_WAVES"):
        return None
    per_wave = c["SQ_INSTS_VALU"] / c["SQ_WAVES"]
    return {"valu_insts_per_wavefront": per_wave, "waves_per_dispatch": c["SQ_WAVES"],
            "issue_util": per_wave * 4.0 / (avg_launch_s * clock_hz), "source": os.path.basename(files[-1])}


def bench_stepper(args, workload, rank, local_rank, world, dev, K=None, W=None, cpu=True, backend="nccl", dump=None):
    """BASELINE configs 2 / 3: the ground-truth stepper alone.  Returns the bench line (dict)."""
    from srlhip import _lib, sharding
    n = args.envs_per_gpu
    # one bench step = a T = 2048-step rollout of every env (each Kuka env crosses >= 2 auto-resets, each
    # MobileRobot env 8), after a warm-up of >= 256 steps (one 2048-step rollout by default)
    inner = args.inner_steps or 2048
    K = K if K is not None else (args.steps if args.steps is not None else 20)
    W = W if W is not None else (args.warmup if args.warmup is not None else (5 if workload == "mobile" else 1))

    kind = _lib.ENV_MOBILE if workload == "mobile" else _lib.ENV_KUKA_BUTTON
    cfg = _lib.default_config(kind)
    first_env_id, _ = sharding.shard_range(world * n, world, rank)
    cfg.num_envs, cfg.device_id, cfg.first_env_id, cfg.seed0 = n, local_rank, first_env_id, 0
    cfg.rng_mode = _lib.RNG_PHILOX if args.rng == "philox" else _lib.RNG_MT19937
    cfg.auto_reset, cfg.io_device = 1, 1
    if workload == "kuka":
        cfg.kuka_model = _lib.KUKA_MODEL_FULL if args.kuka_model == "full" else _lib.KUKA_MODEL_LUMPED
    h = _lib.Handle(cfg)                  # raises SrlHipError when the library / GPU is missing: no fallback workload
    od = h.obs_dim
    obs0 = torch.zeros((n, od), dtype=torch.float32, device=dev)
    obs = torch.zeros((inner, n, od), dtype=torch.float32, device=dev)
    rew = torch.zeros((inner, n), dtype=torch.float32, device=dev)
    done = torch.zeros((inner, n), dtype=torch.uint8, device=dev)
    act = torch.zeros((inner, n), dtype=torch.int32, device=dev)
    out = (obs.data_ptr(), rew.data_ptr(), done.data_ptr(), act.data_ptr())
    h.reset(obs_out=obs0.data_ptr())
    h.sync()

    gathered = None
    if world > 1:
        import torch.distributed as dist
        gathered = torch.zeros((world * n,), dtype=torch.float32, device=dev)

    ext = torch.cuda.ExternalStream(h.stream(), device=dev) if world > 1 else None

    ep_ret = torch.zeros((n,), dtype=torch.float32, device=dev)      # Monitor's r of each env's last finished episode

    def one_step():
        h.rollout(inner, out=out)
        if world > 1:
            # the path's only exchange: per-env episode returns, once per rollout, RCCL over xGMI.  No host
            # sync: the stepper's stream narrows its episode statistics into `ep_ret` (srlhip_episode_stats_device),
            # torch's stream waits for that and all-gathers; the next rollout only waits until the gather has read `ep_ret`.
            h.episode_stats_device(last_return=ep_ret.data_ptr())
            cur = torch.cuda.current_stream(dev)
            cur.wait_stream(ext)
            sharding.gather_episode_returns(ep_ret, out=gathered)
            done_reading = torch.cuda.Event()
            done_reading.record(cur)
            ext.wait_event(done_reading)

    def fence():
        h.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(W):
        one_step()
    fence()
    h.timing_begin()
    t0 = time.perf_counter()
    for _ in range(K):
        one_step()
    kernel_ms = h.timing_end()          # HIP events on the stepper's own stream
    fence()
    dt = time.perf_counter() - t0
    dt_ranks = sharding.per_rank(dt, device=dev)
    dt = sharding.max_over_ranks(dt, device=dev)
    if dump and rank == 0:      # the planes of the last timed rollout, [T][n] (this rank's shard)
        dump_outputs(dump, {"obs": (obs, 1), "reward": (rew, 1), "done": (done, 1), "actions": (act, 1)}, n)

    total_env_steps = world * n * inner * K
    value = total_env_steps / dt
    steps_per_launch = n * inner
    avg_launch_s = kernel_ms * 1e-3 / K
    achieved_gbs = ALG_BYTES[workload] * steps_per_launch / avg_launch_s / 1e9
    kernel = "mobile_rollout_ep_k" if workload == "mobile" else {"tree": "kuka_tree_rollout_k", "group": "kuka_group_rollout_k", "lane": "kuka_rollout_k"}[h.kuka_kernel()]
    traffic, traffic_live = None, False
    if world == 1 and rank == 0:
        traffic = live_traffic(args, workload, kernel)          # re-measured now: child passes under rocprofv3 --pmc
        traffic_live = traffic is not None
    if traffic is None and n == 4096 and inner == 2048:       # geometry the committed PMC passes were taken at
        traffic = measured_traffic(kernel, steps_per_launch)
    if workload == "mobile":
        # The SURVEY 8(d) contract prices a step-at-a-time stepper (73 algorithmic bytes per env-step); a fused rollout keeps the state
        # in VGPRs and never moves most of them, so that formula exceeds 1.  `frac` is therefore the fraction by the bytes that physically
        # cross HBM (PMC FETCH_SIZE x2 + WRITE_SIZE per launch); the contract figure rides along under its own name.
        roofline = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": traffic, "kernel": kernel,
                    "avg_launch_ms": avg_launch_s * 1e3,
                    "alg_bytes_per_env_step": ALG_BYTES[workload], "env_steps_per_launch": steps_per_launch,
                    "survey_8d_contract_gbs": achieved_gbs, "survey_8d_contract_frac": achieved_gbs / HBM_PEAK_GBS,
                    "note": "achieved / frac = bytes that physically cross HBM per launch (`traffic`, PMC) / launch time / 8 TB/s; "
                            "survey_8d_contract_* = the SURVEY 8(d) formula (73 algorithmic bytes per env-step of a step-at-a-time "
                            "stepper), which a fused rollout with its state in VGPRs does not move"}
        if traffic is not None:
            roofline["achieved"] = traffic / avg_launch_s / 1e9
            roofline["frac"] = roofline["achieved"] / HBM_PEAK_GBS
            roofline["physical_hbm_gbs"], roofline["physical_hbm_frac"] = roofline["achieved"], roofline["frac"]
            roofline["frac_basis"] = "physical"
        else:
            # no PMC figure for this geometry (no rocprofv3, or not 4096 x 2048): achieved / frac stay NUMERIC — the SURVEY 8(d)
            # contract figure, flagged (it can exceed 1 for a fused rollout, see `note`)
            roofline["achieved"], roofline["frac"], roofline["frac_basis"] = achieved_gbs, achieved_gbs / HBM_PEAK_GBS, "survey_8d_contract (no PMC traffic for this geometry)"
    else:
        from srlhip import kuka_model
        kk = h.kuka_kernel()
        group = kk != "lane"
        flops = {"tree": kuka_model.FLOPS_PER_ENV_STEP_TREE, "group": kuka_model.FLOPS_PER_ENV_STEP_GROUP, "lane": kuka_model.FLOPS_PER_ENV_STEP}[kk]
        tf = flops * steps_per_launch / avg_launch_s / 1e12
        # the Kuka stepper is bounded by the float64 vector pipe (issue rate / dependency latency of the 150 Gauss-Seidel
        # sweeps), so `frac` is the FP64-VALU fraction; the HBM fraction the north star asks for rides along
        roofline = {"bound": "valu_fp64", "achieved": tf, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": tf / FP64_VALU_PEAK_TFLOPS, "traffic": traffic, "kernel": kernel,
                    "avg_launch_ms": avg_launch_s * 1e3, "flops_per_env_step": flops,
                    "flops_source": "srlhip/kuka_model.py: algorithmic float64 operations of the row set the {} kernel "
                                    "integrates (FMA = 2)".format({"tree": "tree lane-group (full 12-DoF model)", "group": "lane-group", "lane": "lane-per-env"}[kk]),
                    "hbm_achieved_gbs": achieved_gbs, "hbm_frac": achieved_gbs / HBM_PEAK_GBS,
                    "alg_bytes_per_env_step": ALG_BYTES[workload], "env_steps_per_launch": steps_per_launch,
                    "launch_geometry": "16 lanes per env, 1 wavefront per workgroup: {} wavefronts".format((n + 3) // 4)
                    if group else "1 lane per env: {} wavefronts".format((n + 63) // 64),
                    "note": "FP64-VALU issue / dependency-latency bound, not HBM bound (SURVEY 7 hard parts); hbm_frac is "
                            "reported because the north star asks for it"}
        util = None
        agg = live_pmc(args, workload) if (world == 1 and rank == 0) else None
        if agg and kernel in agg and "SQ_INSTS_VALU" in agg[kernel] and "SQ_WAVES" in agg[kernel]:
            # wavefronts per launch from the launch geometry (SQ_WAVES is reported beside it: the counter has been seen to absorb
            # the previous dispatch's wavefronts once in a while)
            waves = float((n + 3) // 4 if group else (n + 63) // 64)
            per_wave = agg[kernel]["SQ_INSTS_VALU"][0] / agg[kernel]["SQ_INSTS_VALU"][1] / waves
            util = {"valu_insts_per_wavefront": per_wave, "waves_per_dispatch": waves,
                    "sq_waves_per_dispatch": agg[kernel]["SQ_WAVES"][0] / agg[kernel]["SQ_WAVES"][1],
                    "issue_util": per_wave * 4.0 / (avg_launch_s * 2.35e9), "source": "rocprofv3 --pmc child pass of this run"}
        elif n == 4096 and inner == 2048:
            util = pmc_issue_util(kernel, avg_launch_s)
        if util:
            roofline.update(util)
            # what the number is measured against: ONE wavefront per SIMD running ONE dependent float64 chain (which is what a
            # Gauss-Seidel sweep is) completes an operation every 2.60 ns where the SIMD's issue limit is 1.72 ns
            # (profiles/probes/f64_issue_rate.hip, profiles/r04_f64_issue_rate.txt)
            roofline["issue_util_of_one_dependent_f64_chain"] = 0.66
    if traffic is not None:
        roofline["traffic_source"] = ("measured in this run: the same command re-run as child processes under rocprofv3 --pmc "
                                      "(separate FETCH_SIZE / WRITE_SIZE passes; FETCH_SIZE x2 + WRITE_SIZE, KiB), bytes per launch"
                                      if traffic_live else
                                      "profiles/ PMC summaries of this command (FETCH_SIZE x2 + WRITE_SIZE, KiB), bytes per "
                                      "launch; committed, not re-measured in this run")
    line = {
        "metric": "env steps/sec (whole node), {} {} envs/GPU".format(
            "KukaButtonGymEnv" if workload == "kuka" else "MobileRobotGymEnv", n),
        "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": dt * 1e3 / K, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "{}-v0 ground_truth obs, {} envs per GPU, random-agent discrete actions".format(
            "KukaButtonGymEnv" if workload == "kuka" else "MobileRobotGymEnv", n),
            "envs_per_gpu": n, "inner_steps": inner, "env_steps_per_bench_step": world * n * inner,
            "rng_mode": args.rng, "auto_reset": True, "parallelism": "env-shard x{}".format(world),
            "x_vs_published_250fps_cpu": value / PUBLISHED_REFERENCE_FPS},
        "roofline": roofline,
    }
    if workload == "kuka":
        line["config"]["kuka_model"] = h.kuka_model_name()
        if args.kuka_model == "full":
            # rounds 1-2 reported this metric for the lumped-gripper model (2.4e8): a different, cheaper simulation
            line["config"]["model_note"] = ("the full arm + gripper model since round 3; the rounds 1-2 lumped-gripper model "
                                            "(gripper welded to link 7, 7 DoF) is `--kuka-model lumped`")
    if world > 1:
        torch.cuda.synchronize()
        # stragglers: every rank's own time for the K steps (value uses the maximum)
        line["config"]["ms_per_step_ranks"] = {"min": min(dt_ranks) * 1e3 / K, "max": max(dt_ranks) * 1e3 / K, "all": [x * 1e3 / K for x in dt_ranks]}
        line["config"]["episode_returns_allgathered"] = {"count": int(gathered.numel()), "mean": float(gathered.mean().item()),
                                                         "collective": "all_gather_into_tensor float32[{}] per rank, once per rollout ({})".format(n, backend)}
    if rank == 0 and world == 1 and cpu and args.full and not args.no_cpu_baseline:
        try:
            line["cpu_baseline"] = cpu_baseline(workload, n, full=args.kuka_model == "full")
            line["cpu_baseline"]["host"] = "{} logical cores".format(os.cpu_count())
        except Exception as exc:      # the checker must never sink the measurement
            line["cpu_baseline"] = {"value": None, "error": repr(exc)}
    h.close()
    return line


def bench_per_step(args, emit=True):
    """The per-step API of the drop-in (rl_baselines/utils.py:213-229 -> HipVecEnv): K x (step_async + step_wait) with host-side random
    actions, every shard launched before any is collected.  ONE process; n = envs_per_gpu x number of shards.  Also reports the split
    (time inside step_async = launches only; inside step_wait = the GPU's step + collection) and the single-shard figure beside it."""
    from srlhip.vec_env import HipVecEnv, parse_device_ids
    device_ids = parse_device_ids(args.device_ids) or [0]
    workload = "kuka" if args.workload == "auto" else args.workload
    env_id = {"kuka": "KukaButtonGymEnv-v0", "mobile": "MobileRobotGymEnv-v0"}[workload]
    K = args.steps if args.steps is not None else 2000
    W = args.warmup if args.warmup is not None else 300

    def run(ids, persistent=None, dump=None):
        n = args.envs_per_gpu * len(ids)
        env = HipVecEnv(env_id, n, seed=0, env_kwargs={"srl_model": "ground_truth"}, device_ids=ids, rng_mode=args.rng, persistent=persistent)
        env.reset()
        acts = np.random.RandomState(0).randint(env.action_space.n, size=(64, n)).astype(np.int32)
        for t in range(W):
            env.step(acts[t % 64])
        ta = tw = 0.0
        lat = np.zeros(K)
        t_begin = time.perf_counter()
        for t in range(K):
            t0 = time.perf_counter()
            env.step_async(acts[t % 64])
            t1 = time.perf_counter()
            obs, rew, dones, _ = env.step_wait()
            t2 = time.perf_counter()
            ta += t1 - t0; tw += t2 - t1; lat[t] = t2 - t0
        dt = time.perf_counter() - t_begin
        if dump:       # what the last timed step_wait returned
            dump_outputs(dump, {"obs": (obs, 0), "reward": (rew, 0), "done": (dones, 0)}, n)
        env.close()
        return {"n": n, "value": n * K / dt, "us_per_step_mean": dt / K * 1e6, "us_per_step_median": float(np.median(lat)) * 1e6,
                "us_in_step_async": ta / K * 1e6, "us_in_step_wait": tw / K * 1e6}

    r = run(device_ids, True if args.persistent else None, dump=args.dump_outputs if emit else None)
    line = {"metric": "env steps/sec, per-step VecEnv API (HipVecEnv.step{}), {} {} envs per shard x {} shard(s)".format(
                ", persistent stepping" if args.persistent else "", env_id.split("-")[0], args.envs_per_gpu, len(device_ids)),
            "value": r["value"], "unit": "env-steps/s", "n_gpus": len(set(device_ids)), "steps": K, "warmup": W, "ms_per_step": r["us_per_step_mean"] / 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "{} ground_truth obs through HipVecEnv.step_async / step_wait, one process, device_ids {}".format(env_id, device_ids),
                       "envs_per_shard": args.envs_per_gpu, "device_ids": device_ids, "rng_mode": args.rng, "per_step": r}}
    if args.persistent:
        line["config"]["persistent"] = True
        line["config"]["launch_per_step"] = run(device_ids)
    if len(device_ids) > 1:
        line["config"]["single_shard"] = run(device_ids[:1], True if args.persistent else None)
        line["config"]["step_time_vs_single_shard"] = r["us_per_step_median"] / line["config"]["single_shard"]["us_per_step_median"]
    if emit:
        print(json.dumps(line))
    return line


def main():
    args = parse()
    if args.per_step:
        return bench_per_step(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args)
    from srlhip import sharding
    rank, local_rank, world = sharding.dist_env()
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus {} but the launcher started {} rank(s)".format(args.gpus, world))
    backend = os.environ.get("SRLHIP_DIST_BACKEND", "nccl")   # "nccl" == RCCL over xGMI on ROCm
    if os.environ.get("SRLHIP_SINGLE_DEVICE"):                # dry run of the N>1 path on a 1-GPU box (gloo)
        local_rank = 0
    if world > 1:
        import torch.distributed as dist
        sharding.init_process_group(backend, local_rank)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    # "auto" = the configuration the metric is quoted on (BASELINE config 3).  No fallback: a missing library / GPU raises.
    workload = "kuka" if args.workload == "auto" else args.workload
    if workload == "kuka_pixels":
        line = bench_pixels(args, rank, local_rank, world, dev, dump=args.dump_outputs)
    else:
        line = bench_stepper(args, workload, rank, local_rank, world, dev, backend=backend, dump=args.dump_outputs)
    line["config"]["ranks_seen"] = world
    line["config"]["dist_backend"] = ("{} (RCCL over xGMI)".format(backend) if backend == "nccl" else backend) if world > 1 else None
    if args.full and args.workload == "auto" and world == 1 and not args.no_secondary and args.envs_per_gpu == 4096:
        # BASELINE configs 2 and 4, briefly, in the same driver-run line (their own value / roofline / cpu_baseline)
        sec = {}
        saved = args.inner_steps
        saved_img = args.img_size
        for name in ("mobile", "kuka_pixels", "kuka_pixels_224"):
            try:
                args.inner_steps = None
                args.img_size = saved_img
                if name == "kuka_pixels_224":
                    # the reference's own frame size (kuka_button_gym_env.py:21-22 RENDER 224 x 224): rasteriser + the layered encoder
                    # (csrc/encoder_general.hip); 16 VecEnv steps per bench step, 2 bench steps
                    args.img_size, args.inner_steps = 224, 16
                    sub = bench_pixels(args, rank, local_rank, world, dev, K=2, W=1, cpu=False)
                elif name == "mobile":
                    # (a rollout of this family lasts 0.1 ms: 300 of them, so that the GPU clocks are up and the timed region is not
                    #  2 ms; the headline's CPU baseline has just torn down 256 worker processes and a 256-thread OpenMP team: give
                    #  the host two seconds, this leg issues a launch every 50 us)
                    time.sleep(2.0)
                    sub = bench_stepper(args, "mobile", rank, local_rank, world, dev, K=200, W=100)
                else:
                    sub = bench_pixels(args, rank, local_rank, world, dev, K=4, W=1, phys_baseline=line.get("cpu_baseline"))
                sec[name] = {k: sub[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype", "roofline",
                                                  "cpu_baseline") if k in sub}
                sec[name]["workload"] = sub["config"]["workload"]
                if "kernel_ms" in sub["config"]:
                    sec[name]["kernel_ms"] = sub["config"]["kernel_ms"]
            except Exception as exc:          # a secondary leg must never sink the headline measurement
                sec[name] = {"value": None, "error": repr(exc)}
        args.img_size = saved_img
        # the rounds 1-2 lumped-gripper model on the same workload (round-3 advisor: the default moved to the full model without an
        # external pin — both are reported): a different, cheaper simulation, NOT the headline
        saved_model = args.kuka_model
        try:
            args.inner_steps = None
            args.kuka_model = "lumped"
            sub = bench_stepper(args, "kuka", rank, local_rank, world, dev, K=6, W=2, cpu=False)
            sec["kuka_lumped_model"] = {"value": sub["value"], "unit": sub["unit"], "steps": sub["steps"], "warmup": sub["warmup"], "ms_per_step": sub["ms_per_step"],
                                        "kernel": sub["roofline"]["kernel"], "workload": sub["config"]["workload"] + " (gripper welded to link 7: 7 DoF, 6 contact spheres, no friction rows)"}
        except Exception as exc:
            sec["kuka_lumped_model"] = {"value": None, "error": repr(exc)}
        finally:
            args.kuka_model, args.inner_steps = saved_model, saved
        # the per-step VecEnv API (what rl_baselines.train drives: rl_baselines/utils.py:213-229), steady state (every env past its first
        # episode), the reference's MT19937 streams: persistent stepping with the launching path's figure beside it
        try:
            import copy
            a = copy.copy(args)
            a.workload, a.persistent, a.device_ids, a.steps, a.warmup, a.rng = "kuka", True, None, 1000, 1100, "mt19937"
            sub = bench_per_step(a, emit=False)
            sec["per_step_api"] = {"metric": sub["metric"], "value": sub["value"], "unit": sub["unit"], "steps": sub["steps"], "warmup": sub["warmup"],
                                   "ms_per_step": sub["ms_per_step"], "us_per_step_median": sub["config"]["per_step"]["us_per_step_median"],
                                   "launch_per_step": sub["config"]["launch_per_step"], "workload": sub["config"]["workload"]}
        except Exception as exc:
            sec["per_step_api"] = {"value": None, "error": repr(exc)}
        line["secondary"] = sec
    if rank == 0:
        print(json.dumps(line))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
