"""Microbenchmark of the device JPEG encoder (csrc/jpeg.hip) in the style of profiles/encoder_microbench.py: srlhip_jpeg_encode on
4096 rasterised KukaButton frames at 64x64x3 and 224x224x3, timed with HIP events on the stream after a warm-up, beside what the
recorder paid for the same frames before: the device-to-host copy of the raw batch and Pillow's save(quality=95) per frame on one host
core.  --end-to-end adds dataset_generator on MobileRobot (256 lanes, 256 episodes, 224x224) with and without --device-jpeg.
Prints one JSON line per measurement."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "robotics-rl-srl_amd"))


def frames_of(n, size):
    from srlhip import _lib
    cfg = _lib.default_config(_lib.ENV_KUKA_BUTTON)
    cfg.num_envs, cfg.seed0, cfg.rng_mode = n, 1, _lib.RNG_PHILOX
    cfg.img_h = cfg.img_w = size
    h = _lib.Handle(cfg)
    h.reset()
    acts = np.random.RandomState(0).randint(6, size=(20, n)).astype(np.int32)
    for t in range(20):
        h.step(acts[t])
    out = h.render()
    h.close()
    return out


def event_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def microbench(n, size, reps, warmup):
    import torch
    from PIL import Image
    from srlhip import _lib
    host = frames_of(n, size)
    img = torch.from_numpy(host).cuda()
    cap = 1024 + size * size * 3
    blob = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    off, ovf = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def encode():
        rc = _lib.jpeg_encode(img.data_ptr(), n, size, size, 3, 95, blob.data_ptr(), cap, off.data_ptr(), ovf.data_ptr(), stream=stream)
        assert rc == 0, rc
    enc = event_ms(encode, reps, warmup)
    total = int(off[-1].item())
    assert not bool(ovf.any().item())
    pinned = torch.empty_like(img, device="cpu").pin_memory()
    d2h_raw = event_ms(lambda: pinned.copy_(img, non_blocking=True), reps, warmup)
    pinned_blob = torch.empty(total, dtype=torch.uint8).pin_memory()
    d2h_jpeg = event_ms(lambda: pinned_blob.copy_(blob[:total], non_blocking=True), reps, warmup)
    k = min(n, 256)
    t0 = time.perf_counter()
    sizes = []
    for i in range(k):
        buf = io.BytesIO()
        Image.fromarray(host[i]).save(buf, format="JPEG", quality=95)
        sizes.append(buf.tell())
    pillow_ms = (time.perf_counter() - t0) * 1e3 / k
    print(json.dumps({"what": "srlhip_jpeg_encode", "frames": n, "size": size, "quality": 95, "encode_ms_median_min_max": enc,
                      "frames_per_s": n / enc[0] * 1e3, "jpeg_bytes_per_frame": total / n, "pillow_bytes_per_frame": float(np.mean(sizes)),
                      "raw_batch_bytes": int(host.nbytes), "d2h_raw_batch_ms": d2h_raw, "d2h_jpeg_blob_ms": d2h_jpeg,
                      "pillow_ms_per_frame_one_core": pillow_ms, "pillow_ms_whole_batch_one_core": pillow_ms * n}), flush=True)


def end_to_end(lanes, episodes, size):
    from environments import dataset_generator as dg
    for flag in ([], ["--device-jpeg"], [], ["--device-jpeg"]):          # alternating, twice each
        root = tempfile.mkdtemp() + "/"
        t0 = time.perf_counter()
        args = ["--env", "MobileRobotGymEnv-v0", "--num-cpu", str(lanes), "--num-episode", str(episodes), "--img-size", str(size),
                "--save-path", root, "--name", "d", "--seed", "0"] + flag
        with open(os.devnull, "w") as null:
            old, sys.stdout = sys.stdout, null
            try:
                parsed = dg.build_parser().parse_args(args)
                parsed.seed = np.random.RandomState(parsed.seed).randint(int(1e10))
                os.makedirs(root + "d")
                fps = dg.run_batched(parsed)
            finally:
                sys.stdout = old
        n_jpg = sum(f.endswith(".jpg") for _, _, fs in os.walk(root) for f in fs)
        print(json.dumps({"what": "dataset_generator", "device_jpeg": bool(flag), "lanes": lanes, "episodes": episodes, "size": size,
                          "frames_per_s": fps, "jpg_files": n_jpg, "wall_s": time.perf_counter() - t0}), flush=True)
        shutil.rmtree(root)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 224])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--lanes", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=256)
    a = ap.parse_args()
    import torch  # noqa: F401  (before libsrlhip.so: whichever HIP runtime is loaded first serves the process)
    for size in a.sizes:
        microbench(a.frames, size, a.reps, a.warmup)
    if a.end_to_end:
        end_to_end(a.lanes, a.episodes, 224)
