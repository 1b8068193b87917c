"""Microbenchmark of the device JPEG decoder (csrc/jpeg_decode.hip) in the style of profiles/jpeg_microbench.py: 4096 rasterised
KukaButton frames at 64x64x3 and 224x224x3 are encoded on the device (srlhip_jpeg_encode, quality 95) and the blob decoded where it
lies by srlhip_jpeg_decode, timed with HIP events on the stream after a warm-up (median, min, max over --reps calls), beside Pillow's
decode of the same streams on one host core of the same machine.  The decoded frames are compared with the host twin on a sample of
streams first.  The per-launch split comes from a separate run under `rocprofv3 --kernel-trace --stats` (profiles/NOTES.md).
Prints one JSON line per size."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "robotics-rl-srl_amd"))

from jpeg_microbench import event_ms, frames_of  # noqa: E402


def microbench(n, size, reps, warmup, pillow_frames):
    import torch
    from PIL import Image
    from srlhip import _lib
    img = torch.from_numpy(frames_of(n, size)).cuda()
    cap = 1024 + size * size * 3
    blob = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    off, ovf = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.jpeg_encode(img.data_ptr(), n, size, size, 3, 95, blob.data_ptr(), cap, off.data_ptr(), ovf.data_ptr(), stream=stream) == 0
    torch.cuda.synchronize()
    assert not bool(ovf.any().item())
    total = int(off[-1].item())
    work_bytes = _lib.jpeg_decode_workspace_bytes(n, size, size)
    out = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")

    def decode():
        rc = _lib.jpeg_decode(blob.data_ptr(), off.data_ptr(), n, size, size, 3, out.data_ptr(), status.data_ptr(), work.data_ptr(), stream=stream)
        assert rc == 0, rc
    dec = event_ms(decode, reps, warmup)
    assert not bool(status.any().item())
    # what the timed call computed, against the host twin and Pillow on the same bytes
    offsets, host_blob = off.cpu().numpy(), blob[:total].cpu().numpy()
    streams = [host_blob[offsets[s]:offsets[s + 1]].tobytes() for s in range(n)]
    got = out.cpu().numpy()
    for s in range(0, n, max(1, n // 16)):
        assert np.array_equal(got[s], _lib.jpeg_decode_host(streams[s])), s
    k = min(n, pillow_frames)
    t0 = time.perf_counter()
    for s in range(k):
        frame = np.asarray(Image.open(io.BytesIO(streams[s])).convert("RGB"))
    pillow_ms = (time.perf_counter() - t0) * 1e3 / k
    assert np.array_equal(frame, got[k - 1])
    mcus = n * ((size + 15) // 16) ** 2
    # bytes the four launches and the memset move, from the shapes: the stream bytes are read by the scan and by the entropy decode;
    # coefficients zeroed (768 B / MCU), written sparsely and read once; planes (384 B / MCU) written once and read by the pixel pass
    moved = {"stream_bytes_read": 2 * total, "coef_bytes_zeroed": 768 * mcus, "coef_bytes_read": 768 * mcus, "plane_bytes_written": 384 * mcus,
             "plane_bytes_read": 384 * mcus, "frame_bytes_written": int(out.numel())}
    print(json.dumps({"what": "srlhip_jpeg_decode", "frames": n, "size": size, "quality": 95, "decode_ms_median_min_max": dec,
                      "frames_per_s": n / dec[0] * 1e3, "jpeg_bytes_per_frame": total / n, "workspace_bytes": work_bytes, "bytes_moved": moved,
                      "effective_gb_per_s": sum(moved.values()) / dec[0] / 1e6, "pillow_ms_per_frame_one_core": pillow_ms,
                      "pillow_ms_whole_batch_one_core": pillow_ms * n, "pillow_frames_timed": k}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 224])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pillow-frames", type=int, default=1024)
    a = ap.parse_args()
    import torch  # noqa: F401  (before libsrlhip.so: whichever HIP runtime is loaded first serves the process)
    for size in a.sizes:
        microbench(a.frames, size, a.reps, a.warmup, a.pillow_frames)
