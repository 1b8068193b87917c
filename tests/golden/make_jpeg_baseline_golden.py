"""Writes tests/golden/jpeg_baseline_pillow.npz: JPEG streams as Pillow's save() writes them (libjpeg's defaults: the Annex K.3 Huffman
tables, 4:2:0 unless told otherwise, restart markers only on request) and PILLOW'S OWN DECODE of each, so that the tests of
srlhip_jpeg_decode_baseline need no Pillow where they run.  Run it from the repository's root with Pillow installed:
    python tests/golden/make_jpeg_baseline_golden.py
A case is named "h,w,kind,quality,subsampling,restart": kind as tests/jpeg_decode_ref.py's frame(), subsampling 2 (4:2:0) or 0 (4:4:4),
restart none / b1 / b3 (restart_marker_blocks) / r1 (restart_marker_rows=1).  The product of all settings is thinned: every size meets
every kind, and qualities, samplings and restart settings rotate through them; 64x64 additionally meets every sampling x quality x
restart setting once (the GPU test mixes them in one call).  "refused_<what>" are streams the decoder must refuse by its header
(a 64x64 gradient at quality 50 saved progressive, with optimised Huffman tables, as greyscale, with 4:2:2 subsampling): no frames."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_ref as ref  # noqa: E402

SIZES = ((8, 8), (9, 9), (16, 16), (24, 40), (33, 17), (64, 64))
QUALITIES = (10, 50, 95, 100)
RESTARTS = ("none", "b1", "b3", "r1")
NOISE_SEED = 3


def big_frame():
    """224x224: a gradient with a 32x32 patch of noise (small as a stream and as a deflated frame, yet with busy blocks)"""
    f = ref.frame("gradient", 224, 224).copy()
    f[96:128, 64:96] = np.random.RandomState(NOISE_SEED).randint(0, 256, size=(32, 32, 3))
    return f


def source_frame(kind, h, w):
    return big_frame() if kind == "gradient+noise" else ref.frame(kind, h, w, seed=NOISE_SEED)


def save(frame, quality, subsampling, restart):
    kw = {"none": {}, "b1": {"restart_marker_blocks": 1}, "b3": {"restart_marker_blocks": 3}, "r1": {"restart_marker_rows": 1}}[restart]
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def cases():
    out = []
    for i, (h, w) in enumerate(SIZES):
        for j, kind in enumerate(ref.KINDS):
            n = i + j
            out.append((h, w, kind, QUALITIES[n % 4], (0, 2)[(n // 2 + i) % 2], RESTARTS[(n + j // 4) % 4]))
    # 64x64: every sampling x quality x restart setting, the kinds rotating (noise only twice: it does not deflate)
    n = 0
    for sub in (2, 0):
        for q in QUALITIES:
            for r in RESTARTS:
                kind = ("gradient", "quadrants", "checker", "black", "white")[n % 5] if n not in (6, 27) else "noise"
                out.append((64, 64, kind, q, sub, r))
                n += 1
    out += [(8, 8, "noise", 95, 0, "none"), (9, 9, "noise", 95, 2, "none"), (9, 9, "quadrants", 95, 2, "b1"), (33, 17, "quadrants", 95, 2, "none"),
            (24, 40, "noise", 95, 2, "b1"), (24, 40, "noise", 95, 0, "b3"), (24, 40, "quadrants", 50, 2, "b3"), (24, 40, "gradient", 95, 0, "b1"),
            (16, 16, "checker", 100, 2, "b1"), (16, 16, "checker", 100, 0, "none"), (16, 16, "noise", 95, 0, "b1"),
            (224, 224, "gradient+noise", 95, 2, "none")]
    seen, unique = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            unique.append(c)
    return unique


def main():
    arrays, names = {}, []
    for i, (h, w, kind, q, sub, r) in enumerate(cases()):
        data = save(source_frame(kind, h, w), q, sub, r)
        names.append("{},{},{},{},{},{}".format(h, w, kind, q, sub, r))
        arrays["stream_{}".format(i)] = np.frombuffer(data, np.uint8)
        arrays["frame_{}".format(i)] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)
    f = ref.frame("gradient", 64, 64)
    for what, image, kw in (("progressive", f, {"progressive": True}), ("optimised", f, {"optimize": True}), ("greyscale", f[:, :, 0], {}),
                            ("422", f, {"subsampling": 1})):
        buf = io.BytesIO()
        Image.fromarray(image).save(buf, format="JPEG", quality=50, **kw)
        arrays["refused_" + what] = np.frombuffer(buf.getvalue(), np.uint8)
    path = os.path.join(HERE, "jpeg_baseline_pillow.npz")
    np.savez_compressed(path, names=np.array(names), **arrays)
    print("{}: {} cases, {} bytes".format(path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
