"""Recorded JPEG frames from disk to device frames without decoding them on the host: the files' bytes are uploaded as they are and
decoded by srlhip_jpeg_decode (csrc/jpeg_decode.hip).  With accept="own" (the default) only the streams this library's encoder writes
(`dataset_generator --device-jpeg`, Handle.render_jpeg) are accepted; every other JPEG is refused by name and stays Pillow's to read.
With accept="baseline" the files go through srlhip_jpeg_decode_baseline (csrc/jpeg_baseline.hip) instead, which reads what libjpeg writes
by default — Pillow's save(), cv2.imwrite, 4:2:0 or 4:4:4, the standard Huffman tables — and the library's own streams as well."""
import numpy as np

from . import _lib


ACCEPT = ("own", "baseline")
# per class (0 DC, 1 AC) what a DHT segment holds for the Annex K.3 luminance and chrominance tables: 16 BITS, then HUFFVAL; cut out of
# the header the library's own encoder writes (DHT DC0 AC0 DC1 AC1 behind SOI 2, APP0 18, DQT 2 x 69, SOF0 19 bytes)
_K3_TABLES = None


def _k3_tables():
    header = _lib.jpeg_encode_host(np.zeros((8, 8, 3), np.uint8), 50)[:_lib.jpeg_header_bytes()]
    at, tables = 2 + 18 + 2 * 69 + 19, ([], [])
    for _ in range(4):
        length = int.from_bytes(header[at + 2:at + 4], "big")
        tables[header[at + 4] >> 4].append(bytes(header[at + 5:at + 2 + length]))
        at += 2 + length
    return tables


def baseline_refusal(data):
    """why srlhip_jpeg_probe_baseline refuses `data`, in words, for an error message (the probe decides; this only names the reason)"""
    global _K3_TABLES
    if _K3_TABLES is None:
        _K3_TABLES = _k3_tables()
    if data[:2] != b"\xff\xd8":
        return "not a JPEG stream"
    pos, names = 2, {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC9: "arithmetic coding", 0xCA: "progressive, arithmetic coding",
                     0xEE: "an Adobe APP14 segment"}
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        m, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + length]
        if m in names:
            return names[m]
        if m == 0xC0 and len(body) >= 6:
            if body[0] != 8:
                return "{}-bit samples".format(body[0])
            if body[5] != 3:
                return "greyscale" if body[5] == 1 else "{} components".format(body[5])
            sampling = [body[7 + 3 * c] for c in range(3) if 7 + 3 * c < len(body)]
            if sampling not in ([0x22, 0x11, 0x11], [0x11, 0x11, 0x11]):
                known = {(0x21, 0x11, 0x11): "4:2:2", (0x12, 0x11, 0x11): "4:4:0", (0x41, 0x11, 0x11): "4:1:1"}
                return "{} chroma subsampling".format(known.get(tuple(sampling), "/".join("{}x{}".format(v >> 4, v & 15) for v in sampling)))
            h, w = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            if not (8 <= h <= 1024 and 8 <= w <= 1024):
                return "sides {}x{} outside 8..1024".format(h, w)
        if m == 0xDB and any(body[i] >> 4 for i in range(0, len(body), 65)):
            return "16-bit quantisation tables"
        if m == 0xC4:
            while len(body) >= 17:
                n = 17 + sum(body[1:17])
                if body[0] >> 4 <= 1 and body[0] & 15 <= 1 and bytes(body[1:n]) not in _K3_TABLES[body[0] >> 4]:
                    return "optimised Huffman tables"
                body = body[n:]
        if m == 0xDA:
            break
        pos += 2 + length
    return "not the accepted baseline layout"


def read_streams(paths, accept="own"):
    """-> (list of bytes, (h, w)); ValueError naming the first file that is not in the accepted format (accept="baseline": and why) or
    differs in size"""
    if accept not in ACCEPT:
        raise ValueError("accept must be own or baseline")
    streams, shape = [], None
    for p in paths:
        with open(p, "rb") as f:
            data = f.read()
        if accept == "baseline":
            hw = _lib.jpeg_probe_baseline(data)
            if hw is None:
                raise ValueError("{}: not a JPEG stream srlhip_jpeg_decode_baseline reads: {} (read it with Pillow)".format(p, baseline_refusal(data)))
            hw = hw[:2]
        else:
            hw = _lib.jpeg_probe(data)
            if hw is None:
                raise ValueError("{}: not a JPEG stream of this library's encoder (read it with Pillow)".format(p))
        if shape is None:
            shape = hw
        if hw != shape:
            raise ValueError("{}: {}x{} frame among {}x{} frames".format(p, hw[0], hw[1], shape[0], shape[1]))
        streams.append(data)
    return streams, shape


def all_accepted(paths):
    """True when every file probes as accepted and all have one size (reads every file)"""
    try:
        read_streams(paths)
    except ValueError:
        return False
    return len(paths) > 0


def decode_streams(streams, shape, device, n_channels=3, names=None, accept="own"):
    """list of bytes of one (h, w) -> uint8 device tensor [len(streams) * 3 / n_channels][h][w][n_channels]: one blob and one offsets
    array uploaded, one srlhip_jpeg_decode call.  n_channels = 6 pairs streams 2i, 2i + 1 into frame i.  A stream whose status is not 0
    raises ValueError (naming names[s] when given).  accept="baseline": one srlhip_jpeg_decode_baseline call for all of them."""
    import torch
    if accept not in ACCEPT:
        raise ValueError("accept must be own or baseline")
    workspace_bytes, decode, call = ((_lib.jpeg_decode_workspace_bytes, _lib.jpeg_decode, "srlhip_jpeg_decode") if accept == "own" else
                                     (_lib.jpeg_decode_baseline_workspace_bytes, _lib.jpeg_decode_baseline, "srlhip_jpeg_decode_baseline"))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_streams needs a GPU device (got {})".format(device))
    device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
    h, w = shape
    ns, views = len(streams), n_channels // 3
    if n_channels not in (3, 6) or ns == 0 or ns % views:
        raise ValueError("decode_streams: {} streams for {}-channel frames".format(ns, n_channels))
    offsets = np.zeros(ns + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    blob = np.frombuffer(b"".join(streams), np.uint8)
    with torch.cuda.device(device):
        blob_d = torch.from_numpy(blob.copy()).to(device)
        offsets_d = torch.from_numpy(offsets).to(device)
        images = torch.empty((ns // views, h, w, n_channels), dtype=torch.uint8, device=device)
        status = torch.empty((ns,), dtype=torch.int32, device=device)
        work = torch.empty((workspace_bytes(ns, h, w),), dtype=torch.uint8, device=device)
        rc = decode(blob_d.data_ptr(), offsets_d.data_ptr(), ns, h, w, n_channels, images.data_ptr(), status.data_ptr(),
                    work.data_ptr(), device_id=device.index, stream=torch.cuda.current_stream(device).cuda_stream)
        if rc:
            raise _lib.SrlHipError("{} failed ({})".format(call, rc))
        st = status.cpu().numpy()
    if st.any():
        s = int(np.flatnonzero(st)[0])
        raise ValueError("{}: JPEG stream did not decode (status {}; {} of {} streams failed)".format(
            names[s] if names is not None else "stream {}".format(s), int(st[s]), int((st != 0).sum()), ns))
    return images


def decode_files(paths, device, n_channels=3, accept="own"):
    """the JPEG files `paths` -> uint8 device tensor [len(paths) * 3 / n_channels][h][w][n_channels], decoded on `device`"""
    paths = list(paths)
    streams, shape = read_streams(paths, accept=accept)
    if not streams:
        raise ValueError("decode_files: no files")
    return decode_streams(streams, shape, device, n_channels=n_channels, names=paths, accept=accept)
