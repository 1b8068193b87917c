"""Recorded JPEG frames from disk to device frames without decoding them on the host: the files' bytes are uploaded as they are and
decoded by srlhip_jpeg_decode (csrc/jpeg_decode.hip).  Only the streams this library's encoder writes (`dataset_generator
--device-jpeg`, Handle.render_jpeg) are accepted; every other JPEG is refused by name and stays Pillow's to read."""
import numpy as np

from . import _lib


def read_streams(paths):
    """-> (list of bytes, (h, w)); ValueError naming the first file that is not in the accepted format or differs in size"""
    streams, shape = [], None
    for p in paths:
        with open(p, "rb") as f:
            data = f.read()
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


def decode_streams(streams, shape, device, n_channels=3, names=None):
    """list of bytes of one (h, w) -> uint8 device tensor [len(streams) * 3 / n_channels][h][w][n_channels]: one blob and one offsets
    array uploaded, one srlhip_jpeg_decode call.  n_channels = 6 pairs streams 2i, 2i + 1 into frame i.  A stream whose status is not 0
    raises ValueError (naming names[s] when given)."""
    import torch
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
        work = torch.empty((_lib.jpeg_decode_workspace_bytes(ns, h, w),), dtype=torch.uint8, device=device)
        rc = _lib.jpeg_decode(blob_d.data_ptr(), offsets_d.data_ptr(), ns, h, w, n_channels, images.data_ptr(), status.data_ptr(),
                              work.data_ptr(), device_id=device.index, stream=torch.cuda.current_stream(device).cuda_stream)
        if rc:
            raise _lib.SrlHipError("srlhip_jpeg_decode failed ({})".format(rc))
        st = status.cpu().numpy()
    if st.any():
        s = int(np.flatnonzero(st)[0])
        raise ValueError("{}: JPEG stream did not decode (status {}; {} of {} streams failed)".format(
            names[s] if names is not None else "stream {}".format(s), int(st[s]), int((st != 0).sum()), ns))
    return images


def decode_files(paths, device, n_channels=3):
    """the JPEG files `paths` -> uint8 device tensor [len(paths) * 3 / n_channels][h][w][n_channels], decoded on `device`"""
    paths = list(paths)
    streams, shape = read_streams(paths)
    if not streams:
        raise ValueError("decode_files: no files")
    return decode_streams(streams, shape, device, n_channels=n_channels, names=paths)
