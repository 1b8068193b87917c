"""GPU: srlhip_jpeg_decode / srlhip.jpeg_io / load_dataset_frames(backend="hip").  The kernels of csrc/jpeg_decode.hip are held byte for
byte to the host twin (srlhip_jpeg_decode_host: the same source on the CPU, which tests/test_jpeg_decode_cpu.py holds to the numpy
restatement of the contract and to Pillow); every buffer the call writes sits inside a larger allocation filled with a sentinel.  Every
shape is the smallest that still reaches its code path."""
import os

import numpy as np
import pytest
import torch

import jpeg_decode_ref as ref
from srlhip import _lib

pytestmark = pytest.mark.gpu
NOISE_SEED = 3
GUARD = 4096                # sentinel bytes in front of and behind every buffer the call writes (a multiple of the workspace's alignment)
_STREAM, _TWIN = {}, {}


def _stream(kind, h, w, q, seed=NOISE_SEED):
    key = (kind, h, w, q, seed)
    if key not in _STREAM:
        _STREAM[key] = _lib.jpeg_encode_host(ref.frame(kind, h, w, seed=seed), q)
    return _STREAM[key]


def _twin(data):
    """the host twin's frame of a stream, computed once per stream and never modified"""
    if data not in _TWIN:
        _TWIN[data] = _lib.jpeg_decode_host(data)
        _TWIN[data].setflags(write=False)
    return _TWIN[data]


def _decode(streams, h, w, c, blob_dev=None, offsets_dev=None):
    """srlhip_jpeg_decode on a list of streams (or on a blob that already lies on the device) -> (rc, frames [n][h][w][c], status);
    asserts that the sentinels around the frames, the status words and the workspace are intact"""
    ns = len(streams)
    if blob_dev is None:
        offsets = np.zeros(ns + 1, np.int64)
        np.cumsum([len(s) for s in streams], out=offsets[1:])
        # the blob is followed by sentinel bytes of its own: a read past a stream would find 0xFF 0xD9 markers there
        blob_dev = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\xff\xd9" * 64, np.uint8).copy()).cuda()
        offsets_dev = torch.from_numpy(offsets).cuda()
    n_img, n_work = ns * 3 // c * h * w * c, _lib.jpeg_decode_workspace_bytes(ns, h, w)
    assert n_work > 0
    images = torch.full((n_img + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.full((n_work + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((ns + 16,), -7, dtype=torch.int32, device="cuda")
    assert (work.data_ptr() + GUARD) % 16 == 0
    rc = _lib.jpeg_decode(blob_dev.data_ptr(), offsets_dev.data_ptr(), ns, h, w, c, images.data_ptr() + GUARD, status.data_ptr() + 32,
                          work.data_ptr() + GUARD, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    images, work, status = images.cpu().numpy(), work.cpu().numpy(), status.cpu().numpy()
    assert (images[:GUARD] == 0xA5).all() and (images[GUARD + n_img:] == 0xA5).all(), "bytes outside the frames were written"
    assert (work[:GUARD] == 0x5A).all() and (work[GUARD + n_work:] == 0x5A).all(), "bytes outside the workspace were written"
    assert (status[:8] == -7).all() and (status[8 + ns:] == -7).all(), "words outside status were written"
    return rc, images[GUARD:GUARD + n_img].reshape(ns * 3 // c, h, w, c), status[8:8 + ns]


def _frames_of(streams, h, w, c):
    views = c // 3
    return np.stack([np.concatenate([_twin(s) for s in streams[views * i:views * (i + 1)]], axis=2) for i in range(len(streams) // views)])


# (h, w, c, n streams): one MCU, all padding; the smallest multi-stream case; crop in both directions, 2 x 3 MCUs; more streams than a
# wavefront has lanes and an uneven last group; 196 MCUs (the marker index wraps mod 8 24 times), two views into one 6-channel frame
@pytest.mark.parametrize("h,w,c,n,qualities", [(8, 8, 3, 1, (95,)), (16, 16, 3, 3, (95,)), (24, 40, 3, 2, (95,)), (64, 64, 3, 65, (95, 10)),
                                               (224, 224, 6, 2, (95,))])
def test_device_equals_the_twin_byte_for_byte(h, w, c, n, qualities):
    # stream s shows kind (s + r) mod 6: every call mixes the kinds; calls with fewer than 6 streams take several rounds to show all
    rounds = range(0, 6, n) if n < 6 else (0,)
    for q in qualities:
        for r in rounds:
            streams = [_stream(ref.KINDS[(s + r) % 6], h, w, q, seed=NOISE_SEED + s // 6) for s in range(n)]
            rc, frames, status = _decode(streams, h, w, c)
            assert rc == 0 and not status.any(), (q, r, status)
            want = _frames_of(streams, h, w, c)
            for i in range(len(want)):
                assert np.array_equal(frames[i], want[i]), (q, r, i)


def test_mixed_call_refuses_four_streams_and_decodes_the_rest():
    """A test of refusal; it must not fault.  Of 8 streams one is empty (status 2), one carries the header of another frame size (1), one
    is cut inside an MCU (3) and one has lost a marker (3): their frames are zeros, the other four equal the twin.  One of those four
    carries ANOTHER QUALITY's header in front of its own data: the contract reads the table values and does not assume them, so that
    header is the accepted layout and the stream decodes — with the tables it carries, exactly as the twin decodes the same bytes."""
    h = w = 64
    good = [_stream(ref.KINDS[s % 6], h, w, 95) for s in range(8)]
    at = [i for i in range(629, len(good[5]) - 1) if good[5][i] == 0xFF and good[5][i + 1] != 0]
    streams = list(good)
    streams[1] = b""                                                                  # what an overflowed encode leaves
    streams[2] = _stream("noise", h, w, 50)[:629] + good[2][629:]                     # another quality's header: decodes (tables are read)
    streams[3] = _lib.jpeg_encode_host(ref.frame("noise", 48, 64), 95)                # another size's header
    streams[4] = good[4][:len(good[4]) // 2]                                          # cut inside an MCU
    streams[5] = good[5][:at[2]] + good[5][at[2] + 2:]                                # a marker removed
    rc, frames, status = _decode(streams, h, w, 3)
    assert rc == 0 and status.tolist() == [0, 2, 0, 1, 3, 3, 0, 0]
    for s in (1, 3, 4, 5):
        assert not frames[s].any(), s
    for s in (0, 2, 6, 7):
        assert np.array_equal(frames[s], _twin(streams[s])), s


def test_single_damaged_bytes_are_refused_or_decode_like_the_twin():
    h = w = 64
    base = _stream("noise", h, w, 95)
    streams, want = [], []
    for pos in (629, 700, len(base) // 2, len(base) - 3):
        for value in (0x00, 0xFF):
            d = bytearray(base)
            d[pos] = value
            streams.append(bytes(d))
            want.append(_lib.jpeg_decode_host(bytes(d), return_status=True))
    rc, frames, status = _decode(streams, h, w, 3)
    assert rc == 0
    for s, (frame, st) in enumerate(want):
        assert status[s] == st and np.array_equal(frames[s], frame), s


def _handle(kind):
    cfg = _lib.default_config(kind)
    cfg.num_envs, cfg.seed0, cfg.rng_mode, cfg.auto_reset, cfg.io_device = 4, 5, _lib.RNG_MT19937, 1, 1
    cfg.img_h = cfg.img_w = 64
    return _lib.Handle(cfg)


@pytest.mark.parametrize("kind", [_lib.ENV_KUKA_BUTTON, _lib.ENV_MOBILE])
def test_round_trip_on_rendered_frames_where_the_blob_lies(kind):
    """srlhip_render_jpeg on a device-pointer handle, then srlhip_jpeg_decode of that blob without it leaving the device"""
    hd = _handle(kind)
    n, cap = hd.num_envs, 629 + 64 * 64 * 3
    blob = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    offsets, overflow = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    obs = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")            # (room for any env's observation of 4 envs)
    hd.reset(obs_out=obs.data_ptr())
    rc = hd._lib.srlhip_render_jpeg(hd._h, 95, blob.data_ptr(), blob.numel(), offsets.data_ptr(), overflow.data_ptr())
    assert rc == 0
    hd.sync()
    assert not overflow.cpu().numpy().any()
    streams = _lib.split_streams(blob.cpu().numpy(), offsets.cpu().numpy(), overflow.cpu().numpy())
    rc, frames, status = _decode(streams, 64, 64, 3, blob_dev=blob, offsets_dev=offsets)
    assert rc == 0 and not status.any()
    for s in range(n):
        assert _lib.jpeg_probe(streams[s]) == (64, 64)
        assert np.array_equal(frames[s], _lib.jpeg_decode_host(streams[s])), s
    hd.close()


def test_decode_refuses_bad_arguments():
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    off, st = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    call = lambda h, w, c, n=2, blob=p, offs=off.data_ptr(), img=p + 16384, status=st.data_ptr(), work=p + 32768: _lib.jpeg_decode(      # noqa: E731
        blob, offs, n, h, w, c, img, status, work)
    for bad in ((16, 16, 4), (7, 16, 3), (16, 1025, 3), (1025, 16, 6)):
        assert call(*bad) == -22, bad
    assert call(16, 16, 6, n=3) == -22 and call(16, 16, 3, n=-1) == -22
    for name in ("blob", "offs", "img", "status", "work"):
        assert call(16, 16, 3, **{name: 0}) == -22, name
    assert call(16, 16, 3, work=p + 32768 + 4) == -22                      # the workspace is 16-byte aligned
    assert call(16, 16, 3) == 0                                            # two empty streams
    torch.cuda.synchronize()
    assert st.cpu().numpy()[:2].tolist() == [2, 2]


def _write_dataset(root, n=32):
    folder = os.path.join(root, "record_000")
    os.makedirs(folder)
    streams = [_stream(ref.KINDS[i % 6] if i % 6 != 1 else "noise", 16, 16, 95, seed=NOISE_SEED + i) for i in range(n)]
    for i, data in enumerate(streams):
        with open(os.path.join(folder, "frame{:06d}.jpg".format(i)), "wb") as f:
            f.write(data)
    return streams


def test_dataset_path_decodes_on_the_device_and_fits_the_same_model(tmp_path):
    from state_representation import pca_fit
    streams = _write_dataset(str(tmp_path))
    want = np.stack([_twin(s) for s in streams])
    frames = pca_fit.load_dataset_frames(str(tmp_path), backend="hip")
    assert isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8
    assert np.array_equal(frames.cpu().numpy(), want)
    auto = pca_fit.load_dataset_frames(str(tmp_path), backend="auto")
    assert isinstance(auto, torch.Tensor) and np.array_equal(auto.cpu().numpy(), want)
    assert np.array_equal(pca_fit.load_dataset_frames(str(tmp_path)), want)          # the default: Pillow, numpy, the same frames
    a, b = pca_fit.fit_pca(frames, 4, backend="hip"), pca_fit.fit_pca(want, 4, backend="host")
    for name in ("components_", "mean_", "explained_variance_", "singular_values_"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    # the CLI, frames never decoded on the host
    path = pca_fit.main(["--data-folder", str(tmp_path), "--state-dim", "4", "--decode-backend", "hip", "--backend", "hip", "--log-folder", str(tmp_path / "log")])
    import pickle
    with open(path, "rb") as f:
        assert np.array_equal(pickle.load(f).components_, b.components_)


def test_dataset_path_with_a_foreign_file_falls_back_or_names_it(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from state_representation import pca_fit
    streams = _write_dataset(str(tmp_path))
    foreign = os.path.join(str(tmp_path), "record_000", "frame000007.jpg")
    Image.fromarray(ref.frame("gradient", 16, 16)).save(foreign, format="JPEG", quality=95)
    auto = pca_fit.load_dataset_frames(str(tmp_path), backend="auto")
    assert isinstance(auto, np.ndarray) and auto.shape == (32, 16, 16, 3)
    assert np.array_equal(auto[6], _twin(streams[6])) and np.array_equal(auto[7], np.asarray(Image.open(foreign).convert("RGB")))
    with pytest.raises(ValueError, match="frame000007.jpg"):
        pca_fit.load_dataset_frames(str(tmp_path), backend="hip")


def test_decode_files_pairs_two_views_and_reports_a_damaged_file(tmp_path):
    from srlhip import jpeg_io
    paths = []
    for i, kind in enumerate(("quadrants", "noise", "gradient", "checker")):
        paths.append(str(tmp_path / "f{}.jpg".format(i)))
        with open(paths[-1], "wb") as f:
            f.write(_stream(kind, 24, 40, 95))
    six = jpeg_io.decode_files(paths, "cuda", n_channels=6)
    assert tuple(six.shape) == (2, 24, 40, 6)
    assert np.array_equal(six.cpu().numpy(), _frames_of([_stream(k, 24, 40, 95) for k in ("quadrants", "noise", "gradient", "checker")], 24, 40, 6))
    data = _stream("noise", 24, 40, 95)
    with open(paths[2], "wb") as f:
        f.write(data[:-40] + data[-2:])                                   # accepted by the probe, malformed behind the header
    with pytest.raises(ValueError, match="f2.jpg"):
        jpeg_io.decode_files(paths, "cuda")
