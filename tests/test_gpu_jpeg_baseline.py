"""GPU: srlhip_jpeg_decode_baseline / srlhip.jpeg_io(accept="baseline") / load_dataset_frames(backend="hip-baseline").  The kernels of
csrc/jpeg_baseline.hip are held byte for byte to the host twin (srlhip_jpeg_decode_baseline_host: the same source on the CPU, which
tests/test_jpeg_baseline_cpu.py holds to the restatement of the contract and to Pillow's own frames); every buffer the call writes sits
inside a larger allocation filled with a sentinel.  The streams are Pillow's, read from tests/golden/jpeg_baseline_pillow.npz: no Pillow
is needed here.  Every shape is the smallest that still reaches its code path."""
import os
import pickle

import numpy as np
import pytest
import torch

import jpeg_baseline_ref as bref
import jpeg_decode_ref as ref
from srlhip import _lib

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                # sentinel bytes in front of and behind every buffer the call writes (a multiple of the workspace's alignment)
_TWIN = {}


@pytest.fixture(scope="module")
def cases():
    return bref.load_fixture(os.path.join(REPO, "tests", "golden", "jpeg_baseline_pillow.npz"))


@pytest.fixture(scope="module")
def refused():
    return bref.load_refused(os.path.join(REPO, "tests", "golden", "jpeg_baseline_pillow.npz"))


def _twin(data, h, w):
    """(frame, status) of the host twin for a call of sides h x w, computed once per stream and never modified"""
    key = (data, h, w)
    if key not in _TWIN:
        _TWIN[key] = _lib.jpeg_decode_baseline_host(data, shape=(h, w), return_status=True)
        _TWIN[key][0].setflags(write=False)
    return _TWIN[key]


def _decode(streams, h, w, c, call=None, workspace_bytes=None):
    """srlhip_jpeg_decode_baseline (or `call`) on a list of streams -> (rc, frames [n][h][w][c], status); asserts that the sentinels around the
    frames, the status words and the workspace are intact"""
    call, workspace_bytes = call or _lib.jpeg_decode_baseline, workspace_bytes or _lib.jpeg_decode_baseline_workspace_bytes
    ns = len(streams)
    offsets = np.zeros(ns + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    # the blob is followed by sentinel bytes of its own: a read past a stream would find 0xFF 0xD9 markers there
    blob_dev = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\xff\xd9" * 64, np.uint8).copy()).cuda()
    offsets_dev = torch.from_numpy(offsets).cuda()
    n_img, n_work = ns * 3 // c * h * w * c, workspace_bytes(ns, h, w)
    assert n_work > 0
    images = torch.full((n_img + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.full((n_work + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((ns + 16,), -7, dtype=torch.int32, device="cuda")
    assert (work.data_ptr() + GUARD) % 16 == 0
    rc = call(blob_dev.data_ptr(), offsets_dev.data_ptr(), ns, h, w, c, images.data_ptr() + GUARD, status.data_ptr() + 32,
              work.data_ptr() + GUARD, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    images, work, status = images.cpu().numpy(), work.cpu().numpy(), status.cpu().numpy()
    assert (images[:GUARD] == 0xA5).all() and (images[GUARD + n_img:] == 0xA5).all(), "bytes outside the frames were written"
    assert (work[:GUARD] == 0x5A).all() and (work[GUARD + n_work:] == 0x5A).all(), "bytes outside the workspace were written"
    assert (status[:8] == -7).all() and (status[8 + ns:] == -7).all(), "words outside status were written"
    return rc, images[GUARD:GUARD + n_img].reshape(ns * 3 // c, h, w, c), status[8:8 + ns]


def _check_against_twin(streams, h, w, c):
    rc, frames, status = _decode(streams, h, w, c)
    assert rc == 0
    views = c // 3
    for s, data in enumerate(streams):
        frame, st = _twin(data, h, w)
        assert status[s] == st, (s, status[s], st)
        assert np.array_equal(frames[s // views][:, :, 3 * (s % views):3 * (s % views) + 3], frame), s
    return status


def test_one_444_mcu(cases):
    c = bref.pick(cases, h=8, w=8, subsampling=0)
    assert not _check_against_twin([c["stream"]], 8, 8, 3).any()
    assert np.array_equal(_twin(c["stream"], 8, 8)[0], c["frame"])           # and the twin's frame is Pillow's


def test_one_420_mcu_all_padding(cases):
    for c in (k for k in cases if (k["h"], k["w"], k["subsampling"]) == (9, 9, 2)):
        assert not _check_against_twin([c["stream"]], 9, 9, 3).any(), c["name"]


def test_two_streams_with_restart_intervals_1_and_3(cases):
    a, b = bref.pick(cases, h=24, w=40, kind="noise", restart="b1"), bref.pick(cases, h=24, w=40, kind="noise", restart="b3")
    assert (bref.parse(a["stream"])["ri"], bref.parse(b["stream"])["ri"]) == (1, 3)
    assert not _check_against_twin([a["stream"], b["stream"]], 24, 40, 3).any()


def test_65_streams_mixing_samplings_qualities_and_restart_settings(cases):
    """more streams than a wavefront has lanes, an uneven last group; both samplings, the four qualities and every restart setting"""
    pool = [c for c in cases if (c["h"], c["w"]) == (64, 64)]
    assert {(c["subsampling"], c["quality"], c["restart"]) for c in pool} >= {(s, q, r) for s in (2, 0) for q in (10, 50, 95, 100)
                                                                               for r in ("none", "b1", "b3", "r1")}
    streams = [pool[(7 * i) % len(pool)]["stream"] for i in range(65)]       # 7 and the pool's size are coprime: neighbours differ
    assert len(set(streams)) == len(pool)
    assert not _check_against_twin(streams, 64, 64, 3).any()
    for c in pool:
        assert np.array_equal(_twin(c["stream"], 64, 64)[0], c["frame"]), c["name"]


@pytest.mark.parametrize("lanes", ["64", "16", "4", "5"])
def test_every_setting_of_the_lanes_override_gives_the_same_frames(cases, refused, lanes, monkeypatch):
    """SRLHIP_JPEG_BASELINE_LANES (include/srlhip.h): 64 and 16 active lanes per wavefront take other launch shapes and more dynamic LDS
    than the built-in 4; a value that is not one of the three is ignored.  69 streams: more than one wavefront's at 64 lanes, more
    than one workgroup's at 16, an uneven last group at each; three of them refused."""
    monkeypatch.setenv("SRLHIP_JPEG_BASELINE_LANES", lanes)
    pool = [c for c in cases if (c["h"], c["w"]) == (64, 64)]
    streams = [pool[(5 * i) % len(pool)]["stream"] for i in range(69)]
    streams[3], streams[40], streams[68] = refused["optimised"], b"", streams[68][:-40]
    status = _check_against_twin(streams, 64, 64, 3)
    assert [int(status[i]) for i in (3, 40, 68)] == [1, 2, 3] and int((status != 0).sum()) == 3


def test_two_224_streams_into_one_six_channel_frame(cases):
    """Pillow's stream (no restarts) and the library's own of the same size (Ri = 1) as the two views of one frame"""
    c = bref.pick(cases, h=224, w=224)
    own = _lib.jpeg_encode_host(ref.frame("noise", 224, 224, seed=3), 95)
    assert not _check_against_twin([c["stream"], own], 224, 224, 6).any()
    assert np.array_equal(_twin(c["stream"], 224, 224)[0], c["frame"]) and np.array_equal(_twin(own, 224, 224)[0], _lib.jpeg_decode_host(own))


def test_mixed_call_refuses_five_streams_and_decodes_the_rest(cases, refused):
    """A test of refusal; it must not fault.  Of 8 streams one is empty (status 2), one progressive (1), one carries another size's header
    (1), one is cut inside the data (3) and one has lost a restart marker (3): their frames are zeros, the other three equal the twin."""
    pool = [c for c in cases if (c["h"], c["w"]) == (64, 64)]
    good = [bref.pick(pool, subsampling=2, restart="none", quality=95), bref.pick(pool, subsampling=0, restart="b3", quality=50),
            bref.pick(pool, subsampling=2, restart="r1", quality=100)]
    b1 = bref.pick(pool, subsampling=2, restart="b1", quality=50)["stream"]
    start = bref.parse(b1)["data_start"]
    at = [i for i in range(start, len(b1) - 2) if b1[i] == 0xFF and 0xD0 <= b1[i + 1] <= 0xD7]
    streams = [good[0]["stream"], b"", refused["progressive"], bref.pick(cases, h=24, w=40)["stream"], b1[:(start + len(b1)) // 2],
               b1[:at[2]] + b1[at[2] + 2:], good[1]["stream"], good[2]["stream"]]
    rc, frames, status = _decode(streams, 64, 64, 3)
    assert rc == 0 and status.tolist() == [0, 2, 1, 1, 3, 3, 0, 0]
    for s in (1, 2, 3, 4, 5):
        assert not frames[s].any(), s
    for s, c in ((0, good[0]), (6, good[1]), (7, good[2])):
        assert np.array_equal(frames[s], _twin(streams[s], 64, 64)[0]) and np.array_equal(frames[s], c["frame"]), s


def test_single_damaged_bytes_are_refused_or_decode_like_the_twin(cases):
    base = bref.pick(cases, h=16, w=16, subsampling=0, restart="b1", kind="noise")
    status = _check_against_twin([data for _, _, data in bref.damaged(base["stream"])], 16, 16, 3)
    assert set(status.tolist()) == {0, 1, 3}


@pytest.mark.parametrize("h,w", [(64, 64), (24, 40)])
def test_own_streams_decode_as_through_the_own_decoder(h, w):
    streams = [_lib.jpeg_encode_host(ref.frame(ref.KINDS[s % 6], h, w, seed=3 + s), (95, 10)[s % 2]) for s in range(7)]
    rc, frames, status = _decode(streams, h, w, 3)
    rc2, frames2, status2 = _decode(streams, h, w, 3, call=_lib.jpeg_decode, workspace_bytes=_lib.jpeg_decode_workspace_bytes)
    assert rc == 0 and rc2 == 0 and not status.any() and not status2.any()
    assert np.array_equal(frames, frames2)


def test_decode_refuses_bad_arguments():
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    off, st = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    call = lambda h, w, c, n=2, blob=p, offs=off.data_ptr(), img=p + 16384, status=st.data_ptr(), work=p + 32768: _lib.jpeg_decode_baseline(      # noqa: E731
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


def _write_dataset(root, cases):
    """a folder of Pillow's files plus two of the library's encoder -> (streams, frames)"""
    folder = os.path.join(root, "record_000")
    os.makedirs(folder)
    pool = [c for c in cases if (c["h"], c["w"]) == (16, 16)]
    streams, frames = [c["stream"] for c in pool], [c["frame"] for c in pool]
    for kind in ("noise", "quadrants"):
        streams.append(_lib.jpeg_encode_host(ref.frame(kind, 16, 16, seed=9), 95))
        frames.append(_lib.jpeg_decode_host(streams[-1]))
    for i, data in enumerate(streams):
        with open(os.path.join(folder, "frame{:06d}.jpg".format(i)), "wb") as f:
            f.write(data)
    return streams, np.stack(frames)


def test_dataset_path_decodes_pillows_files_on_the_device_and_fits_the_same_model(tmp_path, cases, refused):
    from state_representation import pca_fit
    streams, want = _write_dataset(str(tmp_path), cases)
    assert len(streams) >= 8
    frames = pca_fit.load_dataset_frames(str(tmp_path), backend="hip-baseline")
    assert isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8
    assert np.array_equal(frames.cpu().numpy(), want)
    assert np.array_equal(want, np.stack([_twin(s, 16, 16)[0] for s in streams]))
    a, b = pca_fit.fit_pca(frames, 4, backend="hip"), pca_fit.fit_pca(want, 4, backend="host")
    for name in ("components_", "mean_", "explained_variance_", "singular_values_"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    path = pca_fit.main(["--data-folder", str(tmp_path), "--state-dim", "4", "--decode-backend", "hip-baseline", "--backend", "hip",
                         "--log-folder", str(tmp_path / "log")])
    with open(path, "rb") as f:
        assert np.array_equal(pickle.load(f).components_, b.components_)
    # the old behaviour is intact: backend="hip" still refuses Pillow's file by name
    with pytest.raises(ValueError, match="frame000000.jpg"):
        pca_fit.load_dataset_frames(str(tmp_path), backend="hip")
    # a progressive file in the folder is named
    with open(os.path.join(str(tmp_path), "record_000", "frame000003.jpg"), "wb") as f:
        f.write(refused["progressive"])
    with pytest.raises(ValueError, match="frame000003.jpg.*progressive"):
        pca_fit.load_dataset_frames(str(tmp_path), backend="hip-baseline")
