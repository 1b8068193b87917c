"""srlhip_pca_gram and fit_pca without a GPU: the host twin against numpy's int64 product, the ABI, the stand-alone host programs (plain and
under the address / undefined-behaviour sanitizers), and fit_pca(backend="host") against numpy.linalg.svd within the tolerances
tests/pca_gram_ref.py derives from the data — up to the saved model loaded back through loadSRLModel."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pca_gram_ref as ref
import pca_ref

sys.path.insert(0, os.path.join(ref.REPO, "robotics-rl-srl_amd"))
from srlhip import _lib  # noqa: E402
from state_representation import pca_fit  # noqa: E402

N_FIT, SHAPE_FIT = 96, (12, 12, 3)


@pytest.fixture(scope="module")
def programs():
    ref.build_programs()
    return ref.PROGRAMS


@pytest.mark.parametrize("F", ref.FS)
def test_host_twin_equals_numpy(F):
    """against the exact reference at every shape of the GPU test, and against X.astype(int64) @ X.T itself where numpy's unaccelerated
    integer product stays quick (which also holds the reference to it)"""
    for N in ref.NS:
        for content in ref.CONTENTS:
            x = ref.frames(content, N, F)
            want, want_rows = ref.gram_ref(x)
            if N * N * F <= 65 * 65 * 12288:
                xi = x.astype(np.int64)
                assert np.array_equal(want, xi @ xi.T) and np.array_equal(want_rows, xi.sum(1))
            gram, rowsum = _lib.pca_gram_host(x)
            assert gram.dtype == np.int64 and np.array_equal(gram, want) and np.array_equal(rowsum, want_rows), (N, F, content)


def test_host_twin_at_the_reference_frame_size():
    N, F = ref.BIG
    for content in ("random", "alternating"):
        x = ref.frames(content, N, F)
        xi = x.astype(np.int64)
        gram, rowsum = _lib.pca_gram_host(x)
        assert np.array_equal(gram, xi @ xi.T) and np.array_equal(rowsum, xi.sum(1))
        assert np.array_equal(gram, ref.gram_ref(x)[0])


def test_exports_header_and_abi():
    lib = _lib.load()
    names = ["srlhip_pca_gram_supported", "srlhip_pca_gram", "srlhip_pca_gram_host", "srlhip_pca_gram_last_error"]
    text = open(os.path.join(ref.REPO, "include", "srlhip.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, text), name
    assert lib.srlhip_abi_version() == _lib.ABI_VERSION == 5
    assert "csrc/pca_gram.hip" in text and "65536" in text and "8192" in text


def test_supported_and_refusals_by_code():
    assert _lib.pca_gram_supported(1, 1) and _lib.pca_gram_supported(8192, 150528) and _lib.pca_gram_supported(33, 150528)
    assert not _lib.pca_gram_supported(0, 1) and not _lib.pca_gram_supported(8193, 1) and not _lib.pca_gram_supported(1, 0)
    for N in (1, 33, 8192):
        most = (2 ** 63 - 1) // (2 * N * N * 65025)                    # the largest F with 2 N^2 F 65025 < 2^63
        assert _lib.pca_gram_supported(N, most) and not _lib.pca_gram_supported(N, most + 1), N
    lib = _lib.load()
    x, gram, rowsum = np.zeros((4, 16), np.uint8), np.full((4, 4), -7, np.int64), np.full(4, -7, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.srlhip_pca_gram_host(p(x), 0, 16, p(gram), p(rowsum)) == -95
    assert lib.srlhip_pca_gram_host(p(x), 8193, 16, p(gram), p(rowsum)) == -95
    assert b"1..8192" in lib.srlhip_pca_gram_last_error()
    assert lib.srlhip_pca_gram_host(None, 4, 16, p(gram), p(rowsum)) == -22
    assert lib.srlhip_pca_gram_host(p(x), 4, 16, None, p(rowsum)) == -22
    # the device call refuses before it touches a GPU
    assert lib.srlhip_pca_gram(0, p(x), 0, 16, 0, p(gram), p(rowsum), None) == -95
    assert lib.srlhip_pca_gram(0, p(x), 8193, 16, 0, p(gram), p(rowsum), None) == -95
    assert lib.srlhip_pca_gram(0, None, 4, 16, 0, p(gram), p(rowsum), None) == -22
    assert lib.srlhip_pca_gram(0, p(x), 4, 16, -1, p(gram), p(rowsum), None) == -22
    assert (gram == -7).all() and (rowsum == -7).all()
    with pytest.raises(_lib.SrlHipError):
        _lib.pca_gram_host(np.zeros((0, 4), np.uint8))


def test_host_programs_prove_the_contract(programs):
    """shift identity, chunk bound, the shape rule, the tiles, the loads' cover at every GPU test shape, the twin: every line ok"""
    for program in programs:                               # the second one is the sanitised build: it must run clean
        out = subprocess.run([os.path.join(ref.CSRC, "build", program), "check"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        lines = out.stdout.decode().splitlines()
        assert out.returncode == 0 and not out.stderr, out.stderr.decode()[-2000:]
        assert lines and all(ln.startswith("ok ") for ln in lines), [ln for ln in lines if not ln.startswith("ok ")]
        covered = {tuple(int(v) for v in ln.split()[-3:]) for ln in lines if ln.startswith("ok cover ")}
        for N in ref.NS:
            for F in ref.FS:
                for split in (0, 1, 7):
                    assert (N, F, split) in covered
        assert all(ref.BIG + (split,) in covered for split in (0, 1, 7)) and (256, 12288, 0) in covered
        for word in ("shift identity", "padding", "extreme sums", "128-bit", "upper triangle", "host twin"):
            assert any(word in ln for ln in lines), word


def test_host_programs_give_the_library_bits(programs, tmp_path):
    for N, F, content in ((1, 1, "all255"), (5, 17, "random"), (33, 1000, "random"), (2, 65536 + 17, "alternating")):
        x = ref.frames(content, N, F)
        want = _lib.pca_gram_host(x)
        for program in programs:
            got = ref.run_program(program, tmp_path, x)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    """k -> (frames, the host fit, the svd reference, the derived bounds), once"""
    out = {}
    for k in (3, 8):
        x = ref.spectrum_frames(k, N_FIT, SHAPE_FIT, k)
        model = pca_fit.fit_pca(x, k, backend="host")
        W = (model.components_ @ (x.reshape(N_FIT, -1).astype(np.float64) - model.mean_).T).T / model.singular_values_ ** 2      # ~ U / sqrt(lam)
        out[k] = (x, model, ref.svd_reference(x), ref.fit_bounds(x, k, W))
    return out


@pytest.mark.parametrize("k", [3, 8])
def test_fit_against_the_svd_within_the_derived_tolerances(fits, k):
    x, model, (mean, sigma, vt), bounds = fits[k]
    # the data, not the code: the signal's singular values are prescribed a factor 2 apart (ref.spectrum_frames); the rounding noise adds
    # to each in quadrature, which leaves the realised ones well separated from each other and from the noise floor behind them
    assert (sigma[:k - 1] >= 1.9 * sigma[1:k]).all() and sigma[k - 1] > 2 * sigma[k]
    assert model.backend == "host" and model.components_.shape == (k, x[0].size) and model.whiten is False and model.n_components_ == k
    err = np.abs(model.explained_variance_ - sigma[:k] ** 2 / (N_FIT - 1))
    print("explained variance: max error %.3e, derived tolerance %.3e" % (err.max(), bounds["variance"]))
    assert (err <= bounds["variance"]).all()
    # sqrt(lam) squared against lam / (N - 1) times (N - 1): four roundings, each of relative size at most 2^-53 (doubled by the square)
    assert np.allclose(model.singular_values_ ** 2, model.explained_variance_ * (N_FIT - 1), rtol=8 * ref.EPS, atol=0)
    assert np.array_equal(model.mean_, x.reshape(N_FIT, -1).sum(axis=0, dtype=np.int64) / np.float64(N_FIT))
    cos = np.abs((model.components_ * vt[:k]).sum(axis=1)) / np.linalg.norm(model.components_, axis=1)
    print("components: max 1 - |cos| %.3e, derived sin bounds %s" % ((1 - cos).max(), bounds["sin_component"]))
    assert (bounds["sin_component"] < 1e-3).all()          # the bound says something
    assert (1.0 - cos <= bounds["sin_component"]).all()
    # the sign convention: the largest-magnitude entry of each left vector u_k = Xc v_k / sigma_k is positive
    u = (x.reshape(N_FIT, -1) - model.mean_) @ model.components_.T
    assert (u[np.argmax(np.abs(u), axis=0), np.arange(k)] > 0).all()


@pytest.mark.parametrize("k", [3, 8])
def test_states_of_the_training_frames(fits, k):
    """per-dimension variance explained_variance_, mutually uncorrelated, zero mean — within the derived bounds"""
    x, model, _, bounds = fits[k]
    Z = model.transform(x)
    assert Z.shape == (N_FIT, k)
    cov = Z.T @ Z / (N_FIT - 1)
    err = np.abs(cov - np.diag(model.explained_variance_))
    print("state covariance: max error %.3e, derived tolerances %.3e .. %.3e" % (err.max(), bounds["cov"].min(), bounds["cov"].max()))
    assert (err <= bounds["cov"]).all()
    assert (np.abs(Z.sum(axis=0)) <= bounds["state_sum"]).all()
    assert (np.abs(np.cov(Z.T) - np.diag(model.explained_variance_)) <= bounds["cov"] + np.outer(bounds["state_sum"], bounds["state_sum"]) / (N_FIT * (N_FIT - 1))).all()


def test_saved_model_loads_as_an_srlpca(fits, tmp_path):
    """FittedPCA.save -> loadSRLModel -> SRLPCA (the torch formulation on the CPU) = (X - mean) @ components^T within the projection's bound"""
    import pickle
    from state_representation.models import SRLPCA, loadSRLModel
    x, model, _, _ = fits[3]
    path = model.save(str(tmp_path))
    assert path.endswith(os.path.join("baselines", "pca_ST_DIM3", "pca.pkl"))
    import json
    cfg = json.load(open(os.path.join(os.path.dirname(path), "exp_config.json")))
    assert cfg["state-dim"] == 3 and "losses" not in cfg
    with open(path, "rb") as f:
        back = pickle.load(f)
    assert type(back).__module__ == "state_representation.pca_fit" and pca_ref.same_bits(back.components_, model.components_)
    srl = loadSRLModel(path, cuda=False, img_shape=SHAPE_FIT[:2])
    assert isinstance(srl, SRLPCA) and srl.state_dim == 3 and srl.hip is None
    got = srl.getStates(x).numpy()
    w, b = pca_ref.fold(model)
    X = x.reshape(N_FIT, -1).astype(np.float64)
    want = (X - model.mean_) @ model.components_.T
    # two summations of the same F products and the folded bias: each within pca_ref.bound of the exact value
    bound = 2 * pca_ref.bound(w.shape[0], X @ np.abs(w) + np.abs(b)[None, :] + np.abs(model.mean_) @ np.abs(w))
    assert (np.abs(got - want) <= bound).all()
    assert (np.abs(model.transform(x) - want) == 0).all()


def test_fit_refuses_what_it_cannot_take():
    x = ref.spectrum_frames(1, 8, (4, 4, 3), 2)
    with pytest.raises(ValueError):
        pca_fit.fit_pca(x, 8, backend="host")                      # state_dim > N - 1
    with pytest.raises(ValueError):
        pca_fit.fit_pca(x.astype(np.float32), 2, backend="host")
    with pytest.raises(ValueError):
        pca_fit.fit_pca(x, 2, backend="rocblas")
    with pytest.raises(ValueError):
        pca_fit.fit_pca(np.zeros((8, 4, 4, 3), np.uint8), 2, backend="host")       # no variance at all


def test_command_line_on_a_recorded_dataset(tmp_path):
    """record_*/frame*.jpg as dataset_generator writes them -> pca.pkl that loadSRLModel takes; the subsampling is even"""
    from PIL import Image
    from state_representation.models import loadSRLModel
    x = ref.spectrum_frames(5, 24, (16, 16, 3), 3)
    for i, frame in enumerate(x):
        folder = tmp_path / "data" / ("record_%03d" % (i // 8))
        folder.mkdir(parents=True, exist_ok=True)
        Image.fromarray(frame).save(str(folder / ("frame%06d.jpg" % (i % 8))), quality=95)
    frames = pca_fit.load_dataset_frames(str(tmp_path / "data"), max_frames=12)
    assert frames.shape == (12, 16, 16, 3) and frames.dtype == np.uint8
    path = pca_fit.main(["--data-folder", str(tmp_path / "data"), "--state-dim", "3", "--max-frames", "24", "--backend", "host",
                         "--log-folder", str(tmp_path / "logs")])
    srl = loadSRLModel(path, cuda=False, img_shape=(16, 16))
    assert srl.state_dim == 3 and tuple(srl._w.shape) == (16 * 16 * 3, 3)


def test_against_sklearn_if_it_is_installed(fits):
    """explained variances and |cos| of the components.  The SIGN is not compared: fit_pca fixes it on the left vector u_k, a current
    sklearn on the component's own largest entry, and the two differ on this data (the signed cosines are printed)"""
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        pytest.skip("SKLEARN IS NOT INSTALLED: the svd_flip sign convention and the attributes are compared with numpy.linalg.svd only")
    x, model, _, bounds = fits[3]
    sk = PCA(n_components=3, svd_solver="full").fit(x.reshape(N_FIT, -1).astype(np.float64))
    assert (np.abs(sk.explained_variance_ - model.explained_variance_) <= bounds["variance"]).all()
    cos = (sk.components_ * model.components_).sum(axis=1) / np.linalg.norm(model.components_, axis=1)
    print("signed cos against sklearn", cos)
    assert (1.0 - np.abs(cos) <= bounds["sin_component"]).all()
