"""srlhip_pca_gram's and fit_pca's references, and the DERIVED tolerances of the fit's tests (nothing here is tuned to what the code gives).

GRAM.  gram = X X^T and rowsum = X 1 of uint8 frames are exact integers.  gram_ref() forms them through float64 BLAS: every product is at
most 255^2 and every partial sum at most F 65025 < 2^53 (asserted), so every float64 operation is exact whatever order BLAS sums in — the
same integers as X.astype(int64) @ X.T (tests/test_pca_gram_cpu.py holds the two against each other), at a speed that lets the GPU test
take 200 frames of 65553 features.

FIT.  The fit (state_representation/pca_fit.py) is compared with numpy.linalg.svd of the centred float64 matrix Xc = X - mean.  Write eps =
2^-53, C = Xc Xc^T, lam_k = sigma_k^2 its eigenvalues, p(n) = n for the backward-error constant of LAPACK's symmetric eigensolver and SVD
(computed results are exact for a matrix within p(n) eps ||A||_2 of A; LAPACK's documented form, with the modest polynomial taken as n).
  * The fit's C is float64(M) / float64(N^2) with M the EXACT integer N^2 C: two roundings per element, |dC_ij| <= 2 eps |C_ij|, so
    ||dC||_2 <= ||dC||_F <= 2 eps ||C||_F.  eigh adds N eps ||C||_2.  E_fit = 2 eps ||C||_F + N eps ||C||_2.
  * The reference: Xc carries one rounding of the mean and one of the subtraction, |dXc_if| <= 2 eps 255, and the SVD max(N, F) eps sigma_1:
    dsigma = max(N, F) eps sigma_1 + 2 eps 255 sqrt(N F), which moves lam_k by at most E_ref = 2 sigma_1 dsigma + dsigma^2.
  * Weyl: |lam_k(fit) - lam_k(ref)| <= E = E_fit + E_ref; explained variances differ by at most E / (N - 1).
  * Davis-Kahan (sin theta <= 2 ||E|| / gap): the fit's u_k is within s_u = 2 E / gap_k of the reference's left vector, gap_k the
    distance from the reference's lam_k to its nearest other eigenvalue.  The component is v_k = Xc^T u_k / sigma_k: an error of u_k along
    u_j is scaled by sigma_j / sigma_k <= sigma_1 / sigma_k.  The projection kernel that forms it sums N terms per element within
    pca_ref.bound(N, T) (its own derived bound, T = sum_i x_if |W_ik|), and the mean correction adds 3 roundings of terms no larger than T':
    dv_fk <= bound(N, T_fk) + 3 * 2 eps T'_fk, T'_fk = mean_f sum_i |W_ik|.  So
        sin(v_k(fit), v_k(ref)) <= s_v = (sigma_1 / sigma_k) s_u + ||dv_k||_2 / ||v_k||_2,    |cos| >= 1 - s_v   (cos >= 1 - sin on [0, 1]).
  * The training frames' states Z = Xc V^T: Z_k = (C u_k + Xc dv_k sigma_k) / sigma_k = sqrt(lam_k) u_k + r_k / sqrt(lam_k) + Xc dv_k with
    r_k = C u_k - lam_k u_k the eigenpair's residual, ||r_k|| <= E_fit.  With e_k = E_fit / sqrt(lam_k) + sigma_1 ||dv_k||_2 and
    |u_k . u_l - delta_kl| <= N eps (eigh's orthogonality):
        |Z_k . Z_l - lam_k delta_kl| <= sqrt(lam_k lam_l) N eps + sqrt(lam_k) e_l + sqrt(lam_l) e_k + e_k e_l,
    divided by N - 1 for the (co)variances; the states' means vanish because C 1 = 0 (u_k is orthogonal to 1 up to the same residual):
        |sum_i Z_ik| <= sqrt(N) (E_fit / sqrt(lam_k) + e_k)."""
import os
import subprocess

import numpy as np

import pca_ref

REPO = pca_ref.REPO
CSRC = pca_ref.CSRC
PROGRAMS = ("pca_gram_hostcheck", "pca_gram_hostcheck_san")
EPS = 2.0 ** -53

# the shapes at which the kernel can go wrong: the tile edges in N; in F a lone byte, one below / at / above a 16-byte piece (unaligned row
# strides), one frame of 64 x 64 x 3, one int32 chunk and 17 features, and the reference's 224 x 224 x 3 (three chunks) at N = 33 only
NS = (1, 2, 31, 32, 33, 65, 200)
FS = (1, 15, 16, 17, 12288, 65536 + 17)
BIG = (33, 150528)
CONTENTS = ("random", "zeros", "all255", "alternating")


def frames(content, N, F, seed=0):
    """alternating: rows of 0 and 255 — signed -128 against 127 and -128 against -128, the extremes of a chunk's int32"""
    if content == "random":
        return np.random.RandomState(seed + 7 * N + F % 1009).randint(0, 256, size=(N, F)).astype(np.uint8)
    x = np.zeros((N, F), np.uint8)
    if content == "all255":
        x[:] = 255
    elif content == "alternating":
        x[1::2] = 255
    return x


def gram_ref(x):
    """-> (gram int64 [N][N], rowsum int64 [N]), exact (see the module's text)"""
    x = np.ascontiguousarray(x).reshape(len(x), -1)
    assert x.dtype == np.uint8 and x.shape[1] * 65025 < 2 ** 53
    xf = x.astype(np.float64)
    g = xf @ xf.T
    assert np.array_equal(g, np.rint(g))
    return g.astype(np.int64), x.sum(axis=1, dtype=np.int64)


def build_programs():
    subprocess.check_call(["make", "-s", "-C", CSRC, "pcagramhostcheck"], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))


def run_program(program, tmpdir, x):
    path, res = os.path.join(str(tmpdir), "gram_case.bin"), os.path.join(str(tmpdir), "gram_result.bin")
    N, F = x.shape
    with open(path, "wb") as f:
        f.write(np.array([N, F], np.int64).tobytes())
        f.write(np.ascontiguousarray(x).tobytes())
    subprocess.check_call([os.path.join(CSRC, "build", program), path, res])
    out = np.fromfile(res, np.int64)
    return out[:N * N].reshape(N, N), out[N * N:]


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
def spectrum_frames(seed, N, shape, k):
    """uint8 [N][H][W][C]: 128 + a rank-k signal whose singular values are a factor 2 apart, scaled so that its largest entry is 120 (no
    clipping), rounded to bytes: the rounding is the noise"""
    rng = np.random.RandomState(seed)
    F = int(np.prod(shape))
    u, _ = np.linalg.qr(rng.standard_normal((N, k + 1)) - rng.standard_normal((1, k + 1)))
    u = u - u.mean(axis=0)                                  # centred columns: the signal does not move the mean
    u, _ = np.linalg.qr(u)
    v, _ = np.linalg.qr(rng.standard_normal((F, k)))
    L = (u[:, :k] * (2.0 ** -np.arange(k))[None, :]) @ v.T
    L *= 120.0 / np.abs(L).max()
    x = np.rint(128.0 + L)
    assert x.min() >= 0 and x.max() <= 255
    return x.astype(np.uint8).reshape((N,) + tuple(shape))


def svd_reference(x):
    """numpy.linalg.svd of the centred float64 matrix -> (mean [F], sigma [min(N, F)], Vt)"""
    X = x.reshape(len(x), -1).astype(np.float64)
    mean = X.mean(axis=0)
    _, sigma, vt = np.linalg.svd(X - mean, full_matrices=False)
    return mean, sigma, vt


def fit_bounds(x, k, W):
    """The tolerances of the module's text for the first k pairs.  W [N][k]: the fit's u_k / sqrt(lam_k).  -> dict"""
    X = x.reshape(len(x), -1).astype(np.float64)
    N, F = X.shape
    mean, sigma, _ = svd_reference(x)
    Xc = X - mean
    C = Xc @ Xc.T
    lam = sigma ** 2
    e_fit = 2 * EPS * np.linalg.norm(C, "fro") + N * EPS * lam[0]
    dsigma = max(N, F) * EPS * sigma[0] + 2 * EPS * 255.0 * np.sqrt(N * F)
    e_ref = 2 * sigma[0] * dsigma + dsigma ** 2
    E = e_fit + e_ref
    gap = np.array([min(abs(lam[j] - lam[i]) for i in range(len(lam)) if i != j) for j in range(k)])
    s_u = 2 * E / gap
    T = X.T @ np.abs(W)                                     # [F][k]
    Tm = mean[:, None] * np.abs(W).sum(axis=0)[None, :]
    dv = np.linalg.norm(pca_ref.bound(N, T) + 6 * EPS * Tm, axis=0)      # ||dv_k||_2 (v_k has unit norm)
    s_v = sigma[0] / sigma[:k] * s_u + dv / (1.0 - dv)
    e = e_fit / sigma[:k] + sigma[0] * dv
    sq = sigma[:k]
    gram_tol = np.outer(sq, sq) * N * EPS + np.outer(sq, e) + np.outer(e, sq) + np.outer(e, e)
    return {"variance": E / (N - 1), "sin_component": s_v, "cov": gram_tol / (N - 1), "state_sum": np.sqrt(N) * (e_fit / sq + e),
            "sigma": sigma, "gap": gap}
