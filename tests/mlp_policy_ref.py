"""float64 numpy reference of the fused MLP policy (srlhip_rollout_mlp_policy): parameter layout, scores and the rounding scale the
GPU tests' tolerance is built from.  No GPU, no torch."""
import numpy as np


def param_count(D, H, A):
    return H * D + H + A * H + A


def split(params, D, H, A):
    """[..., P] in nn.Module.parameters() order -> fc_in.weight [..., H, D], fc_in.bias [..., H], fc_out.weight [..., A, H],
    fc_out.bias [..., A]"""
    assert params.shape[-1] == param_count(D, H, A), (params.shape, D, H, A)
    lead, o = params.shape[:-1], 0
    w1 = params[..., o:o + H * D].reshape(lead + (H, D)); o += H * D
    b1 = params[..., o:o + H]; o += H
    w2 = params[..., o:o + A * H].reshape(lead + (A, H)); o += A * H
    b2 = params[..., o:o + A]
    return w1, b1, w2, b2


def normalise(obs, mean=None, std=None, clip=10.0):
    """the float32 x the kernel feeds the MLP"""
    if mean is None:
        return obs.astype(np.float32)
    return np.clip((obs.astype(np.float64) - mean) / std, -clip, clip).astype(np.float32)


def forward(params, x, D, H, A):
    """params [N][P] or [P] (float32 values), x [..., N, D] -> (score [..., N, A], S [..., N, A]) in float64.
    S_a = |b2_a| + sum_j |W2[a][j]| (|b1_j| + sum_d |W1[j][d] x_d|): the scale of the float64 rounding error of score_a."""
    p = np.asarray(params).astype(np.float32).astype(np.float64)
    w1, b1, w2, b2 = split(p, D, H, A)
    x = np.asarray(x, dtype=np.float64)
    terms = w1 * x[..., None, :]                                   # [..., N, H, D]
    pre = b1 + terms.sum(-1)
    h = np.maximum(pre, 0.0)
    score = b2 + (w2 * h[..., None, :]).sum(-1)
    habs = np.abs(b1) + np.abs(terms).sum(-1)
    S = np.abs(b2) + (np.abs(w2) * habs[..., None, :]).sum(-1)
    return score, S


TOL_FACTOR = 2.0 ** -44      # gamma_(H + D + 2) <= 132 * 2^-53 at H = 128, times 4: two layers and the comparison of two scores


def random_params(seed, shape):
    """~ N(0, 0.5) rounded to float32"""
    return (0.5 * np.random.RandomState(seed).standard_normal(shape)).astype(np.float32)
