"""numpy restatement of srlhip_policy_act's arithmetic contract (include/srlhip.h; the library's text is csrc/policy_act.hpp), ORDER-exact:
every product and every sum is one float64 numpy operation, taken in the contract's order, so the result is the kernel's bit for bit.
No GPU, no torch.

    x        the float32 policy input (mlp_policy_ref.normalise: float64 normalisation, clamp, back to float32)
    linear   score_a = x_0 W[0][a] + x_1 W[1][a] + ... (d ascending, starting with the d = 0 product)
    MLP      pre_j = b1_j + W1[j][0] x_0 + ... (d ascending), h_j = pre_j if pre_j > 0 else +0.0; 16 virtual lanes, lane l sums its
             units l, l + 16, ... from b2_a (lane 0) or +0.0; then four stages in which every lane adds its partner's value:
             l ^ 1, l ^ 2, 7 - l inside each half, 15 - l
    select   strict argmax, the float32 row, or the inverse-CDF pick given u and the softmax weights
"""
import numpy as np

import mlp_policy_ref as ref

LANES = 16
PARTNERS = [np.arange(LANES) ^ 1, np.arange(LANES) ^ 2, (np.arange(LANES) & 8) | (7 - (np.arange(LANES) & 7)), 15 - np.arange(LANES)]
ROUNDING = 2.0 ** -48          # mlp_sample_ref's: one exp per side, five additions, one product


def tol_factor(D, H):
    """|score - any other float64 summation of the same terms| <= tol_factor S (the header's bound): D + 1 roundings along a unit's
    chain and at most 13 behind it on the contract's side, at most D + H + 2 on the other."""
    return (2 * D + H + 16) * 2.0 ** -53


def inputs(obs, mean=None, std=None, clip=10.0):
    return ref.normalise(np.asarray(obs, np.float32), mean, std, clip)


def linear_scores(x, W, per_env=True):
    """x [N][D] float32, W [N][D][A] or [D][A] float64 -> score [N][A]"""
    x = np.asarray(x, np.float32).astype(np.float64)
    W = np.asarray(W, np.float64)
    W = W if per_env else np.broadcast_to(W, (x.shape[0],) + W.shape)
    score = x[:, 0, None] * W[:, 0, :]
    for d in range(1, x.shape[1]):
        score = score + x[:, d, None] * W[:, d, :]
    return score


def row_sum16(p):
    """p [..., 16] -> lane 0's value after the four stages"""
    for partner in PARTNERS:
        p = p + p[..., partner]
    return p[..., 0]


def mlp_scores(x, params, hidden, A, per_env=True):
    """x [N][D] float32, params [N][P] or [P] float32 -> score [N][A] float64"""
    x = np.asarray(x, np.float32).astype(np.float64)
    N, D = x.shape
    H = hidden
    p = np.asarray(params, np.float32).astype(np.float64)
    p = p if per_env else np.broadcast_to(p, (N,) + p.shape)
    w1, b1, w2, b2 = ref.split(p, D, H, A)
    pre = b1.copy()
    for d in range(D):
        pre = pre + w1[:, :, d] * x[:, d, None]
    h = np.where(pre > 0.0, pre, 0.0)
    part = np.zeros((N, A, LANES))
    part[:, :, 0] = b2
    for j in range(H):                                  # ascending j: every lane meets its units in ascending order
        part[:, :, j % LANES] = part[:, :, j % LANES] + w2[:, :, j] * h[:, j, None]
    return row_sum16(part)


def plain_mlp_scores(x, params, hidden, A, per_env=True):
    """the plain numpy sums of the same terms (np.sum's own order)"""
    x = np.asarray(x, np.float32)
    score, _ = ref.forward(params if per_env else np.broadcast_to(params, (x.shape[0],) + np.shape(params)), x, x.shape[1], hidden, A)
    return score


def argmax(score):
    return score.argmax(-1).astype(np.int32)            # the first maximum: the strict comparison's


def softmax_weights(score):
    return np.exp(score - score.max(-1, keepdims=True))


def pick(w, u):
    """the inverse CDF given the weights: c_k in index order, z = u c_{A-1}, the number of k < A-1 with z >= c_k"""
    c = np.empty_like(w)
    c[..., 0] = w[..., 0]
    for k in range(1, w.shape[-1]):
        c[..., k] = c[..., k - 1] + w[..., k]
    z = u * c[..., -1]
    return (z[..., None] >= c[..., :-1]).sum(-1).astype(np.int32)


def interval_ok(score, u, actions, rho=ROUNDING):
    """mlp_sample_ref's acceptance rule for live entries, with the scores known exactly (they are compared bit for bit first): what
    is left is the two exp implementations and the additions, rho = 2^-48."""
    w = softmax_weights(score)
    c = w.copy()
    for k in range(1, w.shape[-1]):
        c[..., k] = c[..., k - 1] + w[..., k]
    A = w.shape[-1]
    z = u * c[..., -1]
    a = np.clip(actions, 0, A - 1)
    below = np.take_along_axis(c, np.maximum(a - 1, 0)[..., None], -1)[..., 0]
    own = np.take_along_axis(c, a[..., None], -1)[..., 0]
    lower = (a == 0) | (z * (1 + rho) >= below * (1 - rho))
    upper = (a == A - 1) | (z * (1 - rho) < own * (1 + rho))
    return (actions >= 0) & (actions < A) & lower & upper


def frozen_after(frozen, done_prev, freeze):
    """the frozen plane after a call (freeze_after_done off: untouched, nobody is frozen) -> (plane, who takes `None`)"""
    frozen = np.asarray(frozen, np.uint8)
    if not freeze:
        return frozen.copy(), np.zeros(frozen.shape, bool)
    f = (frozen != 0).astype(np.uint8)
    if done_prev is not None:
        f = f | (np.asarray(done_prev, np.uint8) & 1)
    return f, f != 0


def none_rows(actions, who, discrete, none_nan):
    """the `None` action of the frozen envs: -1, a row of NaNs (Kuka continuous) or a zero row (MobileRobot continuous)"""
    out = actions.copy()
    if discrete:
        out[who] = -1
    else:
        out[who] = np.float32(np.nan) if none_nan else np.float32(0.0)
    return out


def act(obs, D, A, discrete, weights=None, params=None, hidden=None, per_env=True, mean=None, std=None, clip=10.0, freeze=False,
        done_prev=None, frozen=None, none_nan=False, u=None):
    """one srlhip_policy_act call -> dict(score, action, frozen, w).  u (float64 [N]): the sampled form, given the draws."""
    x = inputs(np.asarray(obs, np.float32).reshape(-1, D), mean, std, clip)
    score = linear_scores(x, weights, per_env) if params is None else mlp_scores(x, params, hidden, A, per_env)
    w = None
    if u is not None:
        w = softmax_weights(score)
        action = pick(w, np.asarray(u, np.float64))
    else:
        action = argmax(score) if discrete else score.astype(np.float32)
    fz = np.zeros(len(x), np.uint8) if frozen is None else frozen
    plane, who = frozen_after(fz, done_prev, freeze)
    return dict(score=score, action=none_rows(action, who, discrete, none_nan), frozen=plane, w=w, live=~who)
