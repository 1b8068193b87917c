"""numpy reference of the sampled MLP-policy rollout (srlhip_rollout_mlp_policy_sampled, contract in include/srlhip.h): the uniform
draws of every env's action stream, the contract itself in plain numpy, and the acceptance rule the GPU tests hold a recorded
action to.  No GPU, no torch.

The draw: u = to_double(o[0], o[1]) of the Philox4x32-10 block at counter c0 + t, stream 1, key = the env's seed (lo, hi) — the
definition is tests/rng_stream_ref.py's (philox4x32_10 / project_block / to_double), run here on whole numpy planes.

The acceptance rule (the issue's): with score and S from mlp_policy_ref.forward, tol_k = TOL_FACTOR S_k bounds the error of a score,
so score_k - m is known to E = 2 max_k tol_k and w_k = exp(score_k - m) to a relative expm1(E), plus rounding — one exp per side
(<= 1 ulp each, the device library's documented figure), at most five additions and one product: below 2^-49.  rho = expm1(E) + 2^-48.
A recorded live action a is accepted iff  (a == 0 or z (1 + rho) >= c_{a-1} (1 - rho))  and  (a == A-1 or z (1 - rho) < c_a (1 + rho)),
w, c, z being numpy's.  Frozen entries are exactly -1."""
import numpy as np

import mlp_policy_ref as ref
import rng_stream_ref as rsr

ROUNDING = 2.0 ** -48


def draws(seeds, c0, T):
    """u [T][n]: env e (seed seeds[e]) at counters c0[e] + t (c0: scalar or [n]), stream 1, words 0 and 1"""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1)
    n = len(seeds)
    ctr = (np.broadcast_to(np.asarray(c0, dtype=np.uint64), (n,))[None, :] + np.arange(T, dtype=np.uint64)[:, None]).astype(object)
    k0 = np.broadcast_to((seeds & np.uint64(rsr.M32)).astype(object), (T, n))
    k1 = np.broadcast_to((seeds >> np.uint64(32)).astype(object), (T, n))
    # rng_stream_ref.project_block on object arrays of Python ints: the plain-integer definition, element by element
    o = rsr.project_block(k0, k1, ctr, 1)
    return np.asarray(rsr.to_double(o[0], o[1]), dtype=np.float64)


def cdf(score):
    """score [..., A] -> (c [..., A] partial sums of exp(score - max) in index order, w)"""
    w = np.exp(score - score.max(-1, keepdims=True))
    c = np.empty_like(w)
    c[..., 0] = w[..., 0]
    for k in range(1, w.shape[-1]):
        c[..., k] = c[..., k - 1] + w[..., k]
    return c, w


def contract(score, u):
    """the contract in plain numpy: score [..., A], u [...] -> action [...] (int32)"""
    c, _ = cdf(score)
    z = u * c[..., -1]
    return (z[..., None] >= c[..., :-1]).sum(-1).astype(np.int32)


def sample_check(score, S, u, actions, frozen=None):
    """-> (ok [...] bool, differs [...] bool): ok — the acceptance rule above for every entry (a frozen entry: exactly -1); differs —
    live entries the reference itself decides differently at rho = 0."""
    A = score.shape[-1]
    actions = np.asarray(actions)
    frozen = np.zeros(actions.shape, bool) if frozen is None else frozen
    tol = ref.TOL_FACTOR * S
    rho = np.expm1(2.0 * tol.max(-1)) + ROUNDING
    c, _ = cdf(score)
    z = u * c[..., -1]
    in_range = (actions >= 0) & (actions < A)
    a = np.where(in_range, actions, 0)
    below = np.take_along_axis(c, np.maximum(a - 1, 0)[..., None], -1)[..., 0]        # c_{a-1}
    own = np.take_along_axis(c, a[..., None], -1)[..., 0]                               # c_a
    lower_ok = (a == 0) | (z * (1 + rho) >= below * (1 - rho))
    upper_ok = (a == A - 1) | (z * (1 - rho) < own * (1 + rho))
    ok = np.where(frozen, actions == -1, in_range & lower_ok & upper_ok)
    differs = ~frozen & (contract(score, u) != actions)
    return ok, differs
