"""numpy reference of the sampled LINEAR policy (srlhip_rollout_policy_sampled, srlhip_sample_actions; contracts in include/srlhip.h).
No GPU, no torch.  Nothing here is a new definition:

  scores      policy_act_ref.inputs / linear_scores: x_d, then score_a = sum_d (double)x_d W[d][a], d ascending, from the d = 0 product;
  the draw    mlp_sample_ref.draws: u = to_double(o[0], o[1]) of the Philox4x32-10 block (rng_stream_ref) at counter c0 + t, stream 1, key =
              the env's seed;
  selection   mlp_sample_ref.cdf / contract: m, w_k, c_k, z, a;
  acceptance  mlp_sample_ref's rule: a recorded live action a is accepted iff (a == 0 or z (1 + rho) >= c_{a-1} (1 - rho)) and
              (a == A-1 or z (1 - rho) < c_a (1 + rho)); a frozen entry is exactly -1.

THE TOLERANCE THAT ENTERS rho.  The header bounds a score of the MLP against any other float64 summation of the same terms by
(2 D + H + 16) 2^-53 S_a: D + 1 roundings along a hidden unit's chain and at most 13 behind it on the contract's side, at most D + H + 2
on the other.  A linear policy has no hidden layer: S_a shrinks to sum_d |x_d W[d][a]| and the H terms drop out, which leaves
    tol_a = (2 D + 16) 2^-53 sum_d |x_d W[d][a]|
— generous for a chain of D products and D - 1 additions per side (the Kuka kernels may fuse a product with the sum that takes it: one
rounding fewer, inside the same bound), and kept as the header states it.  Then score_k - m is known to E = 2 max_k tol_k, w_k =
exp(score_k - m) to a relative expm1(E), and on top of that the rounding of both sides — one exp each (<= 1 ulp, the device library's
documented figure), at most A - 1 <= 5 additions and one product: below 2^-49.  rho = expm1(E) + 2^-48.
For srlhip_sample_actions the scores are GIVEN, bit for bit the same on both sides: E = 0, and only the 2^-48 remains.

`pinned` says whether a decision lies outside the band: z (1 +- rho) on the same side of every c_k (1 -+ rho).  The CPU test shows that
on the score and weight ranges the GPU tests use every decision of the reference is pinned."""
import numpy as np

import mlp_sample_ref as msr
import policy_act_ref as par

ROUNDING = msr.ROUNDING            # 2^-48
draws = msr.draws
cdf = msr.cdf
contract = msr.contract


def tol_factor(D):
    return (2 * D + 16) * 2.0 ** -53


def scores(obs, W, per_env=True, mean=None, std=None, clip=10.0):
    """obs [N][D] float32 -> (score [N][A], S [N][A] = sum_d |x_d W[d][a]|)"""
    x = par.inputs(obs, mean, std, clip)
    W = np.asarray(W, np.float64)
    Wn = W if per_env else np.broadcast_to(W, (x.shape[0],) + W.shape)
    S = np.abs(x.astype(np.float64)[:, :, None] * Wn).sum(1)
    return par.linear_scores(x, W, per_env), S


def rho_of(S, D):
    """S [..., A] -> rho [...]; S = None: given scores (E = 0)"""
    if S is None:
        return ROUNDING
    return np.expm1(2.0 * (tol_factor(D) * S).max(-1)) + ROUNDING


def sample_check(score, S, D, u, actions, frozen=None):
    """-> (ok, differs, banded), each [...] bool.  ok: the acceptance rule (a frozen entry: exactly -1); differs: live entries the
    reference itself decides differently at rho = 0; banded: live entries whose decision is NOT pinned (they pass only through the band)."""
    A = score.shape[-1]
    actions = np.asarray(actions)
    frozen = np.zeros(actions.shape, bool) if frozen is None else np.asarray(frozen, bool)
    rho = rho_of(S, D)
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
    return ok, differs, ~frozen & ~pinned(score, S, D, u)


def pinned(score, S, D, u):
    """[...] bool: no c_k (k < A - 1) lies within the band around z — every implementation of the contract takes the same action"""
    rho = np.asarray(rho_of(S, D))[..., None]
    c, _ = cdf(score)
    z = (u * c[..., -1])[..., None]
    ck = c[..., :-1]
    above = z * (1 - rho) >= ck * (1 + rho)            # z has passed c_k whatever the rounding
    under = z * (1 + rho) < ck * (1 - rho)             # z has not, whatever the rounding
    return (above | under).all(-1)
