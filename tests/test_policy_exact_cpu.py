"""CPU checks of tests/policy_exact.py, the design behind tests/test_gpu_policy_exact.py: the order-independence predicate is
right where it says yes (every summation order the kernels could use gives the same bits there), is not vacuous (on Gaussian
parameters it says no and the orders do differ), and the cases of the GPU tests — run closed-loop against the CPU oracle alone —
are exact on all but at most 1 % of their triples, produce the ties, clamp hits and dead units they are there for, and raise no IK
conditioning flag."""
from fractions import Fraction

import numpy as np
import pytest

import mlp_policy_ref as ref
import policy_exact as pe


def seq_sum(t, order):
    """left to right along the last axis, in `order`"""
    acc = t[..., order[0]]
    for i in order[1:]:
        acc = acc + t[..., i]
    return acc


def lane_sum(t2, H, reduce):
    """t2 [..., 1 + H]: b2 and the H products.  Lane l of 16 starts from b2 (lane 0) or +0.0 and adds its units l, l + 16, ... (eight
    slots; the ones >= H are +0.0), then the lanes are reduced: "butterfly" (quad_perm [1,0,3,2], quad_perm [2,3,0,1],
    row_half_mirror, row_mirror) or "inorder" (lane 0, then 1, ... 15)."""
    lanes = []
    for l in range(16):
        acc = t2[..., 0] if l == 0 else np.zeros(t2.shape[:-1])
        for u in range(8):
            j = l + 16 * u
            acc = acc + (t2[..., 1 + j] if j < H else 0.0)
        lanes.append(acc)
    v = np.stack(lanes, -1)
    if reduce == "inorder":
        return seq_sum(v, list(range(16)))
    i = np.arange(16)
    for perm in (i ^ 1, i ^ 2, (i & 8) | (7 - (i & 7)), 15 - i):
        v = v + v[..., perm]
    assert all(np.array_equal(v[..., 0], v[..., k]) for k in range(16))
    return v[..., 0]


def all_orders(params, x, D, H, A, seed):
    """-> list of (name, score [M][A]) of the forward pass of one block on x [M][D] in different summation orders, and the score terms"""
    rng = np.random.RandomState(seed)
    w1, b1, w2, b2 = ref.split(np.asarray(params, np.float32).astype(np.float64), D, H, A)
    t1 = np.concatenate([np.broadcast_to(b1, (len(x), H))[..., None], w1 * x.astype(np.float64)[:, None, :]], -1)       # [M][H][1 + D]
    out = []
    h_nat = None
    for name, o1 in [("natural", list(range(D + 1)))] + [("perm%d" % k, list(rng.permutation(D + 1))) for k in range(3)]:
        h = np.maximum(seq_sum(t1, o1), 0.0)
        h_nat = h if h_nat is None else h_nat
        t2 = np.concatenate([np.broadcast_to(b2, (len(x), A))[..., None], w2 * h[:, None, :]], -1)                        # [M][A][1 + H]
        out.append((name + "/pairwise", t2.sum(-1)))
        out.append((name + "/perm", seq_sum(t2, list(rng.permutation(H + 1)))))
        out.append((name + "/butterfly", lane_sum(t2, H, "butterfly")))
        out.append((name + "/inorder", lane_sum(t2, H, "inorder")))
    t2 = np.concatenate([np.broadcast_to(b2, (len(x), A))[..., None], w2 * h_nat[:, None, :]], -1)
    return out, t1, t2


def inputs(D, M, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-3.0, 3.0, size=(M, D)).astype(np.float32)
    x[rng.random_sample((M, D)) < 0.1] = 0.0
    x[::17, 0] = np.float32(2.0 ** -40 * (1 + 2.0 ** -20))         # a nonzero |x| far below 2^-15: the predicate has to say no somewhere
    return x


@pytest.mark.parametrize("D,H,A", [(1, 1, 2), (2, 15, 4), (2, 17, 2), (3, 33, 7), (3, 128, 6)])
def test_where_the_predicate_holds_every_order_gives_the_same_bits(D, H, A):
    M = 400
    params = pe.dyadic_params(7 + H, D, A, hidden=H, dead=0.2)
    x = inputs(D, M, H)
    orders, t1, t2 = all_orders(params, x, D, H, A, H)
    score, exact, _ = pe.expected(x[:, None, :], params[None], False, hidden=H)
    score, exact = score[:, 0], exact[:, 0]
    assert 0.5 < exact.mean() and (H == 1 or not exact.all())          # both sides occur (H = 1: too few terms to lose a bit)
    for name, s in orders:
        assert np.array_equal(pe.bits(s + 0.0)[exact], pe.bits(score)[exact]), name
    # the real sum, on a sample (the hidden units' sums first: they feed the score's terms)
    pick = np.flatnonzero(exact.all(-1))[:40]
    for m in pick:
        for j in range(H):
            assert float(sum(Fraction(float(v)) for v in t1[m, j])) == t1[m, j].sum()
        for a in range(A):
            assert float(sum(Fraction(float(v)) for v in t2[m, a])) == score[m, a]


def test_linear_policy_where_the_predicate_holds_every_order_gives_the_same_bits():
    D, A, M = 3, 6, 400
    W = pe.dyadic_params(3, D, A)
    x = inputs(D, M, 5)
    score, exact, _ = pe.expected(x[:, None, :], W, False, per_env=False)
    terms = x.astype(np.float64)[:, :, None] * W
    assert 0.5 < exact.mean() < 1.0
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1]):
        s = seq_sum(np.moveaxis(terms, 1, -1), order)
        assert np.array_equal((s == score[:, 0])[exact[:, 0]], np.ones(int(exact.sum()), bool)), order
    for m in np.flatnonzero(exact[:, 0].all(-1))[:40]:
        for a in range(A):
            assert float(sum(Fraction(float(v)) for v in terms[m, :, a])) == score[m, 0, a]


def test_on_gaussian_parameters_the_predicate_says_no_and_the_orders_differ():
    D, H, A, M = 3, 100, 6, 400
    params = ref.random_params(11, (ref.param_count(D, H, A),))
    x = inputs(D, M, 1)
    orders, t1, t2 = all_orders(params, x, D, H, A, 1)
    assert pe.order_free(t2).mean() < 0.01
    assert not pe.expected(x[:, None, :], params[None], False, hidden=H)[1].any()
    base = orders[0][1]
    differing = [name for name, s in orders[1:] if not np.array_equal(s, base)]
    assert any("butterfly" in n for n in differing) and any("inorder" in n for n in differing) and any("/perm" in n for n in differing)


def test_order_free_on_hand_made_sums():
    assert pe.order_free(np.array([1.0, 2.0 ** -50, -1.0]))            # B < 4, E = 2: quantum 2^-50
    assert not pe.order_free(np.array([1.0, 2.0 ** -53, -1.0]))       # (1 + 2^-53) - 1 is 0 in float64
    assert not pe.order_free(np.array([2.0, 2.0, 2.0 ** -50]))        # B > 4: quantum 2^-49
    assert pe.order_free(np.zeros(5)) and pe.order_free(np.array([-0.0, 0.0]))
    assert pe.order_free(np.array([[1.0, 3.0], [1.0, 2.0 ** -60]]), axis=1).tolist() == [True, False]
    assert pe.one_bit(pe.WEIGHTS) and not pe.one_bit(np.array([0.75]))


def test_dyadic_parameters_have_the_values_and_the_structure_they_promise():
    D, H, A, n = 3, 17, 6, 12
    p = pe.dyadic_params(5, D, A, n, hidden=H, tie_groups=pe.tie_patterns(A), dead=0.25, all_dead_every=3, zero_every=11, neg_zero_b2_every=5)
    assert p.dtype == np.float32 and p.shape == (n, ref.param_count(D, H, A))
    w1, b1, w2, b2 = ref.split(p, D, H, A)
    assert np.isin(w1, pe.WEIGHTS).all() and np.isin(w2, pe.WEIGHTS).all()
    for b in (b1, b2):
        assert np.array_equal(np.rint(b * 16), b * 16) and np.abs(b).max() <= 2.5
    assert (np.signbit(b1) & (b1 == 0)).any() and np.signbit(b2[0]).all() and (b2[0] == 0).all()        # -0.0 among the biases
    assert not w1[2].any() and (b1[2] <= 0).all() and (b1[1] > 0).any()                                   # env 2: every unit dead
    assert not p[9].any() and not np.signbit(p[9]).any()                                                  # env 9: the +0.0 block
    for e, pat in [(1, [(1, 4), (2, 3)]), (6, [(0, 1, 2, 3, 4, 5)]), (8, [(0, 5)])]:
        for g in pat:
            for k in g[1:]:
                assert np.array_equal(pe.bits(w2[e, k]), pe.bits(w2[e, g[0]])) and pe.bits(b2[e, k:k + 1]) == pe.bits(b2[e, g[0]:g[0] + 1])
    assert (w2[3] == w2[3, 2]).all() and b2[3, 2] == b2[3, 4] and (np.delete(b2[3], [2, 4]) < b2[3, 2]).all()      # "top": {2, 4} above the rest
    W = pe.dyadic_params(6, D, A, n, tie_groups=pe.tie_patterns(A))
    assert W.dtype == np.float64 and W.shape == (n, D, A) and np.isin(W, pe.WEIGHTS).all()
    assert np.array_equal(W[0, :, 0], W[0, :, 5]) and np.array_equal(W[3, :, 2], W[3, :, 4]) and np.array_equal(W[3, :, 0] * 2, W[3, :, 2])


@pytest.mark.parametrize("family,case", pe.ALL_CASES, ids=["{}-{}".format(f, "-".join(str(x) for x in c)) for f, c in pe.ALL_CASES])
def test_closed_loop_on_the_cpu_oracle_is_exact_and_reaches_what_the_case_is_for(family, case):
    """The policy against the CPU oracle alone.  The share of non-exact triples is capped at 1 % (a cap so that the tolerance fallback
    of the GPU test cannot hide a failure, not a measurement; a triple is non-exact only when some nonzero |x_d| < ~2^-15, so the share
    should be 0 — profiles/NOTES.md has the figures).  A case over the cap, or a Kuka case with an IK flag, gets another seed."""
    r = pe.closed_loop_report(family, case)
    print(family, case, r)
    assert r["share"] <= pe.MAX_SHARE
    assert r["flags"] == 0
    if "clamp" in r:
        assert r["clamp"] == (True, True, True), "+clip, -clip and the interior all have to occur"
    discrete = case[1]
    ties_wanted = discrete and (family != "mobile_linear" or case[6] is not None)
    if ties_wanted:
        assert r["ties"] > 0
        per_env = case[4] if family == "mobile_linear" else (case[5] if family == "mobile_mlp" else case[6])
        kind1 = family != "kuka" and case[0] == 1
        if per_env and not kind1 and "zero" not in case:
            assert r["ties_off0"] > 0, "a tied maximum away from index 0"
    if family == "mobile_linear" and case[6] == "zero":
        assert r["ties"] == r["steps"]
