// knn.hpp — the arithmetic, the order, the limits, the refusal rules and the index math of srlhip_knn (contract: include/srlhip.h), host +
// gfx950 device code.  Called by the kernels of knn.hip, by the library's host twin srlhip_knn_host and by the stand-alone host program
// knn_hostcheck.cpp (make knnhostcheck); tests/knn_ref.py restates it in numpy.  What it scores: state_representation/evaluate.py (KNN-MSE).
//
// INPUTS.  states [N][S] float64, or float32 with states_f32 = 1 (each value widened exactly to float64 on load).  queries int32 [Q],
// indices into 0 .. N - 1, duplicates allowed; NULL means Q = N and queries[q] = q.  ground_truth optional, float64 [N][G].
//
// DISTANCE.  For query row i and candidate j: diff_s = x[i][s] - x[j][s] in float64, d = fma(diff_s, diff_s, d) for s = 0 .. S - 1 in
// ascending order starting from +0.0 (knn_distance_step).  No Gram-trick expansion, no reassociation: d(i, j) and d(j, i) are the same bits.
//
// NEIGHBOURS.  The k neighbours of i are the k smallest elements of {(d(i, j), j) : j != i} under the total order "smaller d first, then
// smaller j" (knn_before), listed ascending.  j == i is excluded by INDEX, not by distance: a duplicate state at another index is a
// legitimate neighbour at distance 0.  A candidate enters a list only through d < worst || (d == worst && j < worst_j): a NaN distance
// never enters, and neither does +inf (the empty slot is (-1, +inf)).  A list that cannot be filled keeps (-1, +inf) in its tail.
//
// OUTPUTS.  idx int32 [Q][k], dist float64 [Q][k].  With ground_truth, err float64 [Q]: i = queries[q], e from +0.0, n = 0 .. k - 1 outer
// and g = 0 .. G - 1 inner, t = gt[idx[q][n]][g] - gt[i][g], e = fma(t, t, e); err[q] = e / (double)k.  Slots with index -1 are skipped,
// the divisor stays k.
//
// SHAPES.  2 <= N <= 2^20, 1 <= S <= 64, 1 <= k <= min(32, N - 1), 1 <= Q <= 2^20, 1 <= G <= 32 (G = 0: no ground truth).
//
// The order is total and every operation is an IEEE float64 operation in a fixed sequence, so the result is unique: it does not depend
// on Q, on a query's place in the list, on the launch shape or on the split, and the device equals the host twin bit for bit (both sides
// are compiled with -ffp-contract=off; the only fused operations are the fma calls written here).
//
// A list in the kernels is KMAX >= k slots (KMAX a compile-time size, every slot in a register of its own): the first k of the KMAX
// smallest are the k smallest, so the extra slots change nothing.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "api_rules.hpp"
#include "rng.hpp"

namespace srl {

constexpr int kKnnMaxN = 1 << 20, kKnnMaxQ = 1 << 20, kKnnMaxS = 64, kKnnMaxK = 32, kKnnMaxG = 32;
constexpr int kKnnBlock = 256;                 // queries of a workgroup: one lane each
constexpr int kKnnTile = 64;                   // candidates staged in LDS at a time
constexpr int kKnnStep = 4;                    // distance steps the kernel runs without a test of S (rows are padded with +0.0)
constexpr int64_t kKnnTargetWaves = 2048;      // the automatic split stops once the launch has this many wavefronts (256 CUs x 8) ...
constexpr int64_t kKnnMinSlice = 1024;         // ... leaves a slice at least this many candidates (a short slice is all list insertions) ...
constexpr int64_t kKnnMaxAutoSlices = 64;      // ... and the merge at most this many lists per query

// ---- the arithmetic and the order ------------------------------------------------------------------------------------------------------
SRL_HD double knn_distance_step(double xi, double xj, double d) {
    const double diff = xi - xj;
    return fma(diff, diff, d);
}
// (d, j) comes before (wd, wj): the ONLY way into a list.  False for a NaN d and, against the empty slot (+inf, -1), for d = +inf.
SRL_HD bool knn_before(double d, int32_t j, double wd, int32_t wj) { return d < wd || (d == wd && j < wj); }

SRL_HD uint64_t knn_bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
SRL_HD double knn_double(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }

// a sorted list of KMAX slots, ascending; insertion keeps every index static so that the kernels' lists stay in registers
template <int KMAX> struct KnnList {
    double d[KMAX];
    int32_t j[KMAX];
    SRL_HD void clear() {
#pragma unroll
        for (int n = 0; n < KMAX; n++) { d[n] = INFINITY; j[n] = -1; }
    }
    SRL_HD bool admits(double cd, int32_t cj) const { return knn_before(cd, cj, d[KMAX - 1], j[KMAX - 1]); }
    // call only when admits(): the candidate takes the last slot and moves up one slot at a time while it comes before its lower
    // neighbour.  A step touches two slots and exchanges them through bit masks, not through ?: — the compiler turns a chain of
    // conditional exchanges into branches and a second copy of the list, which does not fit the registers beside a 64-value query.
    SRL_HD void insert(double cd, int32_t cj) {
        d[KMAX - 1] = cd; j[KMAX - 1] = cj;
#pragma unroll
        for (int n = KMAX - 1; n > 0; n--) {
            const uint64_t m = knn_before(d[n], j[n], d[n - 1], j[n - 1]) ? ~(uint64_t)0 : 0;
            const uint64_t a = knn_bits(d[n]), b = knn_bits(d[n - 1]), flip = (a ^ b) & m;
            const uint32_t jflip = ((uint32_t)j[n] ^ (uint32_t)j[n - 1]) & (uint32_t)m;
            d[n] = knn_double(a ^ flip); d[n - 1] = knn_double(b ^ flip);
            j[n] = (int32_t)((uint32_t)j[n] ^ jflip); j[n - 1] = (int32_t)((uint32_t)j[n - 1] ^ jflip);
        }
    }
    SRL_HD void offer(double cd, int32_t cj) { if (admits(cd, cj)) insert(cd, cj); }
};

// err of one query from its finished list
template <int KMAX> SRL_HD double knn_error(const KnnList<KMAX> &l, int32_t k, const double *gt, int32_t G, int64_t i) {
    double e = 0.0;
#pragma unroll
    for (int n = 0; n < KMAX; n++) {
        if (n >= k || l.j[n] < 0) continue;
        for (int g = 0; g < G; g++) {
            const double t = gt[(int64_t)l.j[n] * G + g] - gt[i * G + g];
            e = fma(t, t, e);
        }
    }
    return e / (double)k;
}

// ---- the rules ------------------------------------------------------------------------------------------------------------------------
inline Verdict check_knn_shape(int64_t N, int64_t S, int64_t k, int64_t Q, int64_t G) {
    if (N < 2 || N > kKnnMaxN) return {SRLHIP_ENOTSUP, "knn: n must be 2..2^20"};
    if (S < 1 || S > kKnnMaxS) return {SRLHIP_ENOTSUP, "knn: s must be 1..64"};
    if (k < 1 || k > kKnnMaxK) return {SRLHIP_ENOTSUP, "knn: k must be 1..32"};
    if (k > N - 1) return {SRLHIP_ENOTSUP, "knn: k must be at most n - 1"};
    if (Q < 1 || Q > kKnnMaxQ) return {SRLHIP_ENOTSUP, "knn: q must be 1..2^20"};
    if (G < 0 || G > kKnnMaxG) return {SRLHIP_ENOTSUP, "knn: g must be 1..32 (0: no ground truth)"};
    return kAccepted;
}
inline bool knn_supported(int64_t N, int64_t S, int64_t k, int64_t Q, int64_t G) { return check_knn_shape(N, S, k, Q, G).code == 0; }
// has_gt / has_err: the pointers; G: the caller's g
inline Verdict check_knn(int64_t N, int64_t S, int64_t k, int64_t Q, int64_t G, int32_t split, bool has_states, bool has_idx, bool has_dist,
                         bool has_gt, bool has_err) {
    const Verdict v = check_knn_shape(N, S, k, Q, has_gt || has_err ? (G < 1 ? -1 : G) : 0);
    if (v.code) return v;
    if (split < 0) return {SRLHIP_EINVAL, "knn: split is 0 (automatic) or the number of candidate slices"};
    if (!has_states || !has_idx || !has_dist) return {SRLHIP_EINVAL, "knn: null states, idx or dist"};
    if (has_gt != has_err) return {SRLHIP_EINVAL, "knn: ground_truth and err are both given or both null"};
    return kAccepted;
}

// ---- the index math (no bit of the result depends on it) --------------------------------------------------------------------------------
// candidate slices: a split into `split` slices gives every slice per = ceil(N / split) candidates rounded up to whole tiles, slice c takes
// [c per, min((c + 1) per, N)), and ceil(N / per) slices are not empty: those are launched.
SRL_HD int64_t knn_slice_len(int64_t N, int64_t split) {
    const int64_t per = (N + split - 1) / split;
    return (per + kKnnTile - 1) / kKnnTile * kKnnTile;
}
SRL_HD int64_t knn_slices(int64_t N, int64_t per) { return (N + per - 1) / per; }
SRL_HD int64_t knn_query_blocks(int64_t Q) { return (Q + kKnnBlock - 1) / kKnnBlock; }
inline int64_t knn_auto_split(int64_t N, int64_t Q) {
    const int64_t waves = knn_query_blocks(Q) * (kKnnBlock / 64);
    int64_t want = (kKnnTargetWaves + waves - 1) / waves, most = N / kKnnMinSlice;
    if (most > kKnnMaxAutoSlices) most = kKnnMaxAutoSlices;
    if (most < 1) most = 1;
    return want < most ? want : most;
}
inline int64_t knn_slice_len_for(int64_t N, int64_t Q, int32_t split) { return knn_slice_len(N, split > 0 ? split : knn_auto_split(N, Q)); }
// the partial lists: float64 dist [slices][k][Q], then int32 idx [slices][k][Q] (q fastest: a wavefront's accesses are contiguous)
SRL_HD int64_t knn_partial_at(int64_t slice, int64_t n, int64_t q, int64_t k, int64_t Q) { return (slice * k + n) * Q + q; }
inline size_t knn_workspace_bytes(int64_t N, int64_t S, int64_t k, int64_t Q, int32_t split) {
    if (!knn_supported(N, S, k, Q, 0) || split < 0) return 0;
    const int64_t slices = knn_slices(N, knn_slice_len_for(N, Q, split));
    return (size_t)(slices * k * Q) * (sizeof(double) + sizeof(int32_t));
}

// ---- the host twin -------------------------------------------------------------------------------------------------------------------
template <class T> inline void knn_host_rows(const T *x, int64_t N, int64_t S, const int32_t *queries, int64_t Q, int32_t k, const double *gt,
                                             int32_t G, int32_t *idx, double *dist, double *err) {
    for (int64_t q = 0; q < Q; q++) {
        const int64_t i = queries ? queries[q] : q;
        KnnList<kKnnMaxK> l;
        l.clear();
        for (int64_t j = 0; j < N; j++) {
            if (j == i) continue;
            double d = 0.0;
            for (int64_t s = 0; s < S; s++) d = knn_distance_step((double)x[i * S + s], (double)x[j * S + s], d);
            l.offer(d, (int32_t)j);
        }
        for (int n = 0; n < k; n++) { idx[q * k + n] = l.j[n]; dist[q * k + n] = l.d[n]; }
        if (gt) err[q] = knn_error(l, k, gt, G, i);
    }
}
// -> false when a query index is outside 0 .. N - 1 (nothing is written then)
inline bool knn_host(const void *states, int32_t states_f32, int64_t N, int64_t S, const int32_t *queries, int64_t Q, int32_t k, const double *gt,
                     int32_t G, int32_t *idx, double *dist, double *err) {
    if (queries)
        for (int64_t q = 0; q < Q; q++)
            if (queries[q] < 0 || queries[q] >= N) return false;
    if (states_f32) knn_host_rows(static_cast<const float *>(states), N, S, queries, Q, k, gt, G, idx, dist, err);
    else knn_host_rows(static_cast<const double *>(states), N, S, queries, Q, k, gt, G, idx, dist, err);
    return true;
}

}  // namespace srl
