// pixel_policy.hpp — the per-env arithmetic of srlhip_pixel_policy_act (contract: include/srlhip.h), host + gfx950 device code.
//
// One definition of every step that fixes a bit of a score — the weight an env sees, a term, the ORDER in which the D terms of a score
// are summed — called by the kernel of pixel_policy.hip and by the stand-alone host program pixel_policy_hostcheck.cpp
// (make pixelpolicyhostcheck), which tests/test_pixel_policy_cpu.py holds to the numpy restatement tests/pixel_policy_ref.py bit for
// bit.  Build every user with -ffp-contract=off: no product may fuse with its sum.  The selection behind the scores is policy_act.hpp's.
//
// THE ORDER, a function of (D, A) alone.  The rows d = 0 .. D - 1 are cut into CHUNKS of kPixChunk rows (the last one ragged).  Inside a
// chunk kPixLanes virtual lanes share the rows: lane v owns the rows c kPixChunk + v + kPixLanes j, j = 0, 1, ..., and adds their
// terms in that order to a partial that starts from +0.0 (rows at or past D add nothing).  The kPixLanes partials meet in a fixed
// pairwise tree, far halves first: v[i] = v[i] + v[i + h] for i < h, h = kPixLanes / 2, ..., 1; v[0] is the chunk's sum.  The score is
// the chunks' sums added in ascending order, starting with chunk 0's.  A launch may give a chunk to a workgroup of its own or walk all
// of them in one: the bits are the same.
#pragma once
#include <stdint.h>

#include "api_rules.hpp"
#include "rng.hpp"

namespace srl {

constexpr int kPixLanes = 256;                    // virtual lanes = the workgroup's threads
constexpr int kPixChunk = 2048;                   // rows per chunk: 8 per lane
constexpr int kPixSteps = kPixChunk / kPixLanes;
constexpr int kPixMaxOut = 8;

inline int pix_chunks(int64_t D) { return (int)((D + kPixChunk - 1) / kPixChunk); }

// the two weights of a direction: env 2k sees M + noise * delta, env 2k + 1 sees M - noise * delta (ars.py:162-166)
SRL_HD void pix_weights(double m, double delta, double noise, double *w_plus, double *w_minus) {
#pragma clang fp contract(off)
    const double t = noise * delta;
    *w_plus = m + t;
    *w_minus = m - t;
}

// one row's term joins a lane's partial: the frame byte as it lies, float64 (np.dot(obs.reshape(-1), W): no / 255)
SRL_HD double pix_step(double acc, uint8_t x, double w) {
#pragma clang fp contract(off)
    const double t = (double)x * w;
    return acc + t;
}

// the tree over the chunk's lane partials: v [kPixLanes][stride], column `col`; the kernel runs the same levels across its threads
SRL_HD double pix_tree_sum(double *v, int stride, int col) {
#pragma clang fp contract(off)
    for (int h = kPixLanes / 2; h >= 1; h /= 2)
        for (int i = 0; i < h; i++) v[(size_t)i * stride + col] = v[(size_t)i * stride + col] + v[(size_t)(i + h) * stride + col];
    return v[col];
}

// a chunk's sum joins the score
SRL_HD double pix_chunk_join(bool first, double score, double chunk_sum) {
#pragma clang fp contract(off)
    return first ? chunk_sum : score + chunk_sum;
}

}  // namespace srl
