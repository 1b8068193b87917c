// cnn_policy.hpp — the per-env arithmetic of srlhip_cnn_policy_act (contract: include/srlhip.h), host + gfx950 device code.
//
// One definition of every step that fixes a bit of a score — the input, a pool cell of a convolution with its summation ORDER, the
// statistics' partial sums and the tree that combines them, the normalisation, the linear layer — called by the kernel of cnn_policy.hip
// and by the stand-alone host program cnn_policy_hostcheck.cpp (make cnnpolicyhostcheck), which walks the workgroup's threads one after
// the other.  Build every user with -ffp-contract=off: no product may fuse with its sum.  Then the device's scores are the host
// program's bit for bit (tests/test_gpu_cnn_policy.py), and both are held to the float64 restatement tests/cnn_policy_ref.py.
// The selection behind the scores is policy_act.hpp's, on (double)score_a.
//
// A layer is walked in POOL CELLS: cell (pi, pj) holds the conv outputs (2 pi + dy, 2 pj + dx), dy, dx in {0, 1}.  The cells cover
// the whole conv plane (an odd plane's last row / column sits in cells the pool drops: they count for the statistics only).  The
// workgroup's kCnnBlock threads are split into G = CO / CG groups of TG threads; group g owns the output channels g CG .. g CG + CG - 1,
// its thread u the cells u, u + TG, ... in that order.
#pragma once
#include <math.h>
#include <stdint.h>

#include "api_rules.hpp"
#include "rng.hpp"

namespace srl {

constexpr int kCnnBlock = 256;
constexpr int kCnnCg1 = 8, kCnnCg2 = 4, kCnnCg3 = 2;      // channels per thread: 1, 4 and 16 groups of 256, 64 and 16 threads
constexpr double kCnnEps = 1e-5;

// the network's input: obs / 255.0 in float64 (numpy), then torch's cast to float32
SRL_HD float cnn_input(uint8_t b) { return (float)((double)b / 255.0); }

// The four conv outputs of cell (pi, pj) for the CG channels from c0: acc[k][2 dy + dx].  in(ci, r, c): the layer's input, 0 outside the
// plane.  wt: the layer's weights TRANSPOSED to [ci][ky][kx][CO] (cnn_weight_slot).  Every chain starts from +0 and takes its taps in
// (ci, ky, kx) order, padding taps included (they add a zero).
template <int K, int PAD, int CG, class In>
SRL_HD void cnn_cell(const In &in, int Cin, int CO, int c0, const float *wt, int pi, int pj, float (&acc)[CG][4]) {
#pragma clang fp contract(off)
    constexpr int PS = K + 2;      // the patch's side: rows 4 pi - PAD .. 4 pi - PAD + K + 1
#pragma unroll
    for (int k = 0; k < CG; k++)
#pragma unroll
        for (int p = 0; p < 4; p++) acc[k][p] = 0.f;
    for (int ci = 0; ci < Cin; ci++) {
        float patch[PS][PS];
#pragma unroll
        for (int r = 0; r < PS; r++)
#pragma unroll
            for (int c = 0; c < PS; c++) patch[r][c] = in(ci, 4 * pi - PAD + r, 4 * pj - PAD + c);
        const float *wc = wt + (size_t)ci * K * K * CO + c0;
#pragma unroll
        for (int ky = 0; ky < K; ky++)
#pragma unroll
            for (int kx = 0; kx < K; kx++) {
                float w[CG];
#pragma unroll
                for (int k = 0; k < CG; k++) w[k] = wc[(ky * K + kx) * CO + k];
#pragma unroll
                for (int k = 0; k < CG; k++)
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const float t = w[k] * patch[2 * (p >> 1) + ky][2 * (p & 1) + kx];
                        acc[k][p] = acc[k][p] + t;
                    }
            }
    }
}
// where element [c][ci][ky][kx] of a conv weight block ([CO][Cin][K][K], parameters() order) sits in the transposed block
SRL_HD int cnn_weight_slot(int i, int Cin, int KK, int CO) {
    const int c = i / (Cin * KK), rest = i % (Cin * KK);
    return rest * CO + c;
}

// What a thread does with a cell's outputs: the valid ones join its channel sums (position order), and a cell the pool keeps leaves its
// window's extreme — the max where gamma >= 0, the min where gamma < 0 — in the pooled plane [CO][hp][wp].
template <int CG>
SRL_HD void cnn_cell_finish(const float (&acc)[CG][4], int pi, int pj, int hc, int wc, int c0, const float *gamma, double *S, double *Q, float *pooled) {
#pragma clang fp contract(off)
    const int hp = hc / 2, wp = wc / 2;
#pragma unroll
    for (int k = 0; k < CG; k++) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (2 * pi + (p >> 1) < hc && 2 * pj + (p & 1) < wc) {
                const double x = (double)acc[k][p], x2 = x * x;
                S[k] = S[k] + x;
                Q[k] = Q[k] + x2;
            }
        }
        if (pi < hp && pj < wp) {
            const bool lo = gamma[c0 + k] < 0.f;
            float m = acc[k][0];
#pragma unroll
            for (int p = 1; p < 4; p++) m = lo ? (acc[k][p] < m ? acc[k][p] : m) : (acc[k][p] > m ? acc[k][p] : m);
            pooled[((size_t)(c0 + k) * hp + pi) * wp + pj] = m;
        }
    }
}

// the threads' partial sums combined: a balanced pairwise tree in thread order (what a butterfly of lane exchanges leaves in lane 0)
SRL_HD double cnn_tree_sum(double *v, int n) {
#pragma clang fp contract(off)
    for (int s = 1; s < n; s *= 2)
        for (int i = 0; i + s < n; i += 2 * s) v[i] = v[i] + v[i + s];
    return v[0];
}

// a channel's statistics from its sums over the n values of the conv plane -> mean and g = gamma / sqrt(var + eps)
SRL_HD void cnn_channel_stats(double S, double Q, int n, float gamma, double *mean, double *g) {
#pragma clang fp contract(off)
    const double m = S / (double)n, m2 = m * m;
    double var = Q / (double)n - m2;
    var = var > 0.0 ? var : 0.0;
    *mean = m;
    *g = (double)gamma / sqrt(var + kCnnEps);
}
// batch-norm and ReLU of one pooled value
SRL_HD float cnn_normalise(float x, double mean, double g, float beta) {
#pragma clang fp contract(off)
    const double d = (double)x - mean, t = d * g;
    const float y = (float)(t + (double)beta);
    return y > 0.f ? y : 0.f;
}

// the linear layer: float64 from the bias, f ascending, rounded once
SRL_HD float cnn_fc(const float *w_row, float bias, const float *x, int F) {
#pragma clang fp contract(off)
    double acc = (double)bias;
    for (int f = 0; f < F; f++) {
        const double t = (double)w_row[f] * (double)x[f];
        acc = acc + t;
    }
    return (float)acc;
}

}  // namespace srl
