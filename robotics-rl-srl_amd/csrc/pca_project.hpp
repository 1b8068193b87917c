// pca_project.hpp — the arithmetic, the limits and the refusal rules of srlhip_pca_* (contract: include/srlhip.h), host + gfx950 device code.
//
// One definition of every step that fixes a bit of a state — a term, the ORDER in which the F terms of a state are summed, the bias, the
// rounding to float32 — called by the kernel of pca_project.hip, by the library's host twin srlhip_pca_project_host and by the stand-alone
// host program pca_project_hostcheck.cpp (make pcahostcheck); tests/pca_ref.py restates it in numpy.  The products are explicit fma()
// calls: every user is built with -ffp-contract=off, so nothing else fuses.
//
// THE ORDER, a function of F alone.  W is [F][S] float64 (whitened, transposed: SRLPCA.set_model's _w), b is [S] (-(mean_ @ W)).  The
// features f = 0 .. F - 1 are cut into CHUNKS of kPcaChunk features (the last one ragged).  A chunk's sum starts from +0.0 and takes
// its features in ascending order, acc = fma((double)x[i][f], W[f][s], acc): the byte as it lies, no / 255.  The state is the chunks'
// sums added in ascending chunk order, starting with chunk 0's; b[s] is added last; with states_f32 the float64 state is rounded once to
// float32.  Nothing of this depends on n, on the frame's place in the batch, on the grid or on how many workgroups share a frame's chunks.
//
// A ZERO TERM CHANGES NOTHING: the kernel pads a ragged chunk (and S up to its register tile) with x = 0 and W = +0.0.  acc is never
// -0.0 — it starts from +0.0, an exact cancellation rounds to +0.0 and (+0.0) + (+-0.0) = +0.0 — so fma(0, +0.0, acc) = acc bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "api_rules.hpp"
#include "rng.hpp"

namespace srl {

constexpr int kPcaChunk = 512;                    // features per chunk
constexpr int kPcaMaxDim = 64;                    // S <= 64 (the reference's baselines: 5, 10, 32)

inline int64_t pca_chunks(int64_t F) { return (F + kPcaChunk - 1) / kPcaChunk; }

// the shapes a projector takes: anything else is SRLHIP_ENOTSUP and the caller keeps the torch formulation
inline Verdict check_pca_shape(int64_t n_features, int32_t state_dim) {
    if (n_features < 1) return {SRLHIP_ENOTSUP, "pca: n_features must be at least 1"};
    if (state_dim < 1 || state_dim > kPcaMaxDim) return {SRLHIP_ENOTSUP, "pca: state_dim must be 1..64"};
    return {0, nullptr};
}

// a forward's arguments: n = 0 is a successful call that launches nothing
inline Verdict check_pca_forward(int32_t n, bool has_images, bool has_states, int32_t states_f32) {
    if (n < 0) return {SRLHIP_EINVAL, "pca: n must not be negative"};
    if (states_f32 != 0 && states_f32 != 1) return {SRLHIP_EINVAL, "pca: states_f32 is 0 (float64 states) or 1 (float32)"};
    if (n > 0 && (!has_images || !has_states)) return {SRLHIP_EINVAL, "pca: null images or states"};
    return {0, nullptr};
}

// one feature's term joins a chunk's sum
SRL_HD double pca_step(double acc, uint8_t x, double w) { return fma((double)x, w, acc); }

// a chunk's sum joins the state
SRL_HD double pca_chunk_join(bool first, double state, double chunk_sum) {
#pragma clang fp contract(off)
    return first ? chunk_sum : state + chunk_sum;
}

// the bias, last
SRL_HD double pca_finish(double state, double bias) {
#pragma clang fp contract(off)
    return state + bias;
}

// the state leaves as float64, or rounded once to float32
SRL_HD void pca_store(void *states, int64_t at, bool states_f32, double v) {
    if (states_f32) static_cast<float *>(states)[at] = (float)v;
    else static_cast<double *>(states)[at] = v;
}

// The whole contract, one frame and one column at a time: the host twin and the host check program.  x [F], w [F][S], b [S].
inline double pca_project_one(const uint8_t *x, const double *w, const double *b, int64_t F, int32_t S, int32_t s) {
    double state = 0.0;
    const int64_t nc = pca_chunks(F);
    for (int64_t c = 0; c < nc; c++) {
        const int64_t f1 = (c + 1) * kPcaChunk < F ? (c + 1) * kPcaChunk : F;
        double acc = 0.0;
        for (int64_t f = c * kPcaChunk; f < f1; f++) acc = pca_step(acc, x[f], w[f * S + s]);
        state = pca_chunk_join(c == 0, state, acc);
    }
    return pca_finish(state, b[s]);
}

// images [n][F] -> states [n][S] (float64, or float32 with states_f32); the arguments have passed check_pca_shape / check_pca_forward
inline void pca_project_host(int64_t F, int32_t S, const double *w, const double *b, const uint8_t *images, int32_t n, void *states, bool states_f32) {
    for (int64_t i = 0; i < n; i++)
        for (int32_t s = 0; s < S; s++) pca_store(states, i * S + s, states_f32, pca_project_one(images + i * F, w, b, F, S, s));
}

// ---- the launch's shape (not the arithmetic: no bit depends on it) --------------------------------------------------------------------
constexpr int kPcaThreads = 256;                  // a workgroup
constexpr int kPcaFR = 4;                         // frames of a lane's register tile
constexpr int kPcaKT = 64;                        // features staged in LDS at a time
constexpr int64_t kPcaScratchBytes = 512ll << 20;  // the chunk sums of one launch stay within this (or are one frame tile's)
constexpr int kPcaLdsPerGroup = 56 * 1024;        // LDS a workgroup of 16 or more columns claims: two workgroups per compute unit (measured: a
                                                  // third and fourth, which the registers would allow, make 4096 frames of 224 x 224 x 3 slower)

// S padded up to the kernel's column tile: 8, 16, 32 or 64
inline int pca_padded_dim(int32_t S) { return S <= 8 ? 8 : S <= 16 ? 16 : S <= 32 ? 32 : 64; }
// columns of a lane's register tile, and the frames of a workgroup's tile, for a padded dimension
constexpr int pca_lane_cols(int SP) { return SP == 8 ? 4 : 8; }
constexpr int pca_tile_frames(int SP) { return kPcaFR * (kPcaThreads / (SP / pca_lane_cols(SP))); }
inline int64_t pca_tiles(int64_t n, int SP) { return (n + pca_tile_frames(SP) - 1) / pca_tile_frames(SP); }
// Every chunk of a frame tile gets a workgroup of its own and the chunk sums meet in a partial buffer.  The frame tiles of one launch:
// as many as keep that buffer within kPcaScratchBytes, at least one; a larger batch goes as several launches, slab after slab.
inline int64_t pca_slab_tiles(int64_t tiles, int64_t chunks, int SP) {
    if (chunks <= 1) return tiles;
    const int64_t per_tile = chunks * pca_tile_frames(SP) * SP * (int64_t)sizeof(double);
    const int64_t fit = kPcaScratchBytes / per_tile < 1 ? 1 : kPcaScratchBytes / per_tile;
    return fit < tiles ? fit : tiles;
}

}  // namespace srl
