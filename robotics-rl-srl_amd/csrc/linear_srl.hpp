// linear_srl.hpp — the arithmetic, the limits and the refusal rules of srlhip_linear_srl_* (contract: include/srlhip.h), host + gfx950
// device code.  The trainable linear state encoder, state = fc(flatten(preprocess(frame))) [srl_zoo's `--model-type linear`; srl_zoo is
// an empty submodule of the reference checkout: recalled, UNVERIFIED], as a forward and a fused gradient + Adam step on the uint8 frames.
//
// One definition of every step that fixes a bit — called by the kernels of linear_srl.hip, by the library's host twins
// srlhip_linear_srl_forward_host / srlhip_linear_srl_step_host and by the stand-alone host program linear_srl_hostcheck.cpp
// (make linearsrlhostcheck); tests/linear_srl_ref.py restates it in numpy.  Every user is built with -ffp-contract=off: the only fused
// operations are the explicit fma() calls below.
//
// THE NORMALISED PIXEL.  frames are uint8 [n][F], flattened NHWC; feature f belongs to channel ch = f mod C.  With the host tables
// scale[C] and offset[C] (the caller passes 1 / (255 std) and mean / std):  xn = fma(scale[ch], (double)x, -offset[ch])  — FUSED.
//
// FORWARD, a function of F alone (the order of the PCA contract, pca_project.hpp, with xn in the raw byte's place).  V is [F][S] float64,
// c is [S].  The features are cut into CHUNKS of kLinChunk = 512 (the last one ragged).  A chunk's sum starts from +0.0 and takes its
// features in ascending order, acc = fma(xn, V[f][s], acc) — FUSED.  The state is the chunks' sums added in ascending chunk order
// starting with chunk 0's (separate additions), then + c[s] (a separate addition).
//
// GRADIENT, a function of n alone.  G is [n][S] float64 (dL/dstate).  g[f][s] starts from +0.0; for i = 0 .. n - 1 ascending,
// g = fma(xn[i][f], G[i][s], g) — FUSED.  No atomics, no split over i: the bits do not depend on the launch's shape.
//
// ADAM, in place on V, m, v [F][S], every operation SEPARATE (a product is rounded before it is added), division and square root IEEE
// double (correctly rounded).  The caller passes bc1 = 1 - beta1^t and bc2 = 1 - beta2^t:
//     m = (beta1 * m) + ((1 - beta1) * g)
//     v = (beta2 * v) + (((1 - beta2) * g) * g)
//     V = V - ((lr / bc1) * (m / ((sqrt(v) / sqrt(bc2)) + eps)))
// (1 - beta1), (1 - beta2), lr / bc1 and sqrt(bc2) are each one rounded double, computed the same way by every user.
//
// NO PADDED TERM JOINS A STORED SUM.  An accumulator CAN be -0.0 here (a tiny negative product may underflow to it), and then a padded
// fma(xn, +0.0, acc) could flip its sign: so the kernels pad only what they never store (S up to the register tile, frames up to the
// frame tile) and bound their loops over the features of a ragged chunk and over the frames of a ragged stage exactly.
#pragma once
#include <math.h>
#include <stdint.h>

#include "api_rules.hpp"
#include "rng.hpp"

namespace srl {

constexpr int kLinChunk = 512;                    // features per chunk of the forward
constexpr int kLinMaxDim = 64;                    // S <= 64
constexpr int kLinMaxChannels = 8;                // C <= 8
constexpr int kLinMaxFrames = 1024;               // n <= 1024 per call

inline int64_t lin_chunks(int64_t F) { return (F + kLinChunk - 1) / kLinChunk; }

// the preprocessing tables, by value: a kernel argument
struct LinNorm {
    double scale[kLinMaxChannels], offset[kLinMaxChannels];
    int32_t C;
};

struct LinAdam { double lr, beta1, beta2, eps, bc1, bc2; };

// the shapes an encoder takes: anything else is SRLHIP_ENOTSUP
inline Verdict check_lin_shape(int64_t n_features, int32_t state_dim, int32_t n_channels) {
    if (n_features < 1) return {SRLHIP_ENOTSUP, "linear_srl: n_features must be at least 1"};
    if (state_dim < 1 || state_dim > kLinMaxDim) return {SRLHIP_ENOTSUP, "linear_srl: state_dim must be 1..64"};
    if (n_channels < 1 || n_channels > kLinMaxChannels) return {SRLHIP_ENOTSUP, "linear_srl: n_channels must be 1..8"};
    return {0, nullptr};
}

// a batch: 1 .. 1024 frames
inline Verdict check_lin_batch(int32_t n) {
    if (n < 1) return {SRLHIP_EINVAL, "linear_srl: n must be at least 1"};
    if (n > kLinMaxFrames) return {SRLHIP_ENOTSUP, "linear_srl: at most 1024 frames per call"};
    return {0, nullptr};
}

inline Verdict check_lin_tables(const double *scale, const double *offset, int32_t C) {
    if (!scale || !offset) return {SRLHIP_EINVAL, "linear_srl: null scale or offset table"};
    for (int32_t k = 0; k < C; k++)
        if (!isfinite(scale[k]) || !isfinite(offset[k])) return {SRLHIP_EINVAL, "linear_srl: a scale or offset is not finite"};
    return {0, nullptr};
}

inline Verdict check_lin_adam(const LinAdam &a) {
    if (!isfinite(a.lr)) return {SRLHIP_EINVAL, "linear_srl: lr is not finite"};
    if (!(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0)) return {SRLHIP_EINVAL, "linear_srl: beta1 and beta2 must be in [0, 1)"};
    if (!(a.eps >= 0.0) || !isfinite(a.eps)) return {SRLHIP_EINVAL, "linear_srl: eps must be finite and not negative"};
    if (!(a.bc1 > 0.0 && a.bc1 <= 1.0) || !(a.bc2 > 0.0 && a.bc2 <= 1.0)) return {SRLHIP_EINVAL, "linear_srl: bc1 and bc2 must be in (0, 1]"};
    return {0, nullptr};
}

inline LinNorm lin_norm(const double *scale, const double *offset, int32_t C) {
    LinNorm t{};
    t.C = C;
    for (int32_t k = 0; k < C; k++) { t.scale[k] = scale[k]; t.offset[k] = offset[k]; }
    return t;
}

// ---- the arithmetic -------------------------------------------------------------------------------------------------------------------
// the normalised pixel of a channel
SRL_HD double lin_xn(double scale, double offset, uint8_t x) { return fma(scale, (double)x, -offset); }

// one feature's term joins a chunk's sum (forward) or one frame's term joins a gradient (step)
SRL_HD double lin_step(double acc, double xn, double w) { return fma(xn, w, acc); }

// a chunk's sum joins the state
SRL_HD double lin_chunk_join(bool first, double state, double chunk_sum) {
#pragma clang fp contract(off)
    return first ? chunk_sum : state + chunk_sum;
}

// the bias, last
SRL_HD double lin_finish(double state, double bias) {
#pragma clang fp contract(off)
    return state + bias;
}

// what an Adam update needs once per launch
struct LinAdamK { double beta1, beta2, omb1, omb2, step, sqrt_bc2, eps; };

inline LinAdamK lin_adam_k(const LinAdam &a) {
#pragma clang fp contract(off)
    return {a.beta1, a.beta2, 1.0 - a.beta1, 1.0 - a.beta2, a.lr / a.bc1, sqrt(a.bc2), a.eps};
}

// one parameter's update from its finished gradient
SRL_HD void lin_adam(const LinAdamK &k, double g, double *V, double *m, double *v) {
#pragma clang fp contract(off)
    const double t1 = k.beta1 * *m, t2 = k.omb1 * g;
    const double mn = t1 + t2;
    const double t3 = k.beta2 * *v, t4 = k.omb2 * g;
    const double t5 = t4 * g;
    const double vn = t3 + t5;
    const double r = sqrt(vn);
    const double q = r / k.sqrt_bc2;
    const double den = q + k.eps;
    const double u = mn / den;
    const double d = k.step * u;
    *m = mn;
    *v = vn;
    *V = *V - d;
}

// ---- the host twins (the arguments have passed the checks) --------------------------------------------------------------------------------
inline double lin_forward_one(const uint8_t *x, const LinNorm &t, const double *V, const double *c, int64_t F, int32_t S, int32_t s) {
    double state = 0.0;
    const int64_t nc = lin_chunks(F);
    for (int64_t ch = 0; ch < nc; ch++) {
        const int64_t f1 = (ch + 1) * kLinChunk < F ? (ch + 1) * kLinChunk : F;
        double acc = 0.0;
        for (int64_t f = ch * kLinChunk; f < f1; f++) {
            const int k = (int)(f % t.C);
            acc = lin_step(acc, lin_xn(t.scale[k], t.offset[k], x[f]), V[f * S + s]);
        }
        state = lin_chunk_join(ch == 0, state, acc);
    }
    return lin_finish(state, c[s]);
}

inline void lin_forward_host(const uint8_t *frames, int32_t n, int64_t F, int32_t S, const LinNorm &t, const double *V, const double *c, double *states) {
    for (int64_t i = 0; i < n; i++)
        for (int32_t s = 0; s < S; s++) states[i * S + s] = lin_forward_one(frames + i * F, t, V, c, F, S, s);
}

inline void lin_step_host(const uint8_t *frames, int32_t n, int64_t F, int32_t S, const LinNorm &t, const double *G, double *V, double *m, double *v,
                          const LinAdam &adam, double *grad_out) {
    const LinAdamK k = lin_adam_k(adam);
    for (int64_t f = 0; f < F; f++) {
        const int ch = (int)(f % t.C);
        double g[kLinMaxDim];
        for (int32_t s = 0; s < S; s++) g[s] = 0.0;
        for (int64_t i = 0; i < n; i++) {
            const double xn = lin_xn(t.scale[ch], t.offset[ch], frames[i * F + f]);
            for (int32_t s = 0; s < S; s++) g[s] = lin_step(g[s], xn, G[i * S + s]);
        }
        for (int32_t s = 0; s < S; s++) {
            if (grad_out) grad_out[f * S + s] = g[s];
            lin_adam(k, g[s], V + f * S + s, m + f * S + s, v + f * S + s);
        }
    }
}

// ---- the launches' shape (not the arithmetic: no bit depends on it) -------------------------------------------------------------------
constexpr int kLinThreads = 256;                  // a workgroup of the forward
constexpr int kLinFR = 2;                         // frames of a forward lane's register tile
constexpr int kLinKT = 64;                        // features the forward stages in LDS at a time
constexpr int kLinStepThreads = 128;              // a workgroup of the step: one lane per feature
constexpr int kLinStepRows = 32;                  // rows of G the step stages in LDS at a time

// forward: S padded up to the kernel's column tile, a lane's columns, the frames of a workgroup's tile
inline int lin_padded_dim(int32_t S) { return S <= 8 ? 8 : S <= 16 ? 16 : S <= 32 ? 32 : 64; }
constexpr int kLinCL = 8;
constexpr int lin_tile_frames(int SP) { return kLinFR * (kLinThreads / (SP / kLinCL)); }
inline int64_t lin_tiles(int64_t n, int SP) { return (n + lin_tile_frames(SP) - 1) / lin_tile_frames(SP); }
// the forward's workspace: every chunk's sums [chunks][n][SP]
inline size_t lin_workspace_bytes(int64_t F, int32_t S, int32_t n) {
    if (check_lin_shape(F, S, 1).code || check_lin_batch(n).code) return 0;
    return (size_t)(lin_chunks(F) * n * lin_padded_dim(S)) * sizeof(double);
}
// step: the columns a lane keeps in registers (a column group), a function of S alone
inline int lin_step_group(int32_t S) { return S <= 8 ? 8 : S <= 16 ? 16 : 32; }
inline int lin_step_groups(int32_t S) { return (S + lin_step_group(S) - 1) / lin_step_group(S); }
inline int64_t lin_step_blocks(int64_t F) { return (F + kLinStepThreads - 1) / kLinStepThreads; }

}  // namespace srl
