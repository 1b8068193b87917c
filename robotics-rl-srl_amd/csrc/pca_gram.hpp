// pca_gram.hpp — the arithmetic, the limits, the refusal rules and the index math of srlhip_pca_gram (contract: include/srlhip.h), host +
// gfx950 device code.  Called by the kernels of pca_gram.hip, by the library's host twin srlhip_pca_gram_host and by the stand-alone host
// program pca_gram_hostcheck.cpp (make pcagramhostcheck); tests/pca_gram_ref.py restates it in numpy.
//
// DEFINITION.  x uint8 [N][F] row-major.  gram[i][j] = sum_f x[i][f] x[j][f] as int64 [N][N], full and symmetric; rowsum[i] = sum_f x[i][f]
// as int64 [N].  Exact integers: every summation order gives the same bits, so no order is part of the contract.
//
// SHIFT.  The int8 matrix instruction multiplies SIGNED bytes, so the kernel works on s = x - 128 (x ^ 0x80 per byte):
//     x y = s t + 128 (x + y) - 16384,     gram[i][j] = S[i][j] + 128 (rowsum[i] + rowsum[j]) - 16384 F,
// S the signed product sum over the F real features only: a padding byte (past F, or a row past N) is a signed 0 — masked AFTER the xor,
// never read from memory.
//
// CHUNK.  |s t| <= 128 x 128 = 16384, so kGramChunk = 65536 features sum to at most 2^30 in magnitude: an int32 accumulator takes one
// chunk and is then added into int64.  224 x 224 x 3 = 150528 features are three chunks.
//
// SHAPES.  1 <= N <= kGramMaxFrames, 1 <= F, 2 N^2 F 65025 < 2^63 — the last keeps fit_pca's integer centring (N^2 gram - N R_i - N R_j + S,
// every term below N^2 F 65025) in int64.  |gram| <= F 65025 itself is far below that.
#pragma once
#include <stdint.h>

#include "api_rules.hpp"
#include "rng.hpp"

namespace srl {

constexpr int64_t kGramChunk = 65536;             // features an int32 accumulator takes
constexpr int kGramMaxFrames = 8192;              // N
constexpr int kGramTile = 32;                     // an output tile is 32 x 32 frames: one v_mfma_i32_32x32x32_i8 accumulator
constexpr int kGramStep = 32;                     // features of one matrix instruction: lane half h = lane >> 5 holds 16 of them
constexpr int kGramPiece = 16;                    // bytes of one lane's operand
constexpr int64_t kGramChunkSteps = kGramChunk / kGramStep;
constexpr int kGramUnroll = 4;                    // steps in flight per loop trip of the kernel: 128 bytes of each row
constexpr int64_t kGramMinSliceSteps = 16;        // the automatic split leaves a K-slice at least 512 features
constexpr int64_t kGramTargetWaves = 2048;        // ... and stops splitting once the launch has this many wavefronts (256 CUs x 8)

// ---- the arithmetic -------------------------------------------------------------------------------------------------------------------
// four bytes x -> four signed bytes x - 128, of which only the lowest `valid` (0..4) are real: the others are a signed 0
SRL_HD uint32_t gram_signed_word(uint32_t w, int valid) {
    const uint32_t mask = valid >= 4 ? 0xffffffffu : valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
    return (w ^ 0x80808080u) & mask;
}
// S -> gram: the shift identity (on slice 0's share only; the other slices add their bare sums)
SRL_HD int64_t gram_unshift(int64_t signed_sum, int64_t rowsum_i, int64_t rowsum_j, int64_t F) {
    return signed_sum + 128 * (rowsum_i + rowsum_j) - 16384 * F;
}
// the largest magnitude an int32 accumulator reaches over `features` features
constexpr int64_t gram_chunk_bound(int64_t features) { return features * 16384; }
static_assert(gram_chunk_bound(kGramChunk) == (int64_t)1 << 30 && gram_chunk_bound(kGramChunk) <= INT32_MAX, "a chunk fits an int32");
static_assert(gram_chunk_bound(2 * kGramChunk) > INT32_MAX, "two chunks do not");

// ---- the rules ------------------------------------------------------------------------------------------------------------------------
inline bool pca_gram_supported(int64_t N, int64_t F) {
    if (N < 1 || N > kGramMaxFrames || F < 1) return false;
    return F <= (((int64_t)1 << 62) - 1) / (N * N * 65025);          // 2 N^2 F 65025 < 2^63
}
inline Verdict check_pca_gram(int64_t N, int64_t F, int32_t split, bool has_frames, bool has_gram, bool has_rowsum) {
    if (N < 1 || N > kGramMaxFrames) return {SRLHIP_ENOTSUP, "pca_gram: n must be 1..8192"};
    if (F < 1) return {SRLHIP_ENOTSUP, "pca_gram: n_features must be at least 1"};
    if (!pca_gram_supported(N, F)) return {SRLHIP_ENOTSUP, "pca_gram: 2 n^2 n_features 65025 must stay below 2^63"};
    if (split < 0) return {SRLHIP_EINVAL, "pca_gram: split is 0 (automatic) or the number of K-slices"};
    if (!has_frames || !has_gram || !has_rowsum) return {SRLHIP_EINVAL, "pca_gram: null frames, gram or rowsum"};
    return {0, nullptr};
}

// ---- the index math (no bit of the result depends on it) --------------------------------------------------------------------------------
// tiles: only the upper triangle tj >= ti is computed, the mirror is written with it.  Work item t = 0 .. tiles_upper - 1 walks the rows
// of the triangle: row ti has tiles_side - ti items.
SRL_HD int64_t gram_tiles_side(int64_t N) { return (N + kGramTile - 1) / kGramTile; }
SRL_HD int64_t gram_tiles_upper(int64_t N) { const int64_t T = gram_tiles_side(N); return T * (T + 1) / 2; }
SRL_HD void gram_tile_of(int64_t t, int64_t side, int *ti, int *tj) {
    int i = 0;
    while (t >= side - i) { t -= side - i; i++; }
    *ti = i; *tj = i + (int)t;
}
// split-K: the F features are ceil(F / 32) steps; a split into `split` slices gives every slice per = ceil(steps / split) steps, slice s
// takes [s per, min((s + 1) per, steps)), and ceil(steps / per) slices are not empty: a forced split larger than the steps there are
// launches no idle workgroups.  The kernel is told `per` and the number of slices, not the split.
SRL_HD int64_t gram_steps(int64_t F) { return (F + kGramStep - 1) / kGramStep; }
SRL_HD int64_t gram_slice_steps(int64_t F, int64_t split) { return (gram_steps(F) + split - 1) / split; }
SRL_HD int64_t gram_slices(int64_t F, int64_t per) { return (gram_steps(F) + per - 1) / per; }
// split = 0: enough slices that tiles x slices reaches kGramTargetWaves, none shorter than kGramMinSliceSteps
inline int64_t gram_auto_split(int64_t N, int64_t F) {
    const int64_t tiles = gram_tiles_upper(N), steps = gram_steps(F);
    int64_t want = (kGramTargetWaves + tiles - 1) / tiles, most = steps / kGramMinSliceSteps;
    if (most < 1) most = 1;
    return want < most ? want : most;
}
SRL_HD void gram_slice_range(int64_t F, int64_t per, int64_t s, int64_t *step0, int64_t *step1) {
    const int64_t steps = gram_steps(F);
    *step0 = s * per < steps ? s * per : steps;
    *step1 = (s + 1) * per < steps ? (s + 1) * per : steps;
}
// One load: lane half h of step `step` takes, of frame `row`, the bytes [begin, begin + count) of the frames' array, count = 0 .. 16 —
// nothing for a row at or past N, a feature at or past F, or a step at or past `step_end` (the kernel walks a chunk of a slice in trips of
// kGramUnroll steps, so its last trip may reach past the chunk's end).  The kernel touches these bytes and no others.
SRL_HD int gram_piece_valid(int64_t F, int64_t step, int h) {
    const int64_t left = F - (step * kGramStep + (int64_t)h * kGramPiece);
    return left <= 0 ? 0 : left >= kGramPiece ? kGramPiece : (int)left;
}
SRL_HD void gram_load_range(int64_t N, int64_t F, int64_t row, int64_t step, int64_t step_end, int h, int64_t *begin, int *count) {
    *count = row < N && step < step_end ? gram_piece_valid(F, step, h) : 0;
    *begin = row * F + step * kGramStep + (int64_t)h * kGramPiece;
}
// the 16-byte load form: every piece is whole or absent and 16-byte aligned
inline bool gram_vec16(int64_t F, uintptr_t base) { return F % kGramPiece == 0 && base % kGramPiece == 0; }

// ---- the host twin: plain int64 loops ------------------------------------------------------------------------------------------------
inline void pca_gram_host(const uint8_t *x, int64_t N, int64_t F, int64_t *gram, int64_t *rowsum) {
    for (int64_t i = 0; i < N; i++) {
        int64_t r = 0;
        for (int64_t f = 0; f < F; f++) r += x[i * F + f];
        rowsum[i] = r;
        for (int64_t j = i; j < N; j++) {
            int64_t acc = 0;
            for (int64_t f = 0; f < F; f++) acc += (int64_t)x[i * F + f] * (int64_t)x[j * F + f];
            gram[i * N + j] = acc;
            gram[j * N + i] = acc;
        }
    }
}

// The kernel's own route on the host, one output at a time: signed bytes through gram_signed_word, int32 chunks of kGramChunk features
// flushed into int64, the slices of a split added up, the shift undone on slice 0 (pca_gram_hostcheck.cpp holds it against the twin).
inline int64_t pca_gram_signed_route(const uint8_t *x, int64_t N, int64_t F, int64_t i, int64_t j, int64_t split, const int64_t *rowsum) {
    int64_t total = 0;
    const int64_t per = gram_slice_steps(F, split), nslices = gram_slices(F, per);
    for (int64_t s = 0; s < nslices; s++) {
        int64_t step0, step1, acc64 = 0;
        gram_slice_range(F, per, s, &step0, &step1);
        for (int64_t c0 = step0; c0 < step1; c0 += kGramChunkSteps) {
            int32_t acc32 = 0;
            const int64_t c1 = c0 + kGramChunkSteps < step1 ? c0 + kGramChunkSteps : step1;
            for (int64_t step = c0; step < c1; step++)
                for (int h = 0; h < 2; h++) {
                    const int valid = gram_piece_valid(F, step, h);
                    for (int w = 0; w < 4; w++) {
                        const int64_t k = step * kGramStep + h * kGramPiece + w * 4;
                        const int v = valid - 4 * w;
                        uint32_t a = 0, b = 0;
                        for (int q = 0; q < 4 && q < v; q++) {
                            a |= (uint32_t)x[i * F + k + q] << (8 * q);
                            b |= (uint32_t)x[j * F + k + q] << (8 * q);
                        }
                        a = gram_signed_word(a, v); b = gram_signed_word(b, v);
                        for (int q = 0; q < 4; q++) acc32 += (int32_t)(int8_t)(a >> (8 * q)) * (int32_t)(int8_t)(b >> (8 * q));
                    }
                }
            acc64 += acc32;
        }
        total += s == 0 ? gram_unshift(acc64, rowsum[i], rowsum[j], F) : acc64;
    }
    (void)N;
    return total;
}

}  // namespace srl
