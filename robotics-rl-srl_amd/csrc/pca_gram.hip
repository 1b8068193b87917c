// pca_gram.hip — srlhip_pca_gram: the Gram matrix X X^T and the row sums of N device-resident uint8 frames, exactly, on the int8 matrix
// pipe (include/srlhip.h has the contract; pca_gram.hpp the arithmetic, the rules and the index math).  The hot part of fitting the PCA
// state baseline (state_representation/pca_fit.py): everything behind it is N x N and small.
//
//   rows      pca_rowsum_k: one workgroup per frame sums its bytes (uint64 per lane, LDS tree), plain stores.
//   tiles     pca_gram_k: ONE WAVEFRONT per (32 x 32 output tile, K-slice).  Both operands of v_mfma_i32_32x32x32_i8 come from the same
//             row-major matrix: lane l holds 16 consecutive bytes of frame (tile row base + l & 31) at feature 32 step + 16 (l >> 5), as the
//             A operand for the tile's rows and as the B operand for its columns — the same (lane, byte) -> k map on both sides, so the
//             instruction's own order of k inside a step does not matter to a sum over k.  No LDS: the wavefronts of neighbouring tiles
//             share rows through the caches.  Bytes become signed with one xor per word, padding is masked to a signed 0 after it
//             (gram_signed_word), and slice 0 undoes the shift with the row sums (gram_unshift).
//   chunks    the int32 accumulator is added into 16 int64 registers every kGramChunk features.
//   split-K   only tiles with tj >= ti are computed, the mirror is written with them.  One slice: plain stores.  Several: the plane
//             is zeroed on the stream first (a kernel of its own) and every slice adds its share with 64-bit vector atomic adds (atomicAdd on unsigned long
//             long) — integer addition: the result does not depend on the split or on the order of arrival.
// Every global access is guarded by gram_load_range / the frame index; every offset is 64-bit.
#include <string>

#include "internal.hpp"
#include "pca_gram.hpp"

namespace srl {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int kRowsumThreads = 256;

struct GramArgs {
    const uint8_t *x;            // [N][F]
    int64_t *gram;               // [N][N]
    int64_t *rowsum;             // [N]
    int64_t N, F, per, nslices;  // steps of a K-slice, slices
    int32_t vec16;
};

__global__ void __launch_bounds__(kRowsumThreads) pca_rowsum_k(GramArgs a) {
    __shared__ uint64_t part[kRowsumThreads];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x, F = a.F;
    const uint8_t *src = a.x + row * F;
    uint64_t sum = 0;
    if (a.vec16) {
        for (int64_t p = tid; p < F / kGramPiece; p += kRowsumThreads) {
            const u4 v = *reinterpret_cast<const u4 *>(src + p * kGramPiece);
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const uint32_t t = (v[w] & 0x00ff00ffu) + ((v[w] >> 8) & 0x00ff00ffu);
                s += (t & 0xffffu) + (t >> 16);
            }
            sum += s;
        }
    } else {
        for (int64_t f = tid; f < F; f += kRowsumThreads) sum += src[f];
    }
    part[tid] = sum;
    __syncthreads();
    for (int w = kRowsumThreads / 2; w > 0; w /= 2) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) a.rowsum[row] = (int64_t)part[0];
}

// the plane's zeroes for a launch of several slices: a kernel, not hipMemsetAsync — a memset node captured into a HIP graph filled the
// plane with a stale pattern when the graph was replayed (profiles/NOTES.md AZ), and the call must be replayable
__global__ void __launch_bounds__(kRowsumThreads) pca_gram_zero_k(int64_t *gram, int64_t count) {
    for (int64_t k = (int64_t)blockIdx.x * kRowsumThreads + threadIdx.x; k < count; k += (int64_t)gridDim.x * kRowsumThreads) gram[k] = 0;
}

// lane half h's operand of step `step` for frame `row`: signed bytes, a signed 0 wherever gram_load_range gives no byte
__device__ __forceinline__ i32x4 gram_operand(const GramArgs &a, int64_t row, int64_t step, int64_t step_end, int h) {
    int64_t begin;
    int count;
    gram_load_range(a.N, a.F, row, step, step_end, h, &begin, &count);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (a.vec16) {
        if (count == kGramPiece) {
            const u4 v = *reinterpret_cast<const u4 *>(a.x + begin);
            w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
        }
    } else {
#pragma unroll
        for (int q = 0; q < kGramPiece; q++)
            if (q < count) w[q / 4] |= (uint32_t)a.x[begin + q] << (8 * (q % 4));
    }
    return i32x4{(int)gram_signed_word(w[0], count), (int)gram_signed_word(w[1], count - 4), (int)gram_signed_word(w[2], count - 8),
                 (int)gram_signed_word(w[3], count - 12)};
}

__global__ void __launch_bounds__(64) pca_gram_k(GramArgs a) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int64_t t = blockIdx.x / a.nslices, s = blockIdx.x % a.nslices;
    int ti, tj;
    gram_tile_of(t, gram_tiles_side(a.N), &ti, &tj);
    const bool diag = ti == tj;
    const int64_t row_a = (int64_t)ti * kGramTile + r, row_b = (int64_t)tj * kGramTile + r;
    int64_t step0, step1;
    gram_slice_range(a.F, a.per, s, &step0, &step1);

    int64_t acc64[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc64[k] = 0;
    for (int64_t c0 = step0; c0 < step1; c0 += kGramChunkSteps) {
        const int64_t c1 = c0 + kGramChunkSteps < step1 ? c0 + kGramChunkSteps : step1;
        i32x16 acc;
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] = 0;
        for (int64_t step = c0; step < c1; step += kGramUnroll) {
            i32x4 A[kGramUnroll], B[kGramUnroll];
#pragma unroll
            for (int u = 0; u < kGramUnroll; u++) {
                A[u] = gram_operand(a, row_a, step + u, c1, h);
                B[u] = diag ? A[u] : gram_operand(a, row_b, step + u, c1, h);
            }
#pragma unroll
            for (int u = 0; u < kGramUnroll; u++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[u], B[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) acc64[k] += acc[k];
    }

    // accumulator register k of lane l: tile row (k & 3) + 8 (k >> 2) + 4 (l >> 5) (the A side), tile column l & 31 (the B side)
    const int64_t fj = (int64_t)tj * kGramTile + r;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int64_t fi = (int64_t)ti * kGramTile + (k & 3) + 8 * (k >> 2) + 4 * h;
        if (fi >= a.N || fj >= a.N) continue;
        const int64_t v = s == 0 ? gram_unshift(acc64[k], a.rowsum[fi], a.rowsum[fj], a.F) : acc64[k];
        if (a.nslices == 1) {
            a.gram[fi * a.N + fj] = v;
            if (!diag) a.gram[fj * a.N + fi] = v;
        } else {
            atomicAdd(reinterpret_cast<unsigned long long *>(a.gram + fi * a.N + fj), (unsigned long long)v);
            if (!diag) atomicAdd(reinterpret_cast<unsigned long long *>(a.gram + fj * a.N + fi), (unsigned long long)v);
        }
    }
}

thread_local std::string g_gram_error;
int gram_fail(int code, const std::string &m) { g_gram_error = m; return code; }

}  // namespace
}  // namespace srl

extern "C" {

int srlhip_pca_gram_supported(int32_t n, int64_t n_features) { return srl::pca_gram_supported(n, n_features) ? 1 : 0; }

int srlhip_pca_gram(int32_t device_id, const uint8_t *frames_dev, int32_t n, int64_t n_features, int32_t split, int64_t *gram_dev,
                    int64_t *rowsum_dev, void *hip_stream) {
    const srl::Verdict v = srl::check_pca_gram(n, n_features, split, frames_dev != nullptr, gram_dev != nullptr, rowsum_dev != nullptr);
    if (v.code) return srl::gram_fail(v.code, std::string("srlhip_pca_gram: ") + v.msg);
    const int64_t per = srl::gram_slice_steps(n_features, split > 0 ? split : srl::gram_auto_split(n, n_features));
    const int64_t nslices = srl::gram_slices(n_features, per), tiles = srl::gram_tiles_upper(n);
    if (tiles * nslices > INT32_MAX) return srl::gram_fail(SRLHIP_ENOTSUP, "srlhip_pca_gram: too many work items for one launch");
    hipError_t rc = hipSetDevice(device_id);
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (rc != hipSuccess) return srl::gram_fail(SRLHIP_EHIP, std::string("srlhip_pca_gram: ") + hipGetErrorString(rc));
    if (nslices > 1) {
        const int64_t count = (int64_t)n * n, blocks = (count + srl::kRowsumThreads - 1) / srl::kRowsumThreads;
        hipLaunchKernelGGL(srl::pca_gram_zero_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(srl::kRowsumThreads), 0, stream, gram_dev, count);
    }
    const srl::GramArgs a{frames_dev, gram_dev, rowsum_dev, n, n_features, per, nslices,
                          srl::gram_vec16(n_features, reinterpret_cast<uintptr_t>(frames_dev)) ? 1 : 0};
    hipLaunchKernelGGL(srl::pca_rowsum_k, dim3((unsigned)n), dim3(srl::kRowsumThreads), 0, stream, a);
    hipLaunchKernelGGL(srl::pca_gram_k, dim3((unsigned)(tiles * nslices)), dim3(64), 0, stream, a);
    rc = hipGetLastError();
    if (rc != hipSuccess) return srl::gram_fail(SRLHIP_EHIP, std::string("srlhip_pca_gram: ") + hipGetErrorString(rc));
    return SRLHIP_OK;
}

int srlhip_pca_gram_host(const uint8_t *frames, int32_t n, int64_t n_features, int64_t *gram, int64_t *rowsum) {
    const srl::Verdict v = srl::check_pca_gram(n, n_features, 0, frames != nullptr, gram != nullptr, rowsum != nullptr);
    if (v.code) return srl::gram_fail(v.code, std::string("srlhip_pca_gram_host: ") + v.msg);
    srl::pca_gram_host(frames, n, n_features, gram, rowsum);
    return SRLHIP_OK;
}

const char *srlhip_pca_gram_last_error(void) { return srl::g_gram_error.c_str(); }

}  // extern "C"
