// knn.hip — srlhip_knn: the exact k nearest neighbours of Q query rows among N device-resident states, and with a ground truth the
// KNN-MSE term of every query (include/srlhip.h has the contract; knn.hpp the arithmetic, the order, the rules and the index math).  What
// state_representation/evaluate.py scores a learned state space with.
//
//   partial   knn_partial_k<SMAX, KMAX>: ONE LANE per query, the query's S <= SMAX values in registers.  A workgroup is 256 queries and
//             one slice of the candidates; the slice is staged in LDS kKnnTile rows at a time (a tile of rows is one contiguous run of the
//             states' array, widened to float64 and padded to whole groups of four values on the way in) and every lane reads the same candidate value: LDS broadcasts.  The lane keeps
//             a sorted list of KMAX >= k slots, every slot a register, and touches it only when a candidate comes before its last slot.
//   slices    4096 queries are 64 wavefronts on 1024 SIMDs, so the candidates are cut into slices over blockIdx.y (knn_auto_split, or the
//             caller's split); a slice's lists go to the workspace as [slice][n][q].  With ONE slice the kernel writes idx / dist / err itself.
//   merge     knn_merge_k<KMAX>: one lane per query offers the slices' lists to a list of its own under the same order, writes idx / dist
//             and, with a ground truth, err.
// Nothing is zeroed or preset on the stream: every list starts in registers.  Every global access is guarded: a candidate row by its index,
// a query lane by q < Q, and a query index outside 0 .. N - 1 is clamped for the load and gives (-1, +inf) rows (it offers nothing).
#include <string>

#include "internal.hpp"
#include "knn.hpp"

namespace srl {
namespace {

struct KnnArgs {
    const void *x;              // [N][S] float64 or float32
    const int32_t *queries;     // [Q] or null
    const double *gt;           // [N][G] or null
    int32_t *idx;               // [Q][k]
    double *dist;               // [Q][k]
    double *err;                // [Q] or null
    double *pdist;              // workspace: [slices][k][Q]
    int32_t *pidx;              //            [slices][k][Q]
    int64_t N, Q, per, nslices; // candidates of a slice, slices
    int32_t S, k, G, f32;
};

__device__ __forceinline__ double knn_load(const KnnArgs &a, int64_t at) {
    return a.f32 ? (double)static_cast<const float *>(a.x)[at] : static_cast<const double *>(a.x)[at];
}

// the finished list of query q (row i of the states): idx, dist and err
template <int KMAX> __device__ __forceinline__ void knn_finish(const KnnArgs &a, const KnnList<KMAX> &l, int64_t q, int64_t i) {
#pragma unroll
    for (int n = 0; n < KMAX; n++)
        if (n < a.k) {
            a.idx[q * a.k + n] = l.j[n]; a.dist[q * a.k + n] = l.d[n];
            __builtin_amdgcn_sched_barrier(0);               // one slot's addresses at a time: the list fills the registers
        }
    if (a.gt) a.err[q] = knn_error(l, a.k, a.gt, a.G, i);
}

// the query of a lane: -> is it a real one (q < Q, index inside the states); *i is always a row that may be loaded
__device__ __forceinline__ bool knn_query_of(const KnnArgs &a, int64_t q, int64_t *i) {
    int64_t v = 0;
    bool real = q < a.Q;
    if (real) {
        v = a.queries ? (int64_t)a.queries[q] : q;
        if (v < 0 || v >= a.N) { real = false; v = 0; }
    }
    *i = v;
    return real;
}

template <int SMAX, int KMAX> __global__ void __launch_bounds__(kKnnBlock) knn_partial_k(KnnArgs a) {
    __shared__ double tile[kKnnTile * SMAX];
    const int tid = threadIdx.x, S = a.S;
    const int64_t q = (int64_t)blockIdx.x * kKnnBlock + tid, slice = blockIdx.y;
    int64_t i;
    const bool real = knn_query_of(a, q, &i);
    const int32_t self = real ? (int32_t)i : -1;

    double x[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; s++) x[s] = s < S ? knn_load(a, i * S + s) : 0.0;
    KnnList<KMAX> l;
    l.clear();

    // a tile row is SP = S rounded up to kKnnStep values, the padding +0.0 like the padding of x: a padded step is d = fma(0, 0, d) = d
    // for every d the chain can hold (+0, positive, +inf, NaN), so whole groups of kKnnStep steps run unguarded and no bit moves
    const int SP = (S + kKnnStep - 1) / kKnnStep * kKnnStep;
    const int64_t c0 = slice * a.per, c1 = c0 + a.per < a.N ? c0 + a.per : a.N;
    for (int64_t base = c0; base < c1; base += kKnnTile) {
        const int rows = (int)(c1 - base < kKnnTile ? c1 - base : kKnnTile), count = rows * SP;
        __syncthreads();                                     // the previous tile has been read
        for (int e = tid; e < count; e += kKnnBlock) {
            const int t = e / SP, s = e - t * SP;
            tile[e] = s < S ? knn_load(a, (base + t) * S + s) : 0.0;
        }
        __syncthreads();
        for (int t = 0; t < rows; t++) {                     // (a lane without a real query computes along and offers nothing)
            const double *c = tile + t * SP;
            double d = 0.0;
#pragma unroll
            for (int s0 = 0; s0 < SMAX; s0 += kKnnStep) {
                if (s0 < S) {
#pragma unroll
                    for (int u = 0; u < kKnnStep; u++) d = knn_distance_step(x[s0 + u], c[s0 + u], d);
                }
            }
            const int32_t j = (int32_t)(base + t);
            if (real && j != self && l.admits(d, j)) l.insert(d, j);
        }
    }

    if (q >= a.Q) return;
    if (a.nslices == 1) {
        knn_finish(a, l, q, i);
    } else {
#pragma unroll
        for (int n = 0; n < KMAX; n++)
            if (n < a.k) {
                const int64_t at = knn_partial_at(slice, n, q, a.k, a.Q);
                a.pdist[at] = l.d[n]; a.pidx[at] = l.j[n];
                __builtin_amdgcn_sched_barrier(0);           // (as in knn_finish)
            }
    }
}

template <int KMAX> __global__ void __launch_bounds__(kKnnBlock) knn_merge_k(KnnArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
    if (q >= a.Q) return;
    int64_t i;
    knn_query_of(a, q, &i);
    KnnList<KMAX> l;
    l.clear();
    for (int64_t slice = 0; slice < a.nslices; slice++)
        for (int n = 0; n < a.k; n++) {
            const int64_t at = knn_partial_at(slice, n, q, a.k, a.Q);
            const int32_t j = a.pidx[at];
            if (j >= 0) l.offer(a.pdist[at], j);
        }
    knn_finish(a, l, q, i);
}

template <int SMAX, int KMAX> void knn_launch(const KnnArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)knn_query_blocks(a.Q), (unsigned)a.nslices);
    hipLaunchKernelGGL((knn_partial_k<SMAX, KMAX>), grid, dim3(kKnnBlock), 0, stream, a);
    if (a.nslices > 1) hipLaunchKernelGGL((knn_merge_k<KMAX>), dim3((unsigned)knn_query_blocks(a.Q)), dim3(kKnnBlock), 0, stream, a);
}
template <int SMAX> void knn_launch_k(const KnnArgs &a, hipStream_t stream) {
    if (a.k <= 8) knn_launch<SMAX, 8>(a, stream);
    else knn_launch<SMAX, 32>(a, stream);
}

thread_local std::string g_knn_error;
int knn_fail(int code, const std::string &m) { g_knn_error = m; return code; }

}  // namespace
}  // namespace srl

extern "C" {

int srlhip_knn_supported(int32_t n, int32_t s, int32_t k, int32_t q, int32_t g) { return srl::knn_supported(n, s, k, q, g) ? 1 : 0; }

size_t srlhip_knn_workspace_bytes(int32_t n, int32_t s, int32_t k, int32_t q, int32_t split) { return srl::knn_workspace_bytes(n, s, k, q, split); }

int srlhip_knn(int32_t device_id, const void *states_dev, int32_t states_f32, int32_t n, int32_t s, const int32_t *queries_dev, int32_t q,
               int32_t k, const double *gt_dev, int32_t g, int32_t split, int32_t *idx_dev, double *dist_dev, double *err_dev,
               void *workspace_dev, void *hip_stream) {
    if (!queries_dev) q = n;
    const srl::Verdict v = srl::check_knn(n, s, k, q, g, split, states_dev != nullptr, idx_dev != nullptr, dist_dev != nullptr,
                                          gt_dev != nullptr, err_dev != nullptr);
    if (v.code) return srl::knn_fail(v.code, std::string("srlhip_knn: ") + v.msg);
    if (!workspace_dev) return srl::knn_fail(SRLHIP_EINVAL, "srlhip_knn: knn: null workspace (srlhip_knn_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 8) return srl::knn_fail(SRLHIP_EINVAL, "srlhip_knn: knn: the workspace must be 8-byte aligned");
    const int64_t per = srl::knn_slice_len_for(n, q, split), nslices = srl::knn_slices(n, per);
    if (nslices > 65535) return srl::knn_fail(SRLHIP_ENOTSUP, "srlhip_knn: knn: more than 65535 candidate slices");
    hipError_t rc = hipSetDevice(device_id);
    if (rc != hipSuccess) return srl::knn_fail(SRLHIP_EHIP, std::string("srlhip_knn: ") + hipGetErrorString(rc));
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    double *pdist = static_cast<double *>(workspace_dev);
    const srl::KnnArgs a{states_dev, queries_dev, gt_dev, idx_dev, dist_dev, err_dev, pdist, reinterpret_cast<int32_t *>(pdist + nslices * k * q),
                         n, q, per, nslices, s, k, g, states_f32 ? 1 : 0};
    if (s <= 8) srl::knn_launch_k<8>(a, stream);
    else if (s <= 16) srl::knn_launch_k<16>(a, stream);
    else if (s <= 32) srl::knn_launch_k<32>(a, stream);
    else srl::knn_launch_k<64>(a, stream);
    rc = hipGetLastError();
    if (rc != hipSuccess) return srl::knn_fail(SRLHIP_EHIP, std::string("srlhip_knn: ") + hipGetErrorString(rc));
    return SRLHIP_OK;
}

int srlhip_knn_host(const void *states, int32_t states_f32, int32_t n, int32_t s, const int32_t *queries, int32_t q, int32_t k,
                    const double *gt, int32_t g, int32_t *idx, double *dist, double *err) {
    if (!queries) q = n;
    const srl::Verdict v = srl::check_knn(n, s, k, q, g, 0, states != nullptr, idx != nullptr, dist != nullptr, gt != nullptr, err != nullptr);
    if (v.code) return srl::knn_fail(v.code, std::string("srlhip_knn_host: ") + v.msg);
    if (!srl::knn_host(states, states_f32, n, s, queries, q, k, gt, g, idx, dist, err))
        return srl::knn_fail(SRLHIP_EINVAL, "srlhip_knn_host: knn: a query index is outside 0..n-1");
    return SRLHIP_OK;
}

const char *srlhip_knn_last_error(void) { return srl::g_knn_error.c_str(); }

}  // extern "C"
