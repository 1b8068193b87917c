// pca_project.hip — srlhip_pca_*: the PCA state baseline (state_representation/models.py:196-217, pca.transform of one flattened frame at
// a time on the host) for a whole device-resident batch of uint8 frames as ONE launch (include/srlhip.h has the contract,
// pca_project.hpp the arithmetic, the summation order and the rules).
//
// uint8 [n][F] . float64 [F][S] with W shared by every frame: a GEMM on the float64 VECTOR pipe (v_fma_f64 is a host fma() bit for bit;
// the order in which the matrix instruction sums its four products is not measured here).  A work item is a (frame tile, chunk) pair:
// frame tiles alone would leave most CUs idle at the batch sizes the envs run at.
//   tile      kPcaThreads lanes as (SP / CL column groups) x (frame groups); a lane keeps kPcaFR x CL independent accumulators — its
//             frames fg + j * FG, its columns cg * CL + k — which is what covers the latency of each sequential fma chain.
//   staging   kPcaKT features at a time: the W rows as [kPcaKT][SP] doubles in LDS (S padded with +0.0, rows at or past F zero), shared
//             by the whole tile; the frames' bytes as [frames][kPcaKT] (16-byte loads where F and the base allow them, guarded bytes
//             elsewhere; rows at or past n and features at or past F zero).  A lane reads 16 bytes per frame and converts each byte once
//             for its CL columns — so a frame's byte is converted by each of the SP / CL column groups (2, 4 or 8), not once per
//             tile: 2 VALU operations next to CL fmas (profiles/NOTES.md AU counts it among what is left).
//   join      a chunk's sums go to a partial buffer [chunk][n][SP]; the workgroup that arrives last at its tile's ticket (agent-scope
//             release / acquire around it, pixel_policy.hip's mechanism) adds them in chunk order, adds b and stores.  The ticket
//             words are zero between launches (the last arriver puts the zero back): replayable from a graph.  ONE join: a frame of
//             one chunk (F <= kPcaChunk) has nothing to join, every other launch takes this path whatever n is.
//   scratch   partial buffer and tickets belong to the STREAM the forward is enqueued on (the handle keeps one pair per stream, grow-
//             only): launches on one stream are ordered and may share them, launches on two streams may overlap and must not.  A
//             batch whose chunk sums would pass kPcaScratchBytes goes as several launches over slabs of whole frame tiles, one
//             behind the other on the stream, through the same scratch — which bounds the scratch and the grid.
// Every global access is guarded; every offset is 64-bit (n F passes 2^31 at 224 x 224 x 3).
#include <new>
#include <string>
#include <vector>

#include "internal.hpp"
#include "pca_project.hpp"

namespace srl {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int kPcaRow = kPcaKT + 16;              // LDS stride of a frame's staged bytes: 80 B, so that 16 lanes' 16-byte reads hit 16 slots

struct PcaArgs {
    const uint8_t *images;       // [n][F]
    const double *w;             // [F][S]
    const double *b;             // [S]
    void *states;                // [n][S] float64 / float32
    double *part;                // chunks > 1: [chunks][n][SP] chunk sums
    uint32_t *ticket;            // chunks > 1: [tiles], zero between launches
    int64_t F, n;
    int32_t S, chunks, states_f32, vec16;
};

template <int SP>
__global__ void __launch_bounds__(kPcaThreads) pca_project_k(PcaArgs a) {
    constexpr int CL = pca_lane_cols(SP), CG = SP / CL, FG = kPcaThreads / CG, FR = kPcaFR, FT = pca_tile_frames(SP);
    static_assert(FT == FR * FG && kPcaKT % 16 == 0 && CL % 2 == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) double ws[kPcaKT * SP];
    __shared__ __attribute__((aligned(16))) uint8_t xs[FT * kPcaRow];
    __shared__ uint32_t last;
    const int tid = threadIdx.x, fg = tid % FG, cg = tid / FG;
    const int chunks = a.chunks;
    const int64_t tile = blockIdx.x / chunks, frame0 = tile * FT;
    const int c = (int)(blockIdx.x % chunks);
    const int64_t F = a.F, n = a.n;
    const int S = a.S;

    double acc[FR][CL];
#pragma unroll
    for (int j = 0; j < FR; j++)
#pragma unroll
        for (int k = 0; k < CL; k++) acc[j][k] = 0.0;
    const int64_t cf0 = (int64_t)c * kPcaChunk;
    for (int kt = 0; kt < kPcaChunk / kPcaKT; kt++) {
        const int64_t f0 = cf0 + (int64_t)kt * kPcaKT;
        if (f0 >= F) break;                                // (the same for the whole workgroup)
        __syncthreads();                                   // the previous stage has been read
        for (int idx = tid; idx < kPcaKT * SP; idx += kPcaThreads) {
            const int64_t f = f0 + idx / SP;
            const int s = idx % SP;
            ws[idx] = (f < F && s < S) ? a.w[f * S + s] : 0.0;
        }
        for (int idx = tid; idx < FT * (kPcaKT / 16); idx += kPcaThreads) {
            const int fl = idx / (kPcaKT / 16), piece = idx % (kPcaKT / 16);
            const int64_t frame = frame0 + fl, f = f0 + piece * 16;
            u4 v = {0u, 0u, 0u, 0u};
            if (frame < n && f < F) {
                const uint8_t *src = a.images + frame * F + f;
                if (a.vec16 && f + 16 <= F) v = *reinterpret_cast<const u4 *>(src);
                else {
                    uint32_t wd[4] = {0u, 0u, 0u, 0u};
                    for (int q = 0; q < 16; q++)
                        if (f + q < F) wd[q / 4] |= (uint32_t)src[q] << (8 * (q % 4));
                    v = u4{wd[0], wd[1], wd[2], wd[3]};
                }
            }
            *reinterpret_cast<u4 *>(xs + fl * kPcaRow + piece * 16) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int kk = 0; kk < kPcaKT / 16; kk++) {
            u4 xb[FR];
#pragma unroll
            for (int j = 0; j < FR; j++) xb[j] = *reinterpret_cast<const u4 *>(xs + (fg + j * FG) * kPcaRow + kk * 16);
#pragma unroll
            for (int q = 0; q < 16; q++) {
                double wv[CL];
                const double *wr = ws + (kk * 16 + q) * SP + cg * CL;
#pragma unroll
                for (int k = 0; k < CL; k += 2) {
                    const d2 t = *reinterpret_cast<const d2 *>(wr + k);
                    wv[k] = t.x; wv[k + 1] = t.y;
                }
#pragma unroll
                for (int j = 0; j < FR; j++) {
                    const uint8_t x = (uint8_t)(xb[j][q / 4] >> (8 * (q % 4)));
#pragma unroll
                    for (int k = 0; k < CL; k++) acc[j][k] = pca_step(acc[j][k], x, wv[k]);
                }
            }
        }
    }

    // a one-chunk frame's sum is its state; otherwise acc becomes the state in the join below, in the tile's last arriver only
    if (chunks > 1) {
        // publish this chunk's sums
#pragma unroll
        for (int j = 0; j < FR; j++) {
            const int64_t frame = frame0 + fg + j * FG;
            if (frame < n) {
                double *dst = a.part + ((int64_t)c * n + frame) * SP + cg * CL;
#pragma unroll
                for (int k = 0; k < CL; k += 2) *reinterpret_cast<d2 *>(dst + k) = d2{acc[j][k], acc[j][k + 1]};
            }
        }
        // the last arriver of the tile adds all the chunks' sums in chunk order
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t t = __hip_atomic_fetch_add(a.ticket + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = t == (uint32_t)chunks - 1 ? 1u : 0u;
            if (t == (uint32_t)chunks - 1) {
                __hip_atomic_store(a.ticket + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch on the stream
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (last == 0u) return;
        // (chunk by chunk for all of the lane's frames at once: FR x CL loads in flight per step of the chain, not CL)
        for (int cc = 0; cc < chunks; cc++) {
#pragma unroll
            for (int j = 0; j < FR; j++) {
                const int64_t frame = frame0 + fg + j * FG;
                if (frame >= n) continue;
                const double *src = a.part + ((int64_t)cc * n + frame) * SP + cg * CL;
#pragma unroll
                for (int k = 0; k < CL; k++)
                    acc[j][k] = pca_chunk_join(cc == 0, acc[j][k], __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < FR; j++) {
        const int64_t frame = frame0 + fg + j * FG;
        if (frame >= n) continue;
#pragma unroll
        for (int k = 0; k < CL; k++) {
            const int s = cg * CL + k;
            if (s < S) pca_store(a.states, frame * S + s, a.states_f32 != 0, pca_finish(acc[j][k], a.b[s]));
        }
    }
}

}  // namespace
}  // namespace srl

// the scratch of the launches on one stream
struct PcaScratch {
    hipStream_t stream = nullptr;
    double *d_part = nullptr;        // grow-only: [chunks][frames of a slab][SP]
    uint32_t *d_ticket = nullptr;    // grow-only: [tiles of a slab], zero between launches
    int64_t part_doubles = 0, ticket_words = 0;
};

struct srlhip_pca {
    int device_id = 0;
    int64_t F = 0;
    int32_t S = 0, SP = 0;
    double *d_w = nullptr, *d_b = nullptr;
    std::vector<PcaScratch> scratch;     // one per stream a forward has been enqueued on
    std::string err;
    int fail(int code, const std::string &m) { err = m; return code; }
};

namespace {
thread_local std::string g_pca_create_error;

#define PCA_HIP(errstr, call)                                                                  \
    do {                                                                                       \
        const hipError_t rc_ = (call);                                                         \
        if (rc_ != hipSuccess) { (errstr) = std::string(#call ": ") + hipGetErrorString(rc_); return SRLHIP_EHIP; } \
    } while (0)

// the stream's grow-only scratch; growing waits for the device (a caller that captures a forward calls it once, on the stream it
// captures, with its batch size first)
int pca_scratch(srlhip_pca *p, hipStream_t stream, int64_t part_doubles, int64_t tiles, PcaScratch **out) {
    PcaScratch *sc = nullptr;
    for (PcaScratch &have : p->scratch)
        if (have.stream == stream) sc = &have;
    if (!sc) {
        try { p->scratch.emplace_back(); } catch (const std::bad_alloc &) { return p->fail(SRLHIP_ENOMEM, "srlhip_pca_forward: out of host memory"); }
        sc = &p->scratch.back();
        sc->stream = stream;
    }
    if (part_doubles > sc->part_doubles) {
        if (sc->d_part) { PCA_HIP(p->err, hipFree(sc->d_part)); sc->d_part = nullptr; sc->part_doubles = 0; }
        PCA_HIP(p->err, hipMalloc(reinterpret_cast<void **>(&sc->d_part), (size_t)part_doubles * sizeof(double)));
        sc->part_doubles = part_doubles;
    }
    if (tiles > sc->ticket_words) {
        if (sc->d_ticket) { PCA_HIP(p->err, hipFree(sc->d_ticket)); sc->d_ticket = nullptr; sc->ticket_words = 0; }
        PCA_HIP(p->err, hipMalloc(reinterpret_cast<void **>(&sc->d_ticket), (size_t)tiles * sizeof(uint32_t)));
        PCA_HIP(p->err, hipMemset(sc->d_ticket, 0, (size_t)tiles * sizeof(uint32_t)));
        sc->ticket_words = tiles;
    }
    *out = sc;
    return SRLHIP_OK;
}
}  // namespace

extern "C" {

int srlhip_pca_supported(int64_t n_features, int32_t state_dim) { return srl::check_pca_shape(n_features, state_dim).code == 0 ? 1 : 0; }

int srlhip_pca_create(int32_t device_id, int64_t n_features, int32_t state_dim, const double *w, const double *b, srlhip_pca_handle *out) {
    if (!out) return SRLHIP_EINVAL;
    *out = nullptr;
    const srl::Verdict v = srl::check_pca_shape(n_features, state_dim);
    if (v.code) { g_pca_create_error = std::string("srlhip_pca_create: ") + v.msg; return v.code; }
    if (!w || !b) { g_pca_create_error = "srlhip_pca_create: null weights"; return SRLHIP_EINVAL; }
    srlhip_pca *p = new (std::nothrow) srlhip_pca();
    if (!p) return SRLHIP_ENOMEM;
    p->device_id = device_id; p->F = n_features; p->S = state_dim; p->SP = srl::pca_padded_dim(state_dim);
    const size_t wb = (size_t)n_features * state_dim * sizeof(double), bb = (size_t)state_dim * sizeof(double);
    const auto build = [&]() -> int {
        PCA_HIP(g_pca_create_error, hipSetDevice(device_id));
        PCA_HIP(g_pca_create_error, hipMalloc(reinterpret_cast<void **>(&p->d_w), wb));
        PCA_HIP(g_pca_create_error, hipMalloc(reinterpret_cast<void **>(&p->d_b), bb));
        PCA_HIP(g_pca_create_error, hipMemcpy(p->d_w, w, wb, hipMemcpyHostToDevice));
        PCA_HIP(g_pca_create_error, hipMemcpy(p->d_b, b, bb, hipMemcpyHostToDevice));
        return SRLHIP_OK;
    };
    const int rc = build();
    if (rc != SRLHIP_OK) { srlhip_pca_destroy(p); return rc; }      // whatever had been built so far
    *out = p;
    return SRLHIP_OK;
}

int srlhip_pca_forward(srlhip_pca_handle p, const uint8_t *images_dev, int32_t n, void *states_dev, int32_t states_f32, void *hip_stream) {
    if (!p) return SRLHIP_EINVAL;
    const srl::Verdict v = srl::check_pca_forward(n, images_dev != nullptr, states_dev != nullptr, states_f32);
    if (v.code) return p->fail(v.code, std::string("srlhip_pca_forward: ") + v.msg);
    if (n == 0) return SRLHIP_OK;
    PCA_HIP(p->err, hipSetDevice(p->device_id));
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int64_t chunks = srl::pca_chunks(p->F), tiles = srl::pca_tiles(n, p->SP), ft = srl::pca_tile_frames(p->SP);
    const int64_t slab_tiles = srl::pca_slab_tiles(tiles, chunks, p->SP);
    if (chunks > INT32_MAX || slab_tiles * chunks > INT32_MAX) return p->fail(SRLHIP_ENOTSUP, "srlhip_pca_forward: too many work items for one launch");
    PcaScratch none, *sc = &none;
    if (chunks > 1) {
        const int64_t slab_frames = slab_tiles * ft < n ? slab_tiles * ft : n;
        const int rc = pca_scratch(p, stream, chunks * slab_frames * p->SP, slab_tiles, &sc);
        if (rc != SRLHIP_OK) return rc;
    }
    const int vec16 = p->F % 16 == 0 && reinterpret_cast<uintptr_t>(images_dev) % 16 == 0 ? 1 : 0;      // (a slab starts at a multiple of 16 bytes then)
    const int64_t state_bytes = states_f32 ? 4 : 8;
    for (int64_t t0 = 0; t0 < tiles; t0 += slab_tiles) {
        const int64_t first = t0 * ft, count = n - first < slab_tiles * ft ? n - first : slab_tiles * ft;
        const int64_t grid = ((count + ft - 1) / ft) * chunks;
        srl::PcaArgs a{images_dev + first * p->F, p->d_w, p->d_b, static_cast<char *>(states_dev) + first * p->S * state_bytes,
                       sc->d_part, sc->d_ticket, p->F, count, p->S, (int32_t)chunks, states_f32, vec16};
        const bool launched = srl::dispatch_int<8, 16, 32, 64>(p->SP, [&](auto sp) {
            // (the unused dynamic LDS only holds the residency at two workgroups per compute unit: kPcaLdsPerGroup)
            constexpr int SP = decltype(sp)::value;
            constexpr int used = srl::kPcaKT * SP * (int)sizeof(double) + srl::pca_tile_frames(SP) * srl::kPcaRow + 16;
            constexpr int reserve = SP >= 16 && used < srl::kPcaLdsPerGroup ? srl::kPcaLdsPerGroup - used : 0;
            hipLaunchKernelGGL((srl::pca_project_k<SP>), dim3((unsigned)grid), dim3(srl::kPcaThreads), reserve, stream, a);
        });
        if (!launched) return p->fail(SRLHIP_ENOTSUP, "srlhip_pca_forward: no kernel for this state_dim");
        PCA_HIP(p->err, hipGetLastError());
    }
    return SRLHIP_OK;
}

int srlhip_pca_project_host(int64_t n_features, int32_t state_dim, const double *w, const double *b, const uint8_t *images, int32_t n,
                            void *states, int32_t states_f32) {
    const srl::Verdict shape = srl::check_pca_shape(n_features, state_dim);
    if (shape.code) return shape.code;
    const srl::Verdict v = srl::check_pca_forward(n, images != nullptr, states != nullptr, states_f32);
    if (v.code) return v.code;
    if (n > 0 && (!w || !b)) return SRLHIP_EINVAL;
    srl::pca_project_host(n_features, state_dim, w, b, images, n, states, states_f32 != 0);
    return SRLHIP_OK;
}

int srlhip_pca_destroy(srlhip_pca_handle p) {
    if (!p) return SRLHIP_OK;
    (void)hipSetDevice(p->device_id);
    if (p->d_w) (void)hipFree(p->d_w);
    if (p->d_b) (void)hipFree(p->d_b);
    for (PcaScratch &sc : p->scratch) {
        if (sc.d_part) (void)hipFree(sc.d_part);
        if (sc.d_ticket) (void)hipFree(sc.d_ticket);
    }
    delete p;
    return SRLHIP_OK;
}

const char *srlhip_pca_last_error(srlhip_pca_handle p) { return p ? p->err.c_str() : g_pca_create_error.c_str(); }

}  // extern "C"
