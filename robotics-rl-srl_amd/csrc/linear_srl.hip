// linear_srl.hip — srlhip_linear_srl_*: the trainable linear state encoder on device-resident uint8 frames (include/srlhip.h has the
// contract; linear_srl.hpp the arithmetic, the orders and the rules).  What state_representation/linear_srl.py trains with.
//
//   forward   lin_forward_k<SP>: pca_project.hip's tile — a work item is a (frame tile, chunk of 512 features) pair, kLinThreads lanes as
//             (SP / 8 column groups) x (frame groups), a lane keeps kLinFR x 8 float64 accumulators; V rows, the frames' bytes and the
//             features' (scale, offset) pairs are staged in LDS kLinKT features at a time.  A chunk's sums go to the caller's workspace
//             [chunk][n][SP]; lin_join_k adds them in chunk order, adds c and stores — a second launch behind the first on the stream, no
//             tickets, nothing to zero.  No feature at or past F joins a sum (the loop's bound, the same for the whole workgroup).
//   step      lin_step_k<SG>: ONE launch.  ONE LANE PER FEATURE (byte loads coalesced across f), blockIdx.y a group of SG columns, the
//             lane's SG gradient accumulators in registers; G is staged in LDS kLinStepRows rows at a time and read as a broadcast; the
//             bytes of eight frames are in flight per lane.  No frame at or past n joins a sum.  The finished gradients cross LDS once
//             ([lane][SG + 1]) so that V, m, v and grad_out are read and written with CONSECUTIVE lanes on consecutive doubles: each is
//             touched once.  The frames are read once per column group (1 for S <= 32, 2 above).
// Every global access is guarded; every offset is 64-bit.
#include <string>

#include "internal.hpp"
#include "linear_srl.hpp"

namespace srl {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int kLinRow = kLinKT + 16;              // LDS stride of a frame's staged bytes: 80 B, so that 16 lanes' 16-byte reads hit 16 slots

struct LinFwdArgs {
    const uint8_t *frames;       // [n][F]
    const double *V;             // [F][S]
    double *part;                // [chunks][n][SP] chunk sums
    int64_t F, n;
    int32_t S, chunks, vec16;
    LinNorm t;
};

// a channel's pair out of the by-value tables without a dynamic index (which would put the tables into scratch)
__device__ __forceinline__ void lin_pair(const LinNorm &t, int ch, double *scale, double *offset) {
    double sc = t.scale[0], of = t.offset[0];
#pragma unroll
    for (int k = 1; k < kLinMaxChannels; k++)
        if (ch == k) { sc = t.scale[k]; of = t.offset[k]; }
    *scale = sc; *offset = of;
}

template <int SP>
__global__ void __launch_bounds__(kLinThreads) lin_forward_k(LinFwdArgs a) {
    constexpr int CL = kLinCL, CG = SP / CL, FG = kLinThreads / CG, FR = kLinFR, FT = lin_tile_frames(SP);
    static_assert(FT == FR * FG && kLinKT % 16 == 0 && kLinChunk % kLinKT == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) double ws[kLinKT * SP];
    __shared__ __attribute__((aligned(16))) uint8_t xs[FT * kLinRow];
    __shared__ double nsc[kLinKT], nof[kLinKT];
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
    const int64_t cf0 = (int64_t)c * kLinChunk;
    for (int kt = 0; kt < kLinChunk / kLinKT; kt++) {
        const int64_t f0 = cf0 + (int64_t)kt * kLinKT;
        if (f0 >= F) break;                                // (the same for the whole workgroup)
        const int live = F - f0 < kLinKT ? (int)(F - f0) : kLinKT;      // features of this stage
        __syncthreads();                                   // the previous stage has been read
        for (int idx = tid; idx < kLinKT * SP; idx += kLinThreads) {
            const int64_t f = f0 + idx / SP;
            const int s = idx % SP;
            ws[idx] = (f < F && s < S) ? a.V[f * S + s] : 0.0;
        }
        if (tid < kLinKT) {
            double sc, of;
            lin_pair(a.t, (int)((f0 + tid) % a.t.C), &sc, &of);
            nsc[tid] = sc; nof[tid] = of;
        }
        for (int idx = tid; idx < FT * (kLinKT / 16); idx += kLinThreads) {
            const int fl = idx / (kLinKT / 16), piece = idx % (kLinKT / 16);
            const int64_t frame = frame0 + fl, f = f0 + piece * 16;
            u4 v = {0u, 0u, 0u, 0u};
            if (frame < n && f < F) {
                const uint8_t *src = a.frames + frame * F + f;
                if (a.vec16 && f + 16 <= F) v = *reinterpret_cast<const u4 *>(src);
                else {
                    uint32_t wd[4] = {0u, 0u, 0u, 0u};
                    for (int q = 0; q < 16; q++)
                        if (f + q < F) wd[q / 4] |= (uint32_t)src[q] << (8 * (q % 4));
                    v = u4{wd[0], wd[1], wd[2], wd[3]};
                }
            }
            *reinterpret_cast<u4 *>(xs + fl * kLinRow + piece * 16) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int kk = 0; kk < kLinKT / 16; kk++) {
            if (kk * 16 >= live) break;
            u4 xb[FR];
#pragma unroll
            for (int j = 0; j < FR; j++) xb[j] = *reinterpret_cast<const u4 *>(xs + (fg + j * FG) * kLinRow + kk * 16);
#pragma unroll
            for (int q = 0; q < 16; q++) {
                if (kk * 16 + q < live) {                  // (uniform: no feature at or past F joins a sum)
                    double wv[CL];
                    const double *wr = ws + (kk * 16 + q) * SP + cg * CL;
#pragma unroll
                    for (int k = 0; k < CL; k += 2) {
                        const d2 t = *reinterpret_cast<const d2 *>(wr + k);
                        wv[k] = t.x; wv[k + 1] = t.y;
                    }
                    const double sc = nsc[kk * 16 + q], of = nof[kk * 16 + q];
#pragma unroll
                    for (int j = 0; j < FR; j++) {
                        const double xn = lin_xn(sc, of, (uint8_t)(xb[j][q / 4] >> (8 * (q % 4))));
#pragma unroll
                        for (int k = 0; k < CL; k++) acc[j][k] = lin_step(acc[j][k], xn, wv[k]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < FR; j++) {
        const int64_t frame = frame0 + fg + j * FG;
        if (frame < n) {
            double *dst = a.part + ((int64_t)c * n + frame) * SP + cg * CL;
#pragma unroll
            for (int k = 0; k < CL; k += 2) *reinterpret_cast<d2 *>(dst + k) = d2{acc[j][k], acc[j][k + 1]};
        }
    }
}

// states[i][s] = ((chunk 0 + chunk 1) + ...) + c[s]: one lane per state
__global__ void __launch_bounds__(kLinThreads) lin_join_k(const double *part, const double *c, double *states, int64_t n, int32_t S, int32_t SP, int32_t chunks) {
    const int64_t at = (int64_t)blockIdx.x * kLinThreads + threadIdx.x;
    if (at >= n * S) return;
    const int64_t i = at / S;
    const int s = (int)(at % S);
    double state = 0.0;
    for (int cc = 0; cc < chunks; cc++) state = lin_chunk_join(cc == 0, state, part[((int64_t)cc * n + i) * SP + s]);
    states[at] = lin_finish(state, c[s]);
}

struct LinStepArgs {
    const uint8_t *frames;       // [n][F]
    const double *G;             // [n][S]
    double *V, *m, *v;           // [F][S]
    double *grad;                // [F][S] or null
    int64_t F;
    int32_t n, S;
    LinNorm t;
    LinAdamK k;
};

template <int SG>
__global__ void __launch_bounds__(kLinStepThreads) lin_step_k(LinStepArgs a) {
    constexpr int T = kLinStepThreads, R = kLinStepRows, GL = SG + 1;
    static_assert(R % 8 == 0 && SG % 2 == 0, "stage shape");
    __shared__ __attribute__((aligned(16))) double gs[R * SG];      // a stage of G: [row][column of the group], +0.0 past n or S
    __shared__ double gl[T * GL];                                   // the finished gradients [lane][column], one double of padding
    const int tid = threadIdx.x;
    const int64_t F = a.F, f0 = (int64_t)blockIdx.x * T, f = f0 + tid;
    const int n = a.n, S = a.S, s0 = (int)blockIdx.y * SG;
    const int64_t fl = f < F ? f : F - 1;                           // the feature this lane LOADS: inside the frames for every lane
    double sc, of;
    lin_pair(a.t, (int)(fl % a.t.C), &sc, &of);

    double g[SG];
#pragma unroll
    for (int s = 0; s < SG; s++) g[s] = 0.0;
    for (int i0 = 0; i0 < n; i0 += R) {
        __syncthreads();                                            // the previous stage has been read
        for (int idx = tid; idx < R * SG; idx += T) {
            const int i = i0 + idx / SG, s = s0 + idx % SG;
            gs[idx] = (i < n && s < S) ? a.G[(int64_t)i * S + s] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int r0 = 0; r0 < R; r0 += 8) {
            if (i0 + r0 >= n) break;                                // (the same for the whole workgroup)
            uint8_t xb[8];
#pragma unroll
            for (int j = 0; j < 8; j++) xb[j] = i0 + r0 + j < n ? a.frames[(int64_t)(i0 + r0 + j) * F + fl] : (uint8_t)0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (i0 + r0 + j < n) {                              // (uniform: no frame at or past n joins a sum)
                    const double xn = lin_xn(sc, of, xb[j]);
                    const double *row = gs + (r0 + j) * SG;
#pragma unroll
                    for (int s = 0; s < SG; s += 2) {
                        const d2 t = *reinterpret_cast<const d2 *>(row + s);
                        g[s] = lin_step(g[s], xn, t.x);
                        g[s + 1] = lin_step(g[s + 1], xn, t.y);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SG; s++) gl[tid * GL + s] = g[s];
    __syncthreads();
    // the group's columns of the workgroup's T features, consecutive lanes on consecutive doubles
    const int cols = S - s0 < SG ? S - s0 : SG;
    const int64_t rows = F - f0 < T ? F - f0 : T;
    for (int idx = tid; idx < (int)rows * cols; idx += T) {
        const int r = idx / cols, s = idx % cols;
        const int64_t at = (f0 + r) * S + s0 + s;
        const double gv = gl[r * GL + s];
        double Vv = a.V[at], mv = a.m[at], vv = a.v[at];
        lin_adam(a.k, gv, &Vv, &mv, &vv);
        a.V[at] = Vv; a.m[at] = mv; a.v[at] = vv;
        if (a.grad) a.grad[at] = gv;
    }
}

thread_local std::string g_lin_error;
int lin_fail(int code, const std::string &m) { g_lin_error = m; return code; }

// what both calls and both twins check first: -> 0, or the refusal (its message is set)
int lin_check_common(const char *who, int32_t n, int64_t F, int32_t S, int32_t C, const double *scale, const double *offset) {
    Verdict v = check_lin_shape(F, S, C);
    if (!v.code) v = check_lin_batch(n);
    if (!v.code) v = check_lin_tables(scale, offset, C);
    return v.code ? lin_fail(v.code, std::string(who) + ": " + v.msg) : 0;
}

}  // namespace
}  // namespace srl

extern "C" {

int srlhip_linear_srl_supported(int64_t n_features, int32_t state_dim, int32_t n_channels) {
    return srl::check_lin_shape(n_features, state_dim, n_channels).code == 0 ? 1 : 0;
}

size_t srlhip_linear_srl_workspace_bytes(int64_t n_features, int32_t state_dim, int32_t n) { return srl::lin_workspace_bytes(n_features, state_dim, n); }

int srlhip_linear_srl_forward(int32_t device_id, const uint8_t *frames_dev, int32_t n, int64_t n_features, int32_t state_dim, int32_t n_channels,
                              const double *scale, const double *offset, const double *v_dev, const double *c_dev, double *states_dev,
                              void *workspace_dev, void *hip_stream) {
    const char *who = "srlhip_linear_srl_forward";
    if (const int rc = srl::lin_check_common(who, n, n_features, state_dim, n_channels, scale, offset)) return rc;
    if (!frames_dev || !v_dev || !c_dev || !states_dev) return srl::lin_fail(SRLHIP_EINVAL, std::string(who) + ": linear_srl: null frames, V, c or states");
    if (!workspace_dev) return srl::lin_fail(SRLHIP_EINVAL, std::string(who) + ": linear_srl: null workspace (srlhip_linear_srl_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 16) return srl::lin_fail(SRLHIP_EINVAL, std::string(who) + ": linear_srl: the workspace must be 16-byte aligned");
    const int SP = srl::lin_padded_dim(state_dim);
    const int64_t chunks = srl::lin_chunks(n_features), tiles = srl::lin_tiles(n, SP);
    if (chunks * tiles > INT32_MAX) return srl::lin_fail(SRLHIP_ENOTSUP, std::string(who) + ": linear_srl: too many work items for one launch");
    hipError_t rc = hipSetDevice(device_id);
    if (rc != hipSuccess) return srl::lin_fail(SRLHIP_EHIP, std::string(who) + ": " + hipGetErrorString(rc));
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int vec16 = n_features % 16 == 0 && reinterpret_cast<uintptr_t>(frames_dev) % 16 == 0 ? 1 : 0;
    const srl::LinFwdArgs a{frames_dev, v_dev, static_cast<double *>(workspace_dev), n_features, n, state_dim, (int32_t)chunks, vec16,
                            srl::lin_norm(scale, offset, n_channels)};
    const dim3 grid((unsigned)(chunks * tiles)), block(srl::kLinThreads);
    if (SP == 8) hipLaunchKernelGGL((srl::lin_forward_k<8>), grid, block, 0, stream, a);
    else if (SP == 16) hipLaunchKernelGGL((srl::lin_forward_k<16>), grid, block, 0, stream, a);
    else if (SP == 32) hipLaunchKernelGGL((srl::lin_forward_k<32>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((srl::lin_forward_k<64>), grid, block, 0, stream, a);
    const int64_t states = (int64_t)n * state_dim;
    hipLaunchKernelGGL(srl::lin_join_k, dim3((unsigned)((states + srl::kLinThreads - 1) / srl::kLinThreads)), block, 0, stream,
                       static_cast<const double *>(workspace_dev), c_dev, states_dev, (int64_t)n, state_dim, (int32_t)SP, (int32_t)chunks);
    rc = hipGetLastError();
    if (rc != hipSuccess) return srl::lin_fail(SRLHIP_EHIP, std::string(who) + ": " + hipGetErrorString(rc));
    return SRLHIP_OK;
}

int srlhip_linear_srl_step(int32_t device_id, const uint8_t *frames_dev, int32_t n, int64_t n_features, int32_t state_dim, int32_t n_channels,
                           const double *scale, const double *offset, const double *g_dev, double *v_dev, double *m_dev, double *v2_dev,
                           double lr, double beta1, double beta2, double eps, double bc1, double bc2, double *grad_out_dev, void *hip_stream) {
    const char *who = "srlhip_linear_srl_step";
    if (const int rc = srl::lin_check_common(who, n, n_features, state_dim, n_channels, scale, offset)) return rc;
    const srl::LinAdam adam{lr, beta1, beta2, eps, bc1, bc2};
    const srl::Verdict v = srl::check_lin_adam(adam);
    if (v.code) return srl::lin_fail(v.code, std::string(who) + ": " + v.msg);
    if (!frames_dev || !g_dev || !v_dev || !m_dev || !v2_dev) return srl::lin_fail(SRLHIP_EINVAL, std::string(who) + ": linear_srl: null frames, G, V, m or v");
    const int64_t blocks = srl::lin_step_blocks(n_features);
    if (blocks > INT32_MAX) return srl::lin_fail(SRLHIP_ENOTSUP, std::string(who) + ": linear_srl: too many work items for one launch");
    hipError_t rc = hipSetDevice(device_id);
    if (rc != hipSuccess) return srl::lin_fail(SRLHIP_EHIP, std::string(who) + ": " + hipGetErrorString(rc));
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const srl::LinStepArgs a{frames_dev, g_dev, v_dev, m_dev, v2_dev, grad_out_dev, n_features, n, state_dim,
                             srl::lin_norm(scale, offset, n_channels), srl::lin_adam_k(adam)};
    const int SG = srl::lin_step_group(state_dim);
    const dim3 grid((unsigned)blocks, (unsigned)srl::lin_step_groups(state_dim)), block(srl::kLinStepThreads);
    if (SG == 8) hipLaunchKernelGGL((srl::lin_step_k<8>), grid, block, 0, stream, a);
    else if (SG == 16) hipLaunchKernelGGL((srl::lin_step_k<16>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((srl::lin_step_k<32>), grid, block, 0, stream, a);
    rc = hipGetLastError();
    if (rc != hipSuccess) return srl::lin_fail(SRLHIP_EHIP, std::string(who) + ": " + hipGetErrorString(rc));
    return SRLHIP_OK;
}

int srlhip_linear_srl_forward_host(const uint8_t *frames, int32_t n, int64_t n_features, int32_t state_dim, int32_t n_channels, const double *scale,
                                   const double *offset, const double *v, const double *c, double *states) {
    const char *who = "srlhip_linear_srl_forward_host";
    if (const int rc = srl::lin_check_common(who, n, n_features, state_dim, n_channels, scale, offset)) return rc;
    if (!frames || !v || !c || !states) return srl::lin_fail(SRLHIP_EINVAL, std::string(who) + ": linear_srl: null frames, V, c or states");
    srl::lin_forward_host(frames, n, n_features, state_dim, srl::lin_norm(scale, offset, n_channels), v, c, states);
    return SRLHIP_OK;
}

int srlhip_linear_srl_step_host(const uint8_t *frames, int32_t n, int64_t n_features, int32_t state_dim, int32_t n_channels, const double *scale,
                                const double *offset, const double *g, double *v, double *m, double *v2, double lr, double beta1, double beta2,
                                double eps, double bc1, double bc2, double *grad_out) {
    const char *who = "srlhip_linear_srl_step_host";
    if (const int rc = srl::lin_check_common(who, n, n_features, state_dim, n_channels, scale, offset)) return rc;
    const srl::LinAdam adam{lr, beta1, beta2, eps, bc1, bc2};
    const srl::Verdict vd = srl::check_lin_adam(adam);
    if (vd.code) return srl::lin_fail(vd.code, std::string(who) + ": " + vd.msg);
    if (!frames || !g || !v || !m || !v2) return srl::lin_fail(SRLHIP_EINVAL, std::string(who) + ": linear_srl: null frames, G, V, m or v");
    srl::lin_step_host(frames, n, n_features, state_dim, srl::lin_norm(scale, offset, n_channels), g, v, m, v2, adam, grad_out);
    return SRLHIP_OK;
}

const char *srlhip_linear_srl_last_error(void) { return srl::g_lin_error.c_str(); }

}  // extern "C"
