// policy_act.hip — srlhip_policy_act: a policy's action for every env from an observation plane that is already on the device, as a
// launch of its own between the encoder and the next step (include/srlhip.h has the contract, policy_act.hpp the arithmetic and the finishing step, act_finish), and
// srlhip_sample_actions: the sampled selection alone, on a score plane (sample_actions_k, at the end).
//
// The launch is a stream of the parameter blocks: at D = 200, H = 100 an MLP block is 82 KB per env.  The contract fixes the ORDER of
// every sum (d ascending per hidden unit; 16 virtual lanes, a fixed tree), so a hidden unit is one sequential float64 chain: the
// parallelism is across units (MLP) or across envs and outputs (linear), never across d.
//   MLP     one workgroup per env (per-env blocks) or per four envs (one shared block: staged once, used four times).  fc_in.weight
//           goes through LDS in tiles of all H rows x 64 columns: every row segment is 256 contiguous bytes, fetched 16 bytes per lane
//           into registers one tile ahead of the arithmetic, written to rows of 65 floats (thread j walks row j: bank (j + d) mod 32,
//           conflict-free).  Thread j keeps unit j's chain in a register across the tiles.  fc_in.bias is one coalesced load, fc_out's
//           weight and bias (contiguous, <= 1032 floats) are fetched ahead and staged in the same LDS.  The second layer runs as
//           16 virtual lanes x A outputs, the partials meet in LDS and act_row_sum16 combines them.
//   linear  32 envs x 8 output slots per workgroup; the [D][A] float64 blocks go through LDS in tiles of 8 rows of d (8 A contiguous
//           doubles per env), thread (env, a) keeps score_a's chain.
// Every parameter is loaded once per workgroup that needs it (per-env blocks: once per call), every load and store is guarded: lanes
// of envs >= n, of units >= H, of columns >= D read nothing and store nothing.
#include "internal.hpp"
#include "policy_act.hpp"

namespace srl {
namespace {

constexpr int kBlock = 256;
constexpr int kTileCols = 64, kTileStride = kTileCols + 1, kTileQuads = kActMaxHidden * kTileCols / 4 / kBlock;      // 8 x 16 bytes per thread and tile
constexpr int kW2Floats = kActMaxOut * kActMaxHidden + kActMaxOut, kW2PerThread = (kW2Floats + kBlock - 1) / kBlock;
constexpr int kLinEnvs = 32, kLinRows = 8, kLinStride = kLinRows * kActMaxOut + 1;

struct ActArgs {
    PolicyArgs pol;
    const float *obs;            // [n][D]
    ActFinish fin;
    const uint32_t *key;         // [2][n] the envs' Philox keys
    uint64_t *act_ctr;           // [n] action-stream block counters
    double *score;               // [n][A] or null: the float64 scores as they stood in front of the selection
    int32_t n, D;
};

struct __attribute__((packed, aligned(4))) F4 { float v[4]; };      // 16 bytes at float alignment: a parameter block starts anywhere

// the last step of both kernels, one thread per env: the draw, then policy_act.hpp's finishing step
__device__ __forceinline__ void finish_env(const ActArgs &a, int e, const double *score) {
    act_finish(a.fin, e, score, a.score, a.fin.sample ? act_draw(a.key, a.n, a.act_ctr, e) : 0.0);
}

// E envs per workgroup: 1 with per-env parameter blocks, 4 with one shared block.  Thread t: unit j = t mod 128 of envs (t / 128) and
// (t / 128) + 2 of the workgroup (E = 1: the upper half of the workgroup only fetches).
template <int E>
__global__ void __launch_bounds__(kBlock) policy_act_mlp_k(ActArgs a) {
    constexpr int EA = (E + 1) / 2;
    __shared__ float tile[kActMaxHidden * kTileStride];
    __shared__ float xs[E][kTileCols];
    __shared__ double hs[E][kActMaxHidden];
    __shared__ double part[E][kActMaxOut][kActLanes];
    __shared__ double sc[E][kActMaxOut];
    const int tid = threadIdx.x, j = tid & (kActMaxHidden - 1), slot = tid >> 7;
    const int e0 = blockIdx.x * E;
    const int H = a.pol.hidden, D = a.D, A = a.fin.A;
    const int64_t P = (int64_t)H * D + H + (int64_t)A * H + A;
    const float *w = static_cast<const float *>(a.pol.w) + (E == 1 && a.pol.per_env ? (int64_t)e0 * P : 0);
    const float *w2 = w + (int64_t)H * D + H;      // fc_out.weight [A][H], then fc_out.bias [A]
    const int n2 = A * H + A;
    const bool normalize = a.pol.normalize != 0;

    F4 pre[kTileQuads];
    float xpre = 0.f;
    const auto fetch = [&](int k) {
        const int d0 = k * kTileCols;
#pragma unroll
        for (int q = 0; q < kTileQuads; q++) {
            const int i = tid + kBlock * q, r = i >> 4, c = d0 + (i & 15) * 4;
            F4 v = {{0.f, 0.f, 0.f, 0.f}};
            if (r < H && c < D) {
                const float *src = w + (int64_t)r * D + c;
                if (c + 3 < D) v = *reinterpret_cast<const F4 *>(src);
                else {
                    v.v[0] = src[0];
                    if (c + 1 < D) v.v[1] = src[1];
                    if (c + 2 < D) v.v[2] = src[2];
                }
            }
            pre[q] = v;
        }
        xpre = 0.f;
        if (tid < E * kTileCols) {
            const int e = e0 + tid / kTileCols, d = d0 + tid % kTileCols;
            if (e < a.n && d < D)
                xpre = act_input(a.obs[(int64_t)e * D + d], normalize, normalize ? a.pol.mean[d] : 0.0, normalize ? a.pol.std[d] : 1.0, a.pol.clip);
        }
    };

    float w2pre[kW2PerThread];
#pragma unroll
    for (int q = 0; q < kW2PerThread; q++) { const int i = tid + kBlock * q; w2pre[q] = i < n2 ? w2[i] : 0.f; }
    double acc[EA];
    {
        const double b1 = j < H ? (double)w[(int64_t)H * D + j] : 0.0;
#pragma unroll
        for (int i = 0; i < EA; i++) acc[i] = b1;
    }
    const int nt = (D + kTileCols - 1) / kTileCols;
    fetch(0);
    for (int k = 0; k < nt; k++) {
        __syncthreads();                               // the previous tile has been read
#pragma unroll
        for (int q = 0; q < kTileQuads; q++) {
            const int i = tid + kBlock * q, r = i >> 4, c = (i & 15) * 4;
#pragma unroll
            for (int m = 0; m < 4; m++) tile[r * kTileStride + c + m] = pre[q].v[m];
        }
        if (tid < E * kTileCols) xs[tid / kTileCols][tid % kTileCols] = xpre;
        __syncthreads();
        if (k + 1 < nt) fetch(k + 1);                  // in flight under the arithmetic below
        const int dn = min(kTileCols, D - k * kTileCols);
        if (j < H && slot < E) {
            const float *row = tile + j * kTileStride;
            for (int d = 0; d < dn; d++) {
                const float wv = row[d];
#pragma unroll
                for (int i = 0; i < EA; i++)
                    if (slot + 2 * i < E) acc[i] = act_hidden_step(acc[i], wv, xs[slot + 2 * i][d]);
            }
        }
    }
    __syncthreads();
    if (j < H && slot < E) {
#pragma unroll
        for (int i = 0; i < EA; i++)
            if (slot + 2 * i < E) hs[slot + 2 * i][j] = act_relu(acc[i]);
    }
#pragma unroll
    for (int q = 0; q < kW2PerThread; q++) { const int i = tid + kBlock * q; if (i < n2) tile[i] = w2pre[q]; }
    __syncthreads();
    for (int i = tid; i < E * A * kActLanes; i += kBlock) {
        const int l = i % kActLanes, o = (i / kActLanes) % A, el = i / (kActLanes * A);
        part[el][o][l] = act_lane_partial(l, H, tile + o * H, tile[A * H + o], hs[el]);
    }
    __syncthreads();
    if (tid < E * A) sc[tid / A][tid % A] = act_row_sum16(part[tid / A][tid % A]);
    __syncthreads();
    if (tid < E && e0 + tid < a.n) finish_env(a, e0 + tid, sc[tid]);
}

// thread t: output slot o = t mod 8 of env t / 8 of the workgroup
__global__ void __launch_bounds__(kBlock) policy_act_linear_k(ActArgs a) {
    __shared__ double tile[kLinEnvs * kLinStride];
    __shared__ float xs[kLinEnvs][kLinRows];
    __shared__ double sc[kLinEnvs][kActMaxOut];
    const int tid = threadIdx.x, o = tid & (kActMaxOut - 1), g = tid >> 3;
    const int e0 = blockIdx.x * kLinEnvs, e = e0 + g;
    const int D = a.D, A = a.fin.A, chunk = kLinRows * A;                 // doubles per env and tile
    const int64_t count = (int64_t)D * A;
    const double *W = static_cast<const double *>(a.pol.w);
    const bool per_env = a.pol.per_env != 0, normalize = a.pol.normalize != 0;
    constexpr int kPer = kLinEnvs * kLinRows * kActMaxOut / kBlock;  // 8 doubles per thread and tile
    double pre[kPer];
    float xpre = 0.f;
    const auto fetch = [&](int k) {
        const int64_t off = (int64_t)k * chunk;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int i = tid + kBlock * q, ge = i / chunk, c = i % chunk;
            double v = 0.0;
            if (ge < (per_env ? kLinEnvs : 1) && e0 + ge < a.n && off + c < count) v = W[(per_env ? (int64_t)(e0 + ge) * count : 0) + off + c];
            pre[q] = v;
        }
        const int ge = tid / kLinRows, d = k * kLinRows + tid % kLinRows;
        xpre = 0.f;
        if (e0 + ge < a.n && d < D)
            xpre = act_input(a.obs[(int64_t)(e0 + ge) * D + d], normalize, normalize ? a.pol.mean[d] : 0.0, normalize ? a.pol.std[d] : 1.0, a.pol.clip);
    };
    double acc = 0.0;
    const int nt = (D + kLinRows - 1) / kLinRows;
    fetch(0);
    for (int k = 0; k < nt; k++) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int i = tid + kBlock * q, ge = i / chunk, c = i % chunk;
            if (ge < kLinEnvs) tile[ge * kLinStride + c] = pre[q];
        }
        xs[tid / kLinRows][tid % kLinRows] = xpre;
        __syncthreads();
        if (k + 1 < nt) fetch(k + 1);
        const int dn = min(kLinRows, D - k * kLinRows);
        if (o < A) {
            const double *blk = tile + (per_env ? g : 0) * kLinStride;
            for (int d = 0; d < dn; d++) acc = act_linear_step(k == 0 && d == 0, acc, xs[g][d], blk[d * A + o]);
        }
    }
    if (o < A) sc[g][o] = acc;
    __syncthreads();
    if (o == 0 && e < a.n) finish_env(a, e, sc[g]);
}

// srlhip_sample_actions: act_finish's draw and selection on a score plane the caller holds, one thread per env — not act_finish itself:
// this call only READS the frozen plane, and does so without a freeze flag.  Everything a thread reads is its
// own env's: the score row, the frozen byte, the key and the counter — the result does not depend on n or on the launch geometry.
struct SampleArgs {
    const double *score;         // [n][A]
    const uint8_t *frozen;       // [n] or null
    int32_t *act;                // [n]
    const uint32_t *key;         // [2][n] the envs' Philox keys
    uint64_t *act_ctr;           // [n] action-stream block counters
    int32_t n, A;
};
__global__ void __launch_bounds__(kBlock) sample_actions_k(SampleArgs a) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.n) return;
    double score[kActMaxOut], w[kActMaxOut];
    for (int k = 0; k < a.A; k++) score[k] = a.score[(int64_t)e * a.A + k];
    const double u = act_draw(a.key, a.n, a.act_ctr, e);      // frozen or not
    act_softmax_weights(score, a.A, w);
    const int choice = act_softmax_pick(w, a.A, u);
    a.act[e] = a.frozen && a.frozen[e] ? -1 : choice;
}

}  // namespace

ActFinish act_finish_args(Handle *h, bool freeze, bool sample, int A, bool none_nan, const uint8_t *done_prev, uint8_t *frozen, void *act) {
    if (sample) { h->snap_valid = false; h->prefetch_valid = false; }      // the action-stream counters move past what was drawn ahead
    return ActFinish{done_prev, frozen, act, A, freeze ? 1 : 0, h->cfg.is_discrete ? 1 : 0, sample ? 1 : 0, none_nan ? 1 : 0};
}

int sample_actions_launch(Handle *h, int A, const double *score, const uint8_t *frozen, int32_t *act) {
    h->snap_valid = false; h->prefetch_valid = false;      // the action-stream counters move past what was drawn ahead
    const SampleArgs a{score, frozen, act, h->rng.key, h->rng.act_ctr, h->n, A};
    hipLaunchKernelGGL(sample_actions_k, dim3((h->n + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, a);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

int policy_act_launch(Handle *h, const PolicyArgs &pol, bool sample, int D, int A, bool none_nan, const float *obs, const uint8_t *done_prev,
                      uint8_t *frozen, void *act, double *score) {
    const ActArgs a{pol, obs, act_finish_args(h, pol.freeze != 0, sample, A, none_nan, done_prev, frozen, act), h->rng.key, h->rng.act_ctr, score, h->n, D};
    if (!pol.hidden)
        hipLaunchKernelGGL(policy_act_linear_k, dim3((h->n + kLinEnvs - 1) / kLinEnvs), dim3(kBlock), 0, h->stream, a);
    else if (pol.per_env)
        hipLaunchKernelGGL(policy_act_mlp_k<1>, dim3(h->n), dim3(kBlock), 0, h->stream, a);
    else
        hipLaunchKernelGGL(policy_act_mlp_k<4>, dim3((h->n + 3) / 4), dim3(kBlock), 0, h->stream, a);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

}  // namespace srl
