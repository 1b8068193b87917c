// cnn_policy.hip — srlhip_cnn_policy_act: the action of every env's own three-layer CNN from the frame the rasteriser has just written,
// as one launch between two steps (include/srlhip.h has the contract, cnn_policy.hpp the arithmetic, policy_act.hpp the finishing step
// behind the scores: act_finish).
//
// One workgroup of 256 threads per env: N different networks on N frames share nothing but the code.  The frame is streamed once as
// bytes (a 256-entry table in LDS turns a byte into (float)(b / 255.0)); a layer's weights are staged into LDS transposed, so that the
// channels a thread owns are contiguous, and re-staged per layer into the same buffer.  A layer is walked in pool cells
// (cnn_policy.hpp): a thread forms the 2 x 2 conv outputs of a cell for its channels in registers, adds them to its float64 channel
// sums and keeps only the window's extreme — the pool is taken before the normalisation, exactly (monotone in the direction of gamma's
// sign) — so the layer-1 conv plane (401 KB at 224 x 224) never exists: its pooled plane (100 KB) lives in LDS, and layers 2 and 3
// (a tenth of the work) never leave it.  The sums meet in a butterfly of lane exchanges and, for layer 1, across the four wavefronts
// in LDS.  LDS at 224 x 224: 135 KB, one workgroup per CU; at 64 x 64: 32 KB.
// Every global access is guarded: taps outside the frame read nothing, the grid is exactly num_envs workgroups.
#include "internal.hpp"
#include "cnn_policy.hpp"
#include "policy_act.hpp"

namespace srl {
namespace {

constexpr int kWbufFloats = kCnnCh3 * kCnnCh2 * 9;      // the largest conv block (layer 3: 4608; layer 1 at C = 6: 1200)
constexpr int kRedDoubles = 64;                           // per channel and 64-thread part: S, Q

struct CnnArgs {
    const float *params;         // [n][P] or [P]
    const uint8_t *images;       // [n][H][W][C]
    const uint32_t *key;         // [2][n] the envs' Philox keys
    uint64_t *act_ctr;           // [n] action-stream block counters
    float *score;                // [n][A] or null
    CnnShape s;
    CnnParamLayout L;
    int32_t n, per_env;
    ActFinish fin;               // last: read once, by the finishing thread.  The kernel is at its register limit and the order of this block
                                 // moves its allocation: with `fin` in front of `key` it reserved 36 bytes of scratch (profiles/NOTES.md AX)
};

// the workgroup's LDS: float64 first, then the float planes
struct Lds {
    double *red, *mean, *gs;     // [kRedDoubles], [32], [32]
    float *lut, *wbuf, *gam, *bet, *p1, *p2, *p3, *sc;
};
size_t lds_bytes(const CnnShape &s) {
    const size_t floats = 256 + kWbufFloats + 2 * kCnnCh3 + (size_t)kCnnCh1 * s.hp[0] * s.wp[0] + (size_t)kCnnCh2 * s.hp[1] * s.wp[1] + s.F + kActMaxOut;
    return 8 * (size_t)(kRedDoubles + 2 * kCnnCh3) + 4 * floats;
}

// One layer: stage the weights, walk the cells, combine the sums, normalise the pooled plane.  `in`: the layer's input (0 outside).
template <int K, int PAD, int CO, int CG, class In>
__device__ __forceinline__ void cnn_layer(const In &in, int Cin, int hc, int wc, const float *w, const float *gamma, const float *beta, const Lds &l, float *pooled) {
    constexpr int G = CO / CG, TG = kCnnBlock / G, NP = TG > 64 ? TG / 64 : 1;
    static_assert(CO * NP * 2 <= kRedDoubles, "the reduction block holds every channel's parts");
    const int tid = threadIdx.x;
    for (int i = tid; i < CO * Cin * K * K; i += kCnnBlock) l.wbuf[cnn_weight_slot(i, Cin, K * K, CO)] = w[i];
    if (tid < CO) { l.gam[tid] = gamma[tid]; l.bet[tid] = beta[tid]; }
    __syncthreads();

    const int g = tid / TG, u = tid % TG, c0 = g * CG;
    const int hcell = (hc + 1) / 2, wcell = (wc + 1) / 2, hp = hc / 2, wp = wc / 2;
    double S[CG], Q[CG];
#pragma unroll
    for (int k = 0; k < CG; k++) S[k] = Q[k] = 0.0;
    for (int cell = u; cell < hcell * wcell; cell += TG) {
        const int pi = cell / wcell, pj = cell % wcell;
        float acc[CG][4];
        cnn_cell<K, PAD, CG>(in, Cin, CO, c0, l.wbuf, pi, pj, acc);
        cnn_cell_finish<CG>(acc, pi, pj, hc, wc, c0, l.gam, S, Q, pooled);
    }
    // cnn_tree_sum over the group's TG threads: inside a wavefront by lane exchange (every lane takes part; idle threads hold zeros) ...
#pragma unroll
    for (int k = 0; k < CG; k++)
#pragma unroll
        for (int m = 1; m < (TG < 64 ? TG : 64); m *= 2) {
#pragma clang fp contract(off)
            S[k] = S[k] + __shfl_xor(S[k], m);
            Q[k] = Q[k] + __shfl_xor(Q[k], m);
        }
    if (u % 64 == 0) {
#pragma unroll
        for (int k = 0; k < CG; k++) {
            l.red[((c0 + k) * NP + u / 64) * 2] = S[k];
            l.red[((c0 + k) * NP + u / 64) * 2 + 1] = Q[k];
        }
    }
    __syncthreads();
    // ... and across the wavefronts of layer 1 by the channel's own thread
    if (tid < CO) {
        double vs[NP], vq[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) { vs[p] = l.red[(tid * NP + p) * 2]; vq[p] = l.red[(tid * NP + p) * 2 + 1]; }
        cnn_channel_stats(cnn_tree_sum(vs, NP), cnn_tree_sum(vq, NP), hc * wc, l.gam[tid], &l.mean[tid], &l.gs[tid]);
    }
    __syncthreads();
    for (int i = tid; i < CO * hp * wp; i += kCnnBlock) {
        const int c = i / (hp * wp);
        pooled[i] = cnn_normalise(pooled[i], l.mean[c], l.gs[c], l.bet[c]);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kCnnBlock) cnn_policy_act_k(CnnArgs a) {
    extern __shared__ double lds_raw[];
    const CnnShape &s = a.s;
    Lds l;
    l.red = lds_raw; l.mean = l.red + kRedDoubles; l.gs = l.mean + kCnnCh3;
    l.lut = reinterpret_cast<float *>(l.gs + kCnnCh3); l.wbuf = l.lut + 256; l.gam = l.wbuf + kWbufFloats; l.bet = l.gam + kCnnCh3;
    l.p1 = l.bet + kCnnCh3; l.p2 = l.p1 + kCnnCh1 * s.hp[0] * s.wp[0]; l.p3 = l.p2 + kCnnCh2 * s.hp[1] * s.wp[1]; l.sc = l.p3 + s.F;
    const int tid = threadIdx.x, e = blockIdx.x;
    const float *P = a.params + (a.per_env ? (int64_t)e * (int64_t)a.L.total : 0);
    const uint8_t *img = a.images + (int64_t)e * s.H * s.W * s.C;
    l.lut[tid] = cnn_input((uint8_t)tid);                 // (the layer's first barrier orders it)

    const int H = s.H, W = s.W, C = s.C;
    const float *lut = l.lut;
    const auto frame = [=](int ci, int r, int c) { return (r >= 0 && r < H && c >= 0 && c < W) ? lut[img[((int64_t)r * W + c) * C + ci]] : 0.f; };
    cnn_layer<5, 2, kCnnCh1, kCnnCg1>(frame, C, s.hc[0], s.wc[0], P + a.L.w1, P + a.L.g1, P + a.L.b1, l, l.p1);
    const float *p1 = l.p1;
    const int h1 = s.hp[0], w1 = s.wp[0];
    const auto plane1 = [=](int ci, int r, int c) { return (r >= 0 && r < h1 && c >= 0 && c < w1) ? p1[(ci * h1 + r) * w1 + c] : 0.f; };
    cnn_layer<3, 1, kCnnCh2, kCnnCg2>(plane1, kCnnCh1, s.hc[1], s.wc[1], P + a.L.w2, P + a.L.g2, P + a.L.b2, l, l.p2);
    const float *p2 = l.p2;
    const int h2 = s.hp[1], w2 = s.wp[1];
    const auto plane2 = [=](int ci, int r, int c) { return (r >= 0 && r < h2 && c >= 0 && c < w2) ? p2[(ci * h2 + r) * w2 + c] : 0.f; };
    cnn_layer<3, 1, kCnnCh3, kCnnCg3>(plane2, kCnnCh2, s.hc[2], s.wc[2], P + a.L.w3, P + a.L.g3, P + a.L.b3, l, l.p3);

    if (tid < a.fin.A) l.sc[tid] = cnn_fc(P + a.L.fcw + (int64_t)tid * s.F, P[a.L.fcb + tid], l.p3, s.F);
    __syncthreads();
    if (tid != 0) return;
    // the env's one finishing thread: the draw, then policy_act.hpp's finishing step on (double)score (the score plane stays float32).
    // The float64 scores go where the layers' reduction block was: as a private array they cost the kernel 36 bytes of scratch (profiles/NOTES.md AX)
    static_assert(kActMaxOut <= kRedDoubles, "the reduction block holds the float64 scores");
    for (int k = 0; k < a.fin.A; k++) l.red[k] = (double)l.sc[k];
    act_finish(a.fin, e, l.red, a.score, a.fin.sample ? act_draw(a.key, a.n, a.act_ctr, e) : 0.0);
}

}  // namespace

int cnn_policy_act_launch(Handle *h, const float *params, bool per_env, bool freeze, bool sample, int A, bool none_nan, const uint8_t *images,
                          const uint8_t *done_prev, uint8_t *frozen, void *act, float *score) {
    const srlhip_config &c = h->cfg;
    const int C = c.multi_view ? 6 : 3;
    CnnArgs a{params, images, h->rng.key, h->rng.act_ctr, score, cnn_shape(C, c.img_h, c.img_w), cnn_param_layout(C, c.img_h, c.img_w, A), h->n, per_env ? 1 : 0,
              act_finish_args(h, freeze, sample, A, none_nan, done_prev, frozen, act)};
    const size_t lds = lds_bytes(a.s);
    SRL_HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(cnn_policy_act_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(cnn_policy_act_k, dim3(h->n), dim3(kCnnBlock), lds, h->stream, a);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

}  // namespace srl
