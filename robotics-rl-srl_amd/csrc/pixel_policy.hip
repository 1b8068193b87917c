// pixel_policy.hip — srlhip_pixel_policy_act: ARS's linear policy on the raw frame, np.dot(obs.reshape(-1), M +- noise * delta_k), for every
// env from the frame the rasteriser has just written, as one launch (include/srlhip.h has the contract, pixel_policy.hpp the arithmetic
// and the summation order, policy_act.hpp the finishing step behind the scores: act_finish).
//
// A memory-bound stream.  Envs 2k and 2k + 1 share delta_k and everyone shares M, so a workgroup takes a PAIR: delta_k's [D][A] block is
// read from HBM once and applied to both frames, M comes from L2 / Infinity Cache, and nothing is written but A scores per env.  The
// block is one contiguous run of D A doubles; a wavefront covers 64 rows (64 A doubles) per step with A / 2 loads of 16 bytes per lane
// (A odd: A loads of 8), load i of lane l taking doubles 2 (64 i + l), 2 (64 i + l) + 1: every wave instruction reads 1 KiB contiguous,
// and since the wave advances by whole rows a lane's register i sees the same action column at every step — its accumulators never
// move.  Register i of lane l belongs to the row (2 (64 i + l)) / A of the wave's 64: written to LDS at its flat position the
// accumulators lie as [virtual lane][A], which is where pixel_policy.hpp's tree expects them.
// paired = 0: the same kernel without the delta stream, one env per workgroup.
// SMALL POPULATIONS (fewer work items than CUs): every chunk of kPixChunk rows gets a workgroup of its own, the chunk sums go to the
// handle's partial buffer and the workgroup that arrives last (a ticket per item) adds them in chunk order — the order the unsplit walk
// uses, so the split does not show in the bits.  The hand-off is an agent-scope release / acquire around the ticket; the ticket words are
// zero between launches (the last arriver resets its item's), so the call stays ONE launch and replays from a graph as it is.
// Every global access is guarded: rows at or past D load element 0 and contribute a +0.0 term; the grid is exactly items x split.
#include "internal.hpp"
#include "pixel_policy.hpp"
#include "policy_act.hpp"

namespace srl {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

struct PixArgs {
    const double *weights;       // M [D][A]
    const double *delta;         // [items][D][A] or null
    const uint8_t *images;       // [n][D]
    ActFinish fin;               // (sample is never set: fin.A repeats the kernel's template argument)
    double *score;               // [n][A] or null
    double *part;                // split: [items][chunks][envs of an item][A] chunk sums
    uint32_t *ticket;            // split: [items], zero between launches (allocated zeroed; an item's last arriver puts the zero back)
    double noise;
    int64_t D;
    int32_t chunks, split;
};

template <int VEC> __device__ __forceinline__ void pix_load(const double *p, double (&out)[VEC]) {
    if constexpr (VEC == 2) {
        const d2 v = *reinterpret_cast<const d2 *>(p);
        out[0] = v.x; out[1] = v.y;
    } else out[0] = *p;
}

template <int A, bool PAIRED>
__global__ void __launch_bounds__(kPixLanes) pixel_policy_act_k(PixArgs a) {
    constexpr int VEC = A % 2 == 0 ? 2 : 1, NL = A / VEC, ENVS = PAIRED ? 2 : 1, PLANE = kPixLanes * A;
    __shared__ double red[ENVS * PLANE + 2 * kPixMaxOut + 1];      // one LDS object: the lane partials, the finished scores, the "I am last" word
    double *fin = red + ENVS * PLANE, *last = fin + 2 * kPixMaxOut;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = a.split, item = blockIdx.x / split;
    const int c0 = split > 1 ? (int)(blockIdx.x % split) : 0, c1 = split > 1 ? c0 + 1 : a.chunks;
    const int64_t D = a.D, e0 = (int64_t)item * ENVS;
    const uint8_t *img0 = a.images + e0 * D, *img1 = img0 + (PAIRED ? D : 0);
    const double *dl = PAIRED ? a.delta + (int64_t)item * D * A : nullptr;
    const double noise = a.noise;

    double score = 0.0;                                   // threads 0 .. ENVS A - 1: score [env of the item][a]
    for (int c = c0; c < c1; c++) {
        double acc[ENVS][NL][VEC];
#pragma unroll
        for (int e = 0; e < ENVS; e++)
#pragma unroll
            for (int i = 0; i < NL; i++)
#pragma unroll
                for (int k = 0; k < VEC; k++) acc[e][i][k] = 0.0;
#pragma unroll 2
        for (int j = 0; j < kPixSteps; j++) {
            const int64_t row0 = (int64_t)c * kPixChunk + j * kPixLanes + wave * 64;
            if (row0 >= D) break;                         // (the same for the whole wavefront)
#pragma unroll
            for (int i = 0; i < NL; i++) {
                const int f = (64 * i + lane) * VEC;      // the double inside the wave's 64 rows
                const int64_t row = row0 + f / A;
                const bool ok = row < D;
                const int64_t at = ok ? row0 * A + f : 0, px = ok ? row : 0;
                double m[VEC], dv[VEC];
                pix_load<VEC>(a.weights + at, m);
                if constexpr (PAIRED) pix_load<VEC>(dl + at, dv);
                const uint8_t x0 = img0[px], x1 = img1[px];
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    if constexpr (PAIRED) {
                        double wp, wm;
                        pix_weights(m[k], dv[k], noise, &wp, &wm);
                        acc[0][i][k] = pix_step(acc[0][i][k], x0, ok ? wp : 0.0);
                        acc[1][i][k] = pix_step(acc[1][i][k], x1, ok ? wm : 0.0);
                    } else
                        acc[0][i][k] = pix_step(acc[0][i][k], x0, ok ? m[k] : 0.0);
                }
            }
        }
        // the lane partials as [virtual lane][A] per env, then pixel_policy.hpp's tree: far halves first
#pragma unroll
        for (int e = 0; e < ENVS; e++)
#pragma unroll
            for (int i = 0; i < NL; i++)
#pragma unroll
                for (int k = 0; k < VEC; k++) red[e * PLANE + wave * 64 * A + (64 * i + lane) * VEC + k] = acc[e][i][k];
        __syncthreads();
        for (int h = kPixLanes / 2; h >= 1; h /= 2) {
#pragma clang fp contract(off)
            const int span = h * A;
            for (int idx = tid; idx < ENVS * span; idx += kPixLanes) {
                const int at = (idx / span) * PLANE + idx % span;
                red[at] = red[at] + red[at + span];
            }
            __syncthreads();
        }
        if (tid < ENVS * A) score = pix_chunk_join(c == c0, score, red[(tid / A) * PLANE + tid % A]);
        __syncthreads();
    }

    if (split > 1) {
        // publish this chunk's sums; the last arriver of the item adds all of them in chunk order
        const int64_t slot = (int64_t)item * a.chunks;
        if (tid < ENVS * A) a.part[(slot + c0) * (ENVS * A) + tid] = score;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t t = __hip_atomic_fetch_add(a.ticket + item, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *last = t == (uint32_t)split - 1 ? 1.0 : 0.0;
            if (t == (uint32_t)split - 1) {
                __hip_atomic_store(a.ticket + item, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch on the stream
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (*last == 0.0) return;
        if (tid < ENVS * A)
            for (int c = 0; c < a.chunks; c++)
                score = pix_chunk_join(c == 0, score, __hip_atomic_load(a.part + (slot + c) * (ENVS * A) + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    if (tid < ENVS * A) fin[tid] = score;
    __syncthreads();
    if (tid >= ENVS) return;
    // an env's one finishing thread: policy_act.hpp's finishing step on the env's scores.  Never sampled, so no draw; said here as
    // constants, with A, so that the instantiation carries neither the softmax nor a loop over a run-time A (the scores stay in registers)
    ActFinish f = a.fin;
    f.A = A; f.sample = 0;
    double sc[kPixMaxOut];
#pragma unroll
    for (int k = 0; k < A; k++) sc[k] = fin[tid * A + k];
    act_finish(f, e0 + tid, sc, a.score, 0.0);
}

}  // namespace

int pixel_policy_act_launch(Handle *h, const double *weights, const double *delta, double noise, bool paired, bool freeze, int A, bool none_nan,
                            const uint8_t *images, const uint8_t *done_prev, uint8_t *frozen, void *act, double *score) {
    const srlhip_config &c = h->cfg;
    const int64_t D = (int64_t)frame_bytes(c);
    const int items = paired ? h->n / 2 : h->n, chunks = pix_chunks(D);
    const int split = pix_split(items, chunks) && h->pix_part && h->pix_ticket ? chunks : 1;
    PixArgs a{weights, delta, images, act_finish_args(h, freeze, false, A, none_nan, done_prev, frozen, act), score, h->pix_part, h->pix_ticket, noise, D, chunks, split};
    const bool launched = dispatch_int<2, 3, 4, 6, 7>(A, [&](auto ac) {
        return dispatch_int<0, 1>(paired ? 1 : 0, [&](auto pc) {
            hipLaunchKernelGGL((pixel_policy_act_k<decltype(ac)::value, decltype(pc)::value != 0>), dim3((unsigned)(items * split)), dim3(kPixLanes), 0, h->stream, a);
        });
    });
    if (!launched) return h->fail(SRLHIP_ENOTSUP, "pixel_policy_act: no kernel for this number of policy outputs");
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

}  // namespace srl
