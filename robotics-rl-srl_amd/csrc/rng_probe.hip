// rng_probe.hip — TESTS ONLY: srlhip_selftest_rng.  Runs the script interpreter of rng_probe.hpp over the project's own random
// generators on the device (tests/test_gpu_rng_streams.py holds what they draw to numpy's RandomState and to the Philox4x32-10
// definition).  Built with the flags of the full-model Kuka kernels (csrc/Makefile), where the lane-group generators are used.
#include <string.h>

#include "internal.hpp"
#include "rng_probe.hpp"

namespace srl {
using namespace rngprobe;

namespace {
constexpr int kLaneBlock = 128;                               // per-env forms: one lane per env
constexpr int kRowBlock = grp::kRowsPerWave * grp::GL;        // group forms: one wavefront, four envs (kuka_device.hpp: kGroupBlock)

// The kernels' own guard (kuka_tree_kernels.hpp: kuka_tree_reset_k): a masked-out env and the shadow rows of a tail group never draw.
template <int GEN> __global__ void __launch_bounds__(kLaneBlock) rng_probe_k(Args a) {
    if constexpr (is_group(GEN)) {
        const int e = blockIdx.x * grp::kRowsPerWave + (int)(threadIdx.x / grp::GL);
        const bool valid = e < a.n && !(a.mask && !a.mask[e < a.n ? e : 0]);
        if (!valid) return;
        run_script<GEN>(a, e, grp::lane_id(), grp::GL);
    } else {
        const int e = blockIdx.x * kLaneBlock + threadIdx.x;
        if (e >= a.n || (a.mask && !a.mask[e])) return;
        run_script<GEN>(a, e, 0, 1);
    }
}

struct DeviceBuffers {        // frees what it allocated on every way out
    std::vector<void *> p;
    ~DeviceBuffers() { for (void *q : p) (void)hipFree(q); }
    template <class T> bool alloc(T **out, size_t count, const void *host = nullptr) {
        void *q = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (hipMalloc(&q, bytes) != hipSuccess) return false;
        p.push_back(q);
        *out = static_cast<T *>(q);
        if (host) return hipMemcpy(q, host, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
        return hipMemset(q, 0, bytes) == hipSuccess;
    }
};
}  // namespace

int rng_probe_run(int generator, int stream, int n, int stride, const uint32_t *keys, const int32_t *key_len, const uint8_t *mask,
                  const uint64_t *state_in, const int32_t *script, int n_ops, const double *args, int n_args, const int32_t *skip,
                  uint64_t *out, int64_t out_words, uint64_t *state_out, int64_t state_words) {
    const int64_t values = script_values(generator, script, n_ops, args, n_args);
    if (values < 0 || n < 1 || n > 4096 || !keys || !skip || !out || !state_out || (stream != 0 && stream != 1)) return SRLHIP_EINVAL;
    const bool mt = is_mt(generator), group = is_group(generator);
    const int lanes = group ? grp::GL : 1, sw = mt ? kMtStateWords : 1;
    if (mt && (stride < n || stride > 8192)) return SRLHIP_EINVAL;
    if (mt && !state_in && !key_len) return SRLHIP_EINVAL;
    if (out_words < (int64_t)n * lanes * values || state_words < (int64_t)n * sw) return SRLHIP_EINVAL;
    for (int e = 0; e < n; e++) {
        if (skip[e] < 0 || skip[e] > kMaxSkip) return SRLHIP_EINVAL;
        if (mt && !state_in && key_len[e] != 1 && key_len[e] != 2) return SRLHIP_EINVAL;
    }
    DeviceBuffers db;
    Args a = {};
    a.stream = stream; a.n = n; a.n_ops = n_ops; a.values = values;
    const size_t out_count = (size_t)n * lanes * values;
    int32_t *d_script = nullptr, *d_skip = nullptr; double *d_args = nullptr; uint8_t *d_mask = nullptr; uint32_t *d_keys = nullptr;
    if (!db.alloc(&d_script, 3 * (size_t)n_ops, n_ops ? script : nullptr) || !db.alloc(&d_args, n_args, n_args ? args : nullptr) ||
        !db.alloc(&d_skip, n, skip) || !db.alloc(&d_keys, 2 * (size_t)n, keys) || !db.alloc(&a.out, out_count) ||
        (mask && !db.alloc(&d_mask, n, mask)))
        return SRLHIP_ENOMEM;
    a.script = d_script; a.args = d_args; a.skip = d_skip; a.keys = d_keys; a.mask = d_mask;
    std::vector<uint32_t> words; std::vector<int32_t> mti, has; std::vector<double> gauss;
    if (mt) {
        const size_t s = (size_t)stride;
        a.mt.stride = stride;
        if (state_in) {           // install a state another probe call returned
            words.assign(MT_N * s, 0u); mti.assign(s, 0); has.assign(s, 0); gauss.assign(s, 0.0);
            for (int e = 0; e < n; e++) {
                const uint64_t *st = state_in + (size_t)e * kMtStateWords;
                if (st[MT_N] > (uint64_t)MT_N || st[MT_N + 1] > 1) return SRLHIP_EINVAL;       // an index past 624 would read past the words
                for (int k = 0; k < MT_N; k++) words[k * s + e] = (uint32_t)st[k];
                mti[e] = (int32_t)st[MT_N]; has[e] = (int32_t)st[MT_N + 1]; memcpy(&gauss[e], &st[MT_N + 2], 8);
            }
        }
        if (!db.alloc(&a.mt.mt, MT_N * s, state_in ? words.data() : nullptr) || !db.alloc(&a.mt.mti, s, state_in ? mti.data() : nullptr) ||
            !db.alloc(&a.mt.has_gauss, s, state_in ? has.data() : nullptr) || !db.alloc(&a.mt.gauss, s, state_in ? gauss.data() : nullptr))
            return SRLHIP_ENOMEM;
        if (!state_in) {          // RandomState.seed(key) for every env by srlhip_seed's own kernel
            int32_t *d_len = nullptr;
            if (!db.alloc(&d_len, n, key_len)) return SRLHIP_ENOMEM;
            if (mt_seed_launch(a.mt, n, nullptr, d_keys, d_len, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SRLHIP_EHIP;
        }
    } else {
        if (!db.alloc(&a.ctr, n, state_in)) return SRLHIP_ENOMEM;
    }
    const dim3 grid(group ? (n + grp::kRowsPerWave - 1) / grp::kRowsPerWave : (n + kLaneBlock - 1) / kLaneBlock), block(group ? kRowBlock : kLaneBlock);
    switch (generator) {
        case GEN_MT: hipLaunchKernelGGL(rng_probe_k<GEN_MT>, grid, block, 0, 0, a); break;
        case GEN_GROUP_MT: hipLaunchKernelGGL(rng_probe_k<GEN_GROUP_MT>, grid, block, 0, 0, a); break;
        case GEN_LANE0_MT: hipLaunchKernelGGL(rng_probe_k<GEN_LANE0_MT>, grid, block, 0, 0, a); break;
        case GEN_PHILOX: hipLaunchKernelGGL(rng_probe_k<GEN_PHILOX>, grid, block, 0, 0, a); break;
        case GEN_GROUP_PHILOX: hipLaunchKernelGGL(rng_probe_k<GEN_GROUP_PHILOX>, grid, block, 0, 0, a); break;
        default: hipLaunchKernelGGL(rng_probe_k<GEN_GROUP_ACTIONS>, grid, block, 0, 0, a);
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SRLHIP_EHIP;
    if (out_count && hipMemcpy(out, a.out, out_count * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return SRLHIP_EHIP;
    if (mt) {
        const size_t s = (size_t)stride;
        words.resize(MT_N * s); mti.resize(s); has.resize(s); gauss.resize(s);
        if (hipMemcpy(words.data(), a.mt.mt, MT_N * s * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(mti.data(), a.mt.mti, s * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(has.data(), a.mt.has_gauss, s * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(gauss.data(), a.mt.gauss, s * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return SRLHIP_EHIP;
        for (int e = 0; e < n; e++) {
            uint64_t *st = state_out + (size_t)e * kMtStateWords;
            for (int k = 0; k < MT_N; k++) st[k] = words[k * s + e];
            st[MT_N] = (uint64_t)(uint32_t)mti[e]; st[MT_N + 1] = (uint64_t)(uint32_t)has[e]; memcpy(&st[MT_N + 2], &gauss[e], 8);
        }
    } else if (hipMemcpy(state_out, a.ctr, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return SRLHIP_EHIP;
    return 0;
}

}  // namespace srl
