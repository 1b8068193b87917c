// api.hip — C-ABI front end of libsrlhip (include/srlhip.h): handle lifetime,
// seeding, host<->device staging, state access, timing.  The env kernels live
// in mobile.hip / kuka.hip.
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <cmath>
#include <new>

#include "internal.hpp"

using namespace srl;

namespace {

thread_local std::string g_create_error;
constexpr int kBlock = 256;

// RandomState.seed(digits) for the selected envs, one lane per env.
__global__ void mt_seed_k(Mt19937View v, int n, const uint8_t *mask, const uint32_t *digits, const int32_t *len) {
    int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n || (mask && !mask[e])) return;
    uint32_t key[2] = {digits[e], digits[n + e]};
    Mt19937 m;
    m.load(v, e);
    m.seed_by_array(key, len[e]);
    m.store(v, e);
}

__global__ void key_seed_k(RngState r, int n, const uint8_t *mask, const uint32_t *lohi) {
    int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n || (mask && !mask[e])) return;
    r.key[e] = lohi[e]; r.key[n + e] = lohi[n + e];
    r.ctr[e] = 0; r.act_ctr[e] = 0;
}

int ensure_pinned(Handle *h, PinBuf &b, size_t bytes) {
    if (b.cap >= bytes) return 0;
    if (b.p) (void)hipHostFree(b.p);
    b = PinBuf{};
    // mapped: kernels may address it directly (zero-copy step); coherent (fine-grained): what a RESIDENT kernel writes and releases at
    // system scope is visible to the host while the kernel is still running (persistent stepping; + 16: its copy works in dwords)
    SRL_HIP_CHECK(h, hipHostMalloc(&b.p, bytes + 16, hipHostMallocMapped | hipHostMallocCoherent));
    b.cap = bytes;
    return 0;
}
int stage_in(Handle *h, DevBuf &b, const void *host, size_t bytes) {
    int rc = ensure(h, b, bytes);
    if (rc) return rc;
    SRL_HIP_CHECK(h, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// the handle's step buffers (api_rules.hpp); SRLHIP_ZERO_COPY=0: bounce buffers even where the zero-copy step applies (read once)
StepLayout step_layout(const Handle *h) {
    static const bool zc_enabled = [] { const char *v = getenv("SRLHIP_ZERO_COPY"); return !v || atoi(v) != 0; }();
    return srl::step_layout(h->cfg, (size_t)h->n, zc_enabled);
}

// ---- persistent stepping: host side of the protocol (step_signal.hpp) -------------------------------------------------------------------
PersistHost *persist_ctl(Handle *h) { return static_cast<PersistHost *>(h->persist_host); }

// Resident kernels of several handles on ONE device (the shards of HipVecEnv(device_ids=[0, 0])) must all fit at once: a workgroup that
// waits for the host never makes room for another kernel's.  Per-device tally of the grids of the handles in persistent mode, process-wide.
std::mutex g_persist_mu;
int g_persist_reserved[64] = {0};
void persist_release(Handle *h) {
    if (!h->persist_reserved) return;
    std::lock_guard<std::mutex> lk(g_persist_mu);
    g_persist_reserved[h->cfg.device_id & 63] -= h->persist_reserved;
    h->persist_reserved = 0;
}

// the mapped control block + the device words shared by persistent stepping and by the early completion signal of single-step launches
int ensure_signal_buffers(Handle *h) {
    if (h->persist_host) return 0;
    const size_t bytes = sizeof(PersistHost), blocks = ((size_t)h->n + 3) / 4;
    if (hipHostMalloc(&h->persist_host, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return h->fail(SRLHIP_ENOMEM, "step: hipHostMalloc (control block) failed");
    memset(h->persist_host, 0, bytes);
    const size_t words = signal_words(blocks);
    if (hipMalloc(reinterpret_cast<void **>(&h->persist_relay), words * sizeof(uint32_t)) != hipSuccess) return h->fail(SRLHIP_ENOMEM, "step: hipMalloc (control words) failed");
    SRL_HIP_CHECK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->persist_relay), 0, words, h->stream));
    return 0;
}

// the resident kernel writes the state back and exits; afterwards the handle is an ordinary one again
int persist_park(Handle *h) {
    if (!h->persist_running) return 0;
    PersistHost *c = persist_ctl(h);
    __atomic_store_n(&c->stop, 1u, __ATOMIC_RELEASE);
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    c->stop = 0; c->parked = 0;
    h->persist_running = false;
    return 0;
}

// step_pair: the caller is srlhip_step / _async / _wait.  Every OTHER entry point sees the state in HBM: the resident kernel parks first.
int set_device(Handle *h, bool step_pair = false) {
    SRL_HIP_CHECK(h, hipSetDevice(h->cfg.device_id));
    if (h->persist_running && !step_pair) return persist_park(h);
    return 0;
}

// (re)start the resident kernel; it will treat `start_seq` as the last step it has done
int persist_launch(Handle *h, uint32_t start_seq) {
    PersistHost *c = persist_ctl(h);
    c->stop = 0; c->parked = 0;
    for (uint32_t g = 0; g < 8; g++) c->done[kDoneResident + g] = start_seq;
    SRL_HIP_CHECK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->persist_relay + kWordRelay), (int)start_seq, kWordCount - kWordRelay, h->stream));
    SRL_HIP_CHECK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->persist_relay + kWordCount), 0, kWordStepCount - kWordCount, h->stream));
    void *dctl = nullptr, *din = nullptr, *dout = nullptr;
    SRL_HIP_CHECK(h, hipHostGetDevicePointer(&dctl, h->persist_host, 0));
    SRL_HIP_CHECK(h, hipHostGetDevicePointer(&din, h->pin[PIN_IN].p, 0));
    SRL_HIP_CHECK(h, hipHostGetDevicePointer(&dout, h->pin[PIN_OUT].p, 0));
    PersistArgs pa = signal_args(SignalKind::resident, dctl, h->persist_relay);
    pa.start_seq = start_seq;
    { const char *v = getenv("SRLHIP_PERSIST_STAGED"); pa.force_staged = v && atoi(v) != 0; }
    pa.spin_limit = h->persist_park_us / 2 + 1;        // one poll of workgroup 0: one 8-byte PCIe read + s_sleep 8, ~2 us
    const StepLayout L = step_layout(h);
    pa.stage = static_cast<const uint32_t *>(h->persist_stage); pa.host_out = static_cast<uint32_t *>(dout);
    pa.rew_dw = (uint32_t)(L.out_rew / 4); pa.done_dw = (uint32_t)(L.out_done / 4);
    int rc = env_ops(h).persist_start(h, din, pa);
    if (rc) return rc;
    h->persist_running = true;
    return 0;
}

int seed_impl(Handle *h, const uint8_t *mask, const int64_t *seeds) {
    const int n = h->n;
    std::vector<uint32_t> lohi(2 * (size_t)n), digits(2 * (size_t)n);
    std::vector<int32_t> len(n);
    for (int i = 0; i < n; i++) {
        uint64_t s = (uint64_t)seeds[i];
        lohi[i] = (uint32_t)s; lohi[n + i] = (uint32_t)(s >> 32);
        if (h->cfg.rng_mode == SRLHIP_RNG_MT19937 && (!mask || mask[i])) {
            if (seeds[i] < 0) return h->fail(SRLHIP_EINVAL, "seed must be a non-negative integer (gym seeding)");
            uint32_t d[2];
            len[i] = gym_hash_seed(s, d);
            if (len[i] == 0) return h->fail(SRLHIP_EINVAL, "seed hashes to an empty key");
            digits[i] = d[0]; digits[n + i] = d[1];
        }
    }
    int rc;
    const uint8_t *d_mask = nullptr;
    if (mask) {
        if ((rc = stage_in(h, h->st[ST_MASK], mask, n))) return rc;
        d_mask = static_cast<const uint8_t *>(h->st[ST_MASK].p);
    }
    dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    if ((rc = stage_in(h, h->st[ST_RAND], lohi.data(), lohi.size() * 4))) return rc;
    hipLaunchKernelGGL(key_seed_k, grid, block, 0, h->stream, h->rng, n, d_mask,
                       static_cast<const uint32_t *>(h->st[ST_RAND].p));
    SRL_HIP_CHECK(h, hipGetLastError());
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));   // host vectors die at return
    if (h->cfg.rng_mode == SRLHIP_RNG_MT19937) {
        if ((rc = stage_in(h, h->st[ST_RAND], digits.data(), digits.size() * 4))) return rc;
        if ((rc = stage_in(h, h->st[ST_NOISE], len.data(), len.size() * 4))) return rc;
        SRL_HIP_CHECK(h, mt_seed_launch(h->rng.mt, n, d_mask, static_cast<const uint32_t *>(h->st[ST_RAND].p), static_cast<const int32_t *>(h->st[ST_NOISE].p), h->stream));
        SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

// srlhip_episode_stats_device: Monitor's per-env (r, l) of the last finished episode as f32 / i32 planes in caller memory
__global__ void episode_stats_k(EpisodeStats st, int n, float *ret, int32_t *len, int32_t *fin) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (ret) ret[e] = (float)st.last_return[e];
    if (len) len[e] = st.last_length[e];
    if (fin) fin[e] = st.n_finished[e];
}

int field_lookup(Handle *h, int field, void **dptr, size_t *elem, int *count) {
    *count = 1;
    switch (field) {
        case SRLHIP_F_LAST_RETURN: *dptr = h->stats.last_return; *elem = 8; return 0;
        case SRLHIP_F_LAST_LENGTH: *dptr = h->stats.last_length; *elem = 4; return 0;
        case SRLHIP_F_N_FINISHED: *dptr = h->stats.n_finished; *elem = 4; return 0;
        case SRLHIP_F_LAST_REWARD: *dptr = h->stats.last_reward; *elem = 8; return 0;
        case SRLHIP_F_EP_RETURN: *dptr = h->stats.ep_return; *elem = 8; return 0;
        case SRLHIP_F_EP_LENGTH: *dptr = h->stats.ep_length; *elem = 4; return 0;
    }
    return env_ops(h).field(h, field, dptr, elem, count);
}

}  // namespace

// RandomState.seed for the envs of a view: srlhip_seed's launch, also what the generator self-test (rng_probe.hip) seeds with
hipError_t srl::mt_seed_launch(const Mt19937View &v, int n, const uint8_t *d_mask, const uint32_t *d_digits, const int32_t *d_len, hipStream_t stream) {
    hipLaunchKernelGGL(mt_seed_k, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, v, n, d_mask, d_digits, d_len);
    return hipGetLastError();
}

extern "C" {

int srlhip_abi_version(void) { return SRLHIP_ABI_VERSION; }

int srlhip_default_config(int32_t env_kind, srlhip_config *cfg) {
    if (!cfg || !(is_mobile(env_kind) || is_kuka(env_kind))) return SRLHIP_EINVAL;
    fill_default_config(env_kind, cfg);
    return 0;
}

const char *srlhip_last_error(srlhip_handle hh) {
    if (!hh) return g_create_error.c_str();
    return reinterpret_cast<Handle *>(hh)->err.c_str();
}

int srlhip_create(const srlhip_config *cfg, srlhip_handle *out) {
    if (!cfg || !out) { g_create_error = "create: null argument"; return SRLHIP_EINVAL; }
    *out = nullptr;
    if (const Verdict v = check_config(*cfg); v.code) { g_create_error = v.msg; return v.code; }
    hipError_t e = hipSetDevice(cfg->device_id);
    if (e != hipSuccess) {
        g_create_error = std::string("create: hipSetDevice failed (no MI355X visible?): ") + hipGetErrorString(e);
        return SRLHIP_EHIP;
    }
    Handle *h = new (std::nothrow) Handle();
    if (!h) { g_create_error = "create: out of host memory"; return SRLHIP_ENOMEM; }
    h->cfg = *cfg; h->n = cfg->num_envs;
    int rc = 0;
    auto bail = [&](int code) { g_create_error = h->err; srlhip_destroy(reinterpret_cast<srlhip_handle>(h)); return code; };
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        h->err = "create: hipStreamCreate failed";
        return bail(SRLHIP_EHIP);
    }
    (void)hipEventCreate(&h->ev_begin); (void)hipEventCreate(&h->ev_end);
    const size_t n = (size_t)h->n;
    if ((rc = h->dalloc(&h->rng.key, 2 * n)) || (rc = h->dalloc(&h->rng.ctr, n)) || (rc = h->dalloc(&h->rng.act_ctr, n)))
        return bail(rc);
    if (cfg->rng_mode == SRLHIP_RNG_MT19937) {
        h->rng.mt.stride = (int64_t)n;
        if ((rc = h->dalloc(&h->rng.mt.mt, (size_t)MT_N * n)) || (rc = h->dalloc(&h->rng.mt.mti, n)) ||
            (rc = h->dalloc(&h->rng.mt.has_gauss, n)) || (rc = h->dalloc(&h->rng.mt.gauss, n)))
            return bail(rc);
    }
    EpisodeStats &st = h->stats;
    if ((rc = h->dalloc(&st.ep_return, n)) || (rc = h->dalloc(&st.ep_length, n)) || (rc = h->dalloc(&st.n_finished, n)) || (rc = h->dalloc(&st.last_reward, n)))
        return bail(rc);
    if (!cfg->io_device) {
        // Monitor's (r, l) of the last finished episode where the host can read them without a copy: the kernels' exit stores go
        // over PCIe (12 bytes per env and launch), srlhip_episode_records() hands out the host view
        void *dp = nullptr;
        if (hipHostMalloc(&h->ep_host, episode_block_bytes(n), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&dp, h->ep_host, 0) != hipSuccess) {
            h->err = "create: hipHostMalloc (episode records) failed"; return bail(SRLHIP_ENOMEM);
        }
        memset(h->ep_host, 0, episode_block_bytes(n));
        st.last_return = episode_returns(dp);
        st.last_length = episode_lengths(dp, n);
    } else if ((rc = h->dalloc(&st.last_return, n)) || (rc = h->dalloc(&st.last_length, n))) return bail(rc);
    if ((rc = env_ops(h).alloc(h))) return bail(rc);
    if (cfg->io_device && cfg->obs_mode == SRLHIP_OBS_RAW_PIXELS &&
        ((rc = h->dalloc(&h->pix_part, (size_t)kPixSplitWgs * kPixSplitSlot)) || (rc = h->dalloc(&h->pix_ticket, (size_t)kPixSplitItems))))
        return bail(rc);
    std::vector<int64_t> seeds(n);
    for (size_t i = 0; i < n; i++) seeds[i] = cfg->seed0 + cfg->first_env_id + (int64_t)i;   // environments/utils.py:52
    if ((rc = seed_impl(h, nullptr, seeds.data()))) return bail(rc);
    if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "create: device initialisation failed"; return bail(SRLHIP_EHIP); }
    *out = reinterpret_cast<srlhip_handle>(h);
    return 0;
}

int srlhip_destroy(srlhip_handle hh) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    (void)hipSetDevice(h->cfg.device_id);
    h->persist_step = false;
    (void)persist_park(h);
    persist_release(h);
    if (getenv("SRLHIP_DEBUG_SIGNAL")) fprintf(stderr, "srlhip: handle n=%d: %u signalled steps, %u fell back to the stream synchronisation (XCD mismatch), %u timed out\n", h->n, h->signal_steps, h->signal_fallbacks & 0xffffu, h->signal_fallbacks >> 16);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->persist_host) (void)hipHostFree(h->persist_host);
    if (h->persist_relay) (void)hipFree(h->persist_relay);
    if (h->persist_stage) (void)hipFree(h->persist_stage);
    if (h->kuka) kuka_free(h);
    for (void *p : h->allocs) (void)hipFree(p);
    for (const DevBuf &b : h->st) if (b.p) (void)hipFree(b.p);
    for (const DevBuf &b : h->act_plane) if (b.p) (void)hipFree(b.p);
    for (const PinBuf &b : h->pin) if (b.p) (void)hipHostFree(b.p);
    if (h->ep_host) (void)hipHostFree(h->ep_host);
    if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
    if (h->ev_end) (void)hipEventDestroy(h->ev_end);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int srlhip_obs_dim(srlhip_handle hh) { return hh ? obs_dim_of(reinterpret_cast<Handle *>(hh)->cfg) : SRLHIP_EINVAL; }
int srlhip_obs_bytes(srlhip_handle hh) { return hh ? (int)obs_bytes_per_env(reinterpret_cast<Handle *>(hh)->cfg) : SRLHIP_EINVAL; }
int srlhip_action_dim(srlhip_handle hh) { return hh ? action_dim_of(reinterpret_cast<Handle *>(hh)->cfg) : SRLHIP_EINVAL; }
int srlhip_num_actions(srlhip_handle hh) { return hh ? num_actions_of(reinterpret_cast<Handle *>(hh)->cfg) : SRLHIP_EINVAL; }

int srlhip_reset_rand_count(srlhip_handle hh) { return hh ? reset_rand_count(reinterpret_cast<Handle *>(hh)->cfg) : SRLHIP_EINVAL; }

int srlhip_seed(srlhip_handle hh, const uint8_t *mask, const int64_t *seeds) {
    if (!hh || !seeds) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    h->prefetch_valid = false;                  // the action-stream counters restart
    h->snap_valid = false;
    return rc ? rc : seed_impl(h, mask, seeds);
}

int srlhip_reset(srlhip_handle hh, const uint8_t *mask, const double *host_rand, void *obs_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    const int n = h->n;
    const uint8_t *d_mask = nullptr;
    if (mask) {
        if ((rc = stage_in(h, h->st[ST_MASK], mask, n))) return rc;
        d_mask = static_cast<const uint8_t *>(h->st[ST_MASK].p);
    }
    const double *d_rand = host_rand;
    void *d_obs = obs_out;
    const size_t ob = obs_bytes_per_env(h->cfg) * n;
    if (!h->cfg.io_device) {
        if (host_rand) {
            size_t bytes = sizeof(double) * (size_t)reset_rand_count(h->cfg) * n;
            if ((rc = stage_in(h, h->st[ST_RAND], host_rand, bytes))) return rc;
            d_rand = static_cast<const double *>(h->st[ST_RAND].p);
        }
        if (obs_out) {
            // unselected rows must keep the caller's contents
            if ((rc = stage_in(h, h->st[ST_OBS], obs_out, ob))) return rc;
            d_obs = h->st[ST_OBS].p;
        }
    }
    const bool pixels = h->cfg.obs_mode == SRLHIP_OBS_RAW_PIXELS;
    if ((rc = env_ops(h).reset(h, d_mask, d_rand, pixels ? nullptr : d_obs))) return rc;
    if (pixels && d_obs && (rc = raster_render(h, d_obs))) return rc;     // every env is (re)drawn: rows of unselected envs too
    if (!h->cfg.io_device) {
        if (obs_out) SRL_HIP_CHECK(h, hipMemcpyAsync(obs_out, d_obs, ob, hipMemcpyDeviceToHost, h->stream));
        SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    } else if (mask) {
        SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));   // staged mask must stay valid
    }
    return 0;
}

}  // extern "C"

namespace {
// The host-pointer step in two halves (srlhip_step = both, srlhip_step_async / srlhip_step_wait = one each).
// (the buffers' layout and the zero-copy rule: api_rules.hpp, StepLayout)

// validate + stage the inputs, enqueue the step (and, in bounce mode, the D2H copy of its outputs) on the handle's stream; no wait
int host_step_begin(Handle *h, const void *actions, const double *host_noise, bool want_obs) {
    const int n = h->n;
    const StepLayout L = step_layout(h);
    int rc;
    if (!h->cfg.is_discrete && !continuous_actions_ok(h->cfg, static_cast<const float *>(actions), (size_t)n))
        return h->fail(SRLHIP_EINVAL, "step: non-finite continuous action (a Kuka env's `None` is a row of NaNs)");
    if (host_noise && !all_finite_f64(host_noise, (size_t)n)) return h->fail(SRLHIP_EINVAL, "step: non-finite host_noise");
    if ((rc = ensure_pinned(h, h->pin[PIN_IN], L.in_total)) || (rc = ensure_pinned(h, h->pin[PIN_OUT], L.out_total)))
        return rc;
    void *const pin_in = h->pin[PIN_IN].p;
    if (h->cfg.is_discrete) {
        if (!copy_discrete_checked(static_cast<const int32_t *>(actions), static_cast<int32_t *>(pin_in), (size_t)n, num_actions_of(h->cfg)))
            return h->fail(SRLHIP_EINVAL, "step: discrete action out of range (valid: -1 = no-op, 0 .. num_actions - 1)");
    } else {
        memcpy(pin_in, actions, L.ab);
    }
    if (host_noise) memcpy(static_cast<uint8_t *>(pin_in) + L.in_noise, host_noise, sizeof(double) * n);
    uint8_t *din = nullptr, *o = nullptr;
    if (L.zero_copy) {
        void *dp = nullptr;
        SRL_HIP_CHECK(h, hipHostGetDevicePointer(&dp, pin_in, 0));
        din = static_cast<uint8_t *>(dp);
        SRL_HIP_CHECK(h, hipHostGetDevicePointer(&dp, h->pin[PIN_OUT].p, 0));
        o = static_cast<uint8_t *>(dp);
    } else {
        if ((rc = ensure(h, h->st[ST_ACTIONS], L.in_total)) || (rc = ensure(h, h->st[ST_OBS], L.out_total)))
            return rc;
        SRL_HIP_CHECK(h, hipMemcpyAsync(h->st[ST_ACTIONS].p, pin_in, host_noise ? L.in_total : L.ab, hipMemcpyHostToDevice, h->stream));
        din = static_cast<uint8_t *>(h->st[ST_ACTIONS].p);
        o = static_cast<uint8_t *>(h->st[ST_OBS].p);
    }
    if (h->persist_on && L.zero_copy && !host_noise) {
        // persistent stepping: no launch — (re)start the resident kernel if it is parked, then hand it the step's sequence number
        PersistHost *c = persist_ctl(h);
        if (h->persist_running && c->parked) { if ((rc = persist_park(h))) return rc; }
        if (!h->persist_running && (rc = persist_launch(h, h->persist_seq))) return rc;
        h->persist_seq = h->persist_seq + 1 == kPersistPark ? 1 : h->persist_seq + 1;
        __atomic_store_n(&c->seq, h->persist_seq, __ATOMIC_RELEASE);       // the actions above are visible before the number
        h->persist_step = true;                        // host_step_finish collects this step from the resident kernel
        return 0;
    }
    const double *d_noise = host_noise ? reinterpret_cast<const double *>(din + L.in_noise) : nullptr;
    void *d_obs = want_obs ? o : nullptr;
    float *d_rew = reinterpret_cast<float *>(o + L.out_rew);
    uint8_t *d_done = o + L.out_done;
    // Early completion signal (zero-copy steps of the full-model Kuka kernels and of the MobileRobot per-step kernel; SRLHIP_STEP_SIGNAL=0:
    // always wait for the kernel's end):
    // the kernel reports the step's outputs per eighth of its grid (kuka_tree_kernels.hpp), host_step_finish polls those words instead
    // of synchronising the stream — the kernel's exit stores and the completion wake-up leave the step's latency.
    static const bool sig_enabled = [] { const char *v = getenv("SRLHIP_STEP_SIGNAL"); return !v || atoi(v) != 0; }();
    h->signal_wait = false;
    if (sig_enabled && L.zero_copy && !host_noise && !ensure_signal_buffers(h)) {
        if (h->signal_seq >= 0xfffffff0u) {               // the arrival counters count in step with the sequence number: restart both
            SRL_HIP_CHECK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->persist_relay + kWordStepCount), 0, kWordStamps - kWordStepCount, h->stream));
            h->signal_seq = 0;
        }
        void *dctl = nullptr;
        SRL_HIP_CHECK(h, hipHostGetDevicePointer(&dctl, h->persist_host, 0));
        h->step_signal = signal_args(SignalKind::single_step, dctl, h->persist_relay);
        h->step_signal.start_seq = h->signal_seq + 1;
        h->step_signal_armed = false;
    }
    rc = env_ops(h).step(h, din, d_noise, L.pixels ? nullptr : d_obs, d_rew, d_done);
    h->step_signal = PersistArgs{};
    if (rc) return rc;
    if (h->step_signal_armed) { h->signal_seq += 1; h->signal_wait = true; h->step_signal_armed = false; }
    if (L.pixels && d_obs && (rc = raster_render(h, d_obs))) return rc;
    if (!L.zero_copy) {
        const size_t from = want_obs ? 0 : L.out_rew;
        SRL_HIP_CHECK(h, hipMemcpyAsync(static_cast<uint8_t *>(h->pin[PIN_OUT].p) + from, static_cast<uint8_t *>(h->st[ST_OBS].p) + from,
                                        L.out_total - from, hipMemcpyDeviceToHost, h->stream));
    }
    return 0;
}

// wait for the step enqueued by host_step_begin and hand its planes to the caller
int host_step_finish(Handle *h, void *obs_out, float *reward_out, uint8_t *done_out) {
    const StepLayout L = step_layout(h);
    if (h->persist_step) {
        // wait for every workgroup's `done` word; a kernel that parked before it saw this step (its timeout ran out while the caller
        // was busy) is restarted: workgroup 0 relays either the step to everybody or the park token to everybody, never a mix
        PersistHost *c = persist_ctl(h);
        const uint32_t want = h->persist_seq;
        h->persist_step = false;
        uint64_t spins = 0;
        const auto t0 = std::chrono::steady_clock::now();
        // (eighth g reports iff it holds a real workgroup: persist_eighths, set with the mode)
        for (uint32_t b = 0; b < 8; b++) {
            while (((h->persist_eighths >> b) & 1u) && __atomic_load_n(&c->done[kDoneResident + b], __ATOMIC_ACQUIRE) != want) {
                if ((++spins & 1023u) != 0) continue;
                if (c->parked) {
                    int rc = persist_park(h);
                    if (rc) return rc;
                    if ((rc = persist_launch(h, want == 1 ? kPersistPark - 1 : want - 1))) return rc;
                    b = 0;
                } else if ((spins & ((1u << 20) - 1)) == 0) {
                    // every few ms: a kernel that is gone without having parked has failed; a step never takes 20 s
                    if (hipStreamQuery(h->stream) != hipErrorNotReady) { h->persist_running = false; return h->fail(SRLHIP_EHIP, "persistent step: the resident kernel is gone"); }
                    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
                        (void)persist_park(h);
                        return h->fail(SRLHIP_EHIP, "persistent step: timed out (a workgroup of the resident kernel never started: is the device shared?)");
                    }
                }
            }
        }
    } else if (h->signal_wait) {
        // the early completion signal of a single-step launch: every eighth of the grid that holds a real workgroup reports the step's
        // sequence number.  Nothing depends on the signal ARRIVING: after ~2 ms without it (or when a workgroup found itself on another
        // XCD than its eighth's) the stream synchronisation below is the answer, as before.
        h->signal_wait = false;
        PersistHost *c = persist_ctl(h);
        const uint32_t want = h->signal_seq;
        bool seen = true;
        uint64_t spins = 0;
        const auto t0 = std::chrono::steady_clock::now();
        bool split = false;                              // an eighth of the grid reported from more than one XCD (~want)
        for (uint32_t b = 0; seen && b < 8; b++)
            for (; (h->signal_eighths >> b) & 1u;) {
                const uint32_t v = __atomic_load_n(&c->done[kDoneStep + b], __ATOMIC_ACQUIRE);
                if (v == want) break;
                if (v == ~want) { split = true; break; }
                if ((++spins & 4095u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) { seen = false; break; }
            }
        if (!seen || split) {
            h->signal_fallbacks += 1 + (seen ? 0 : 0x10000);
            SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
        }
        h->signal_steps++;
    } else
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    const uint8_t *po = static_cast<const uint8_t *>(h->pin[PIN_OUT].p);
    if (obs_out) memcpy(obs_out, po, L.ob);
    if (reward_out) memcpy(reward_out, po + L.out_rew, 4 * (size_t)h->n);
    if (done_out) memcpy(done_out, po + L.out_done, h->n);
    return 0;
}

// ---- rollouts on host-pointer handles: the output planes' device twins --------------------------------------------------------------------
struct RolloutPlanes { void *obs; float *rew; uint8_t *done; void *act; };      // [T][n] each; null: not wanted
// every wanted plane of `d` (host pointers on entry) becomes its staging buffer
int stage_rollout_planes(Handle *h, int32_t T, RolloutPlanes &d) {
    const size_t tn = (size_t)h->n * (size_t)T;
    int rc;
    if (d.act) { if ((rc = ensure(h, h->st[ST_ACTIONS], action_bytes(h->cfg, tn)))) return rc; d.act = h->st[ST_ACTIONS].p; }
    if (d.obs) { if ((rc = ensure(h, h->st[ST_OBS], obs_bytes_per_env(h->cfg) * tn))) return rc; d.obs = h->st[ST_OBS].p; }
    if (d.rew) { if ((rc = ensure(h, h->st[ST_REW], 4 * tn))) return rc; d.rew = static_cast<float *>(h->st[ST_REW].p); }
    if (d.done) { if ((rc = ensure(h, h->st[ST_DONE], tn))) return rc; d.done = static_cast<uint8_t *>(h->st[ST_DONE].p); }
    return 0;
}
// ... and back: the planes staged in `dev` (a null dev.act: none was recorded) to the host's, then the call's one synchronisation
int fetch_rollout_planes(Handle *h, int32_t T, const RolloutPlanes &host, const RolloutPlanes &dev) {
    const size_t tn = (size_t)h->n * (size_t)T;
    if (host.obs) SRL_HIP_CHECK(h, hipMemcpyAsync(host.obs, dev.obs, obs_bytes_per_env(h->cfg) * tn, hipMemcpyDeviceToHost, h->stream));
    if (host.rew) SRL_HIP_CHECK(h, hipMemcpyAsync(host.rew, dev.rew, 4 * tn, hipMemcpyDeviceToHost, h->stream));
    if (host.done) SRL_HIP_CHECK(h, hipMemcpyAsync(host.done, dev.done, tn, hipMemcpyDeviceToHost, h->stream));
    if (host.act && dev.act) SRL_HIP_CHECK(h, hipMemcpyAsync(host.act, dev.act, action_bytes(h->cfg, tn), hipMemcpyDeviceToHost, h->stream));
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the fused policy rollouts (and srlhip_policy_act's struct checks): one host path -----------------------------------------------------
// Order of the checks (their text: api_rules.hpp), as before the entry points shared them: check_policy_abi (null policy, struct_size),
// policy_call_begin (T, a pending step), check_policy_shape (the MLP's hidden and reserved), then — in rollout_policy —
// check_policy_pointers, check_rollout_policy_config and, on a host-pointer handle after the device is set, check_policy_values.
// what differs between the entry points
struct PolicyCall {
    const char *name;              // the entry point, as every message begins
    KukaPolicyLaunch kuka;
    bool sample = false;           // srlhip_rollout_policy_sampled / srlhip_rollout_mlp_policy_sampled: the discrete action is drawn from the softmax of the scores
};
int refuse(Handle *h, const char *name, const Verdict &v) { return h->fail(v.code, std::string(name) + ": " + v.msg); }      // (built on a failing call only)
PolicyArgs policy_args(const PolicyView &v) {
    return PolicyArgs{v.w, v.normalize ? v.mean : nullptr, v.normalize ? v.std : nullptr, v.clip, v.per_env ? 1 : 0, v.freeze ? 1 : 0, v.normalize ? 1 : 0, v.hidden};
}

int policy_call_begin(Handle *h, const char *name, int32_t T) {
    if (T <= 0) return h->fail(SRLHIP_EINVAL, std::string(name) + ": T must be positive");
    if (h->step_pending) return h->fail(SRLHIP_EINVAL, std::string(name) + ": a srlhip_step_async is pending (call srlhip_step_wait first)");
    return 0;
}

// summary: null, or the reduced outputs of srlhip_rollout_policy_summary (host's planes are all null then)
int rollout_policy(Handle *h, int32_t T, const PolicyCall &pc, const PolicyView &pv, const RolloutPlanes &host, const srlhip_rollout_summary *summary = nullptr) {
    const srlhip_config &c = h->cfg;
    Verdict v = check_policy_pointers(pv);
    if (!v.code) v = pc.sample && !pv.mlp ? check_rollout_policy_sampled_config(c) : check_rollout_policy_config(c, pc.sample);
    if (v.code) return refuse(h, pc.name, v);
    int rc = set_device(h);                            // (parks a resident kernel)
    if (rc) return rc;
    PolicyArgs pa = policy_args(pv);
    const size_t D = (size_t)obs_dim_of(c), wcount = policy_param_count(c, pv) * (pv.per_env ? (size_t)h->n : 1), elem = pv.mlp ? 4 : 8;
    RolloutPlanes dev = host;
    std::vector<double> packed;                        // host-pointer handles: [mean D][std D] doubles, then the parameters, one staged block
    if (!c.io_device) {
        if ((v = check_policy_values(pv, wcount, D)).code) return refuse(h, pc.name, v);
        packed.assign(2 * D + (elem * wcount + 7) / 8, 1.0);
        if (pa.normalize) { memcpy(packed.data(), pa.mean, 8 * D); memcpy(packed.data() + D, pa.std, 8 * D); }
        memcpy(packed.data() + 2 * D, pa.w, elem * wcount);
        if ((rc = stage_in(h, h->st[ST_RAND], packed.data(), 8 * packed.size()))) return rc;
        const double *blk = static_cast<const double *>(h->st[ST_RAND].p);
        pa.w = blk + 2 * D;
        if (pa.normalize) { pa.mean = blk; pa.std = blk + D; }
        if ((rc = stage_rollout_planes(h, T, dev))) return rc;
    }
    if (!summary) {
        if ((rc = env_ops(h).rollout_policy(h, T, pa, pc.sample, pc.kuka, dev.obs, dev.rew, dev.done, dev.act, nullptr))) return rc;
        return c.io_device ? 0 : fetch_rollout_planes(h, T, host, dev);      // (`packed` must outlive its copy: the synchronisation is in there)
    }
    // the reduced outputs.  Host-pointer handles: one staged block — ret [n], obs_sum [n][D], obs_sqsum [n][D] doubles, then length [n]
    const size_t n = (size_t)h->n;
    SummaryOut so = {summary->ret, summary->length, summary->obs_sum, summary->obs_sqsum};
    if (!c.io_device) {
        if ((rc = ensure(h, h->st[ST_OBS], 8 * n * (1 + 2 * D) + 4 * n))) return rc;
        double *blk = static_cast<double *>(h->st[ST_OBS].p);
        so = {blk, summary->length ? reinterpret_cast<int32_t *>(blk + n * (1 + 2 * D)) : nullptr, summary->obs_sum ? blk + n : nullptr,
              summary->obs_sum ? blk + n * (1 + D) : nullptr};
    }
    if ((rc = env_ops(h).rollout_policy(h, T, pa, pc.sample, pc.kuka, nullptr, nullptr, nullptr, nullptr, &so))) return rc;
    if (c.io_device) return 0;
    SRL_HIP_CHECK(h, hipMemcpyAsync(summary->ret, so.ret, 8 * n, hipMemcpyDeviceToHost, h->stream));
    if (so.length) SRL_HIP_CHECK(h, hipMemcpyAsync(summary->length, so.length, 4 * n, hipMemcpyDeviceToHost, h->stream));
    if (so.obs_sum) {
        SRL_HIP_CHECK(h, hipMemcpyAsync(summary->obs_sum, so.obs_sum, 8 * n * D, hipMemcpyDeviceToHost, h->stream));
        SRL_HIP_CHECK(h, hipMemcpyAsync(summary->obs_sqsum, so.obs_sqsum, 8 * n * D, hipMemcpyDeviceToHost, h->stream));
    }
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));      // (`packed` must outlive its copy)
    return 0;
}

// the four entry points: one body
template <class P>
int rollout_policy_entry(srlhip_handle hh, const PolicyCall &pc, int32_t T, const P *pol, const RolloutPlanes &host) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    Verdict v = check_policy_abi(pol);
    if (v.code) return refuse(h, pc.name, v);
    int rc = policy_call_begin(h, pc.name, T);
    if (rc) return rc;
    const PolicyView pv = policy_view(*pol);
    if ((v = check_policy_shape(pv)).code) return refuse(h, pc.name, v);
    return rollout_policy(h, T, pc, pv, host);
}
}  // namespace

extern "C" {

int srlhip_step(srlhip_handle hh, const void *actions, const double *host_noise, void *obs_out, float *reward_out,
                uint8_t *done_out) {
    if (!hh || !actions) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h, true);
    if (rc) return rc;
    if (h->cfg.rng_mode == SRLHIP_RNG_HOST && !host_noise)
        return h->fail(SRLHIP_EINVAL, "step: RNG_HOST needs host_noise");
    if (h->step_pending) return h->fail(SRLHIP_EINVAL, "step: a srlhip_step_async is pending (call srlhip_step_wait first)");
    if (!h->cfg.io_device) {
        if ((rc = host_step_begin(h, actions, host_noise, obs_out != nullptr))) return rc;
        return host_step_finish(h, obs_out, reward_out, done_out);
    }
    const bool pixels = h->cfg.obs_mode == SRLHIP_OBS_RAW_PIXELS;
    if ((rc = env_ops(h).step(h, actions, host_noise, pixels ? nullptr : obs_out, reward_out, done_out))) return rc;
    if (pixels && obs_out && (rc = raster_render(h, obs_out))) return rc;
    return 0;
}

int srlhip_step_async(srlhip_handle hh, const void *actions, const double *host_noise) {
    if (!hh || !actions) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (h->cfg.io_device) return h->fail(SRLHIP_EINVAL, "step_async: host-pointer handles only (on a device-pointer handle srlhip_step already only enqueues)");
    int rc = set_device(h, true);
    if (rc) return rc;
    if (h->cfg.rng_mode == SRLHIP_RNG_HOST && !host_noise) return h->fail(SRLHIP_EINVAL, "step_async: RNG_HOST needs host_noise");
    if (h->step_pending) return h->fail(SRLHIP_EINVAL, "step_async: the previous srlhip_step_async was not collected (srlhip_step_wait)");
    if ((rc = host_step_begin(h, actions, host_noise, true))) return rc;
    h->step_pending = true;
    return 0;
}

int srlhip_step_wait(srlhip_handle hh, void *obs_out, float *reward_out, uint8_t *done_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h->step_pending) return h->fail(SRLHIP_EINVAL, "step_wait: no srlhip_step_async is pending");
    int rc = set_device(h, true);
    if (rc) return rc;
    h->step_pending = false;
    return host_step_finish(h, obs_out, reward_out, done_out);
}

int srlhip_set_persistent(srlhip_handle hh, int32_t on, int32_t park_us) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (h->step_pending) return h->fail(SRLHIP_EINVAL, "set_persistent: a srlhip_step_async is pending");
    int rc = set_device(h);                            // (parks a resident kernel)
    if (rc) return rc;
    if (!on) { h->persist_on = false; persist_release(h); return 0; }
    if (h->cfg.io_device) return h->fail(SRLHIP_ENOTSUP, "set_persistent: host-pointer handles only");
    int capacity = 0, grid = 0;
    uint32_t eighths = 0;
    const int blocks = env_ops(h).persist_blocks(h, &capacity, &eighths, &grid);
    if (blocks <= 0 || !step_layout(h).zero_copy)
        return h->fail(SRLHIP_ENOTSUP, "set_persistent: needs a MobileRobot env, KukaButtonGymEnv, KukaMovingButtonGymEnv or Kuka2ButtonGymEnv (full model) on a device RNG mode, non-pixel "
                                       "observations, zero-copy step buffers, and a batch whose wavefronts are all resident at once (4096 envs on an MI355X)");
    if ((rc = ensure_signal_buffers(h))) return rc;
    if (!h->persist_stage) {
        const StepLayout L = step_layout(h);
        if ((rc = ensure_pinned(h, h->pin[PIN_IN], L.in_total)) || (rc = ensure_pinned(h, h->pin[PIN_OUT], L.out_total))) return rc;
        if (hipMalloc(&h->persist_stage, L.out_total + 16) != hipSuccess) return h->fail(SRLHIP_ENOMEM, "set_persistent: hipMalloc failed");
    }
    if (!h->persist_reserved) {
        std::lock_guard<std::mutex> lk(g_persist_mu);
        if (g_persist_reserved[h->cfg.device_id & 63] + grid > capacity)
            return h->fail(SRLHIP_ENOTSUP, "set_persistent: the resident kernels of the handles already in persistent mode on this device leave no room for this one");
        g_persist_reserved[h->cfg.device_id & 63] += grid;
        h->persist_reserved = grid;
    }
    h->persist_blocks = (uint32_t)blocks;
    h->persist_eighths = eighths;
    h->persist_park_us = park_us > 0 ? (uint32_t)park_us : 2000u;
    h->persist_on = true;
    return 0;
}

#if defined(SRL_PERSIST_PROF)
// timeline build only (profiles/probes/persist_timeline.py): parks the resident kernel and returns the 8 stamps of every workgroup's last step
int srlhip_debug_persist_prof(srlhip_handle hh, uint64_t *out, int32_t blocks) {
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    SRL_HIP_CHECK(h, hipMemcpy(out, h->persist_relay + kWordStamps, kStampsPerBlock * sizeof(uint64_t) * (size_t)blocks, hipMemcpyDeviceToHost));
    return 0;
}
#endif

int srlhip_step_pending(srlhip_handle hh) { return hh ? (reinterpret_cast<Handle *>(hh)->step_pending ? 1 : 0) : SRLHIP_EINVAL; }

int srlhip_rollout(srlhip_handle hh, int32_t T, const void *actions_TN, void *obs_TN, float *reward_TN,
                   uint8_t *done_TN, void *act_out_TN) {
    if (!hh || T <= 0) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    if (!h->cfg.auto_reset || h->cfg.rng_mode == SRLHIP_RNG_HOST)
        return h->fail(SRLHIP_EINVAL, "rollout: needs auto_reset and a device RNG mode");
    const size_t n = (size_t)h->n, tn = n * (size_t)T;
    const void *d_act = actions_TN;
    const RolloutPlanes host{obs_TN, reward_TN, done_TN, act_out_TN};
    RolloutPlanes dev = host;
    if (!h->cfg.io_device) {
        if (actions_TN && !h->cfg.is_discrete && !continuous_actions_ok(h->cfg, static_cast<const float *>(actions_TN), tn))
            return h->fail(SRLHIP_EINVAL, "rollout: non-finite continuous action (a Kuka env's `None` is a row of NaNs)");
        if (actions_TN) {                              // ST_ACTIONS holds the given plane: none is recorded (below), none comes back
            if ((rc = stage_in(h, h->st[ST_ACTIONS], actions_TN, action_bytes(h->cfg, tn)))) return rc;
            d_act = h->st[ST_ACTIONS].p; dev.act = nullptr;
        }
        if ((rc = stage_rollout_planes(h, T, dev))) return rc;
    }
    if (h->cfg.obs_mode != SRLHIP_OBS_RAW_PIXELS) {
        if ((rc = env_ops(h).rollout(h, T, d_act, dev.obs, dev.rew, dev.done, actions_TN ? nullptr : dev.act))) return rc;
    } else {
        // images are drawn between steps: one stepper launch + one rasteriser launch per step, same stream
        const size_t a_step = action_bytes(h->cfg, n), o_step = obs_bytes_per_env(h->cfg) * n;
        for (int32_t t = 0; t < T; t++) {
            const void *a_t = d_act ? static_cast<const uint8_t *>(d_act) + (size_t)t * a_step : nullptr;
            void *ao_t = (!actions_TN && dev.act) ? static_cast<uint8_t *>(dev.act) + (size_t)t * a_step : nullptr;
            float *r_t = dev.rew ? dev.rew + (size_t)t * n : nullptr;
            uint8_t *dn_t = dev.done ? dev.done + (size_t)t * n : nullptr;
            if ((rc = env_ops(h).rollout(h, 1, a_t, nullptr, r_t, dn_t, ao_t))) return rc;
            if (dev.obs && (rc = raster_render(h, static_cast<uint8_t *>(dev.obs) + (size_t)t * o_step))) return rc;
        }
    }
    return h->cfg.io_device ? 0 : fetch_rollout_planes(h, T, host, dev);
}

int srlhip_rollout_policy(srlhip_handle hh, int32_t T, const srlhip_linear_policy *pol, void *obs_TN, float *reward_TN,
                          uint8_t *done_TN, void *act_out_TN) {
    return rollout_policy_entry(hh, {"rollout_policy", kuka_rollout_policy}, T, pol, {obs_TN, reward_TN, done_TN, act_out_TN});
}

int srlhip_rollout_policy_sampled(srlhip_handle hh, int32_t T, const srlhip_linear_policy *pol, void *obs_TN, float *reward_TN,
                                  uint8_t *done_TN, void *act_out_TN) {
    return rollout_policy_entry(hh, {"rollout_policy_sampled", kuka_rollout_policy_sampled, true}, T, pol, {obs_TN, reward_TN, done_TN, act_out_TN});
}

int srlhip_rollout_mlp_policy(srlhip_handle hh, int32_t T, const srlhip_mlp_policy *pol, void *obs_TN, float *reward_TN,
                              uint8_t *done_TN, void *act_out_TN) {
    return rollout_policy_entry(hh, {"rollout_mlp_policy", kuka_rollout_mlp_policy}, T, pol, {obs_TN, reward_TN, done_TN, act_out_TN});
}

int srlhip_rollout_mlp_policy_sampled(srlhip_handle hh, int32_t T, const srlhip_mlp_policy *pol, void *obs_TN, float *reward_TN,
                                      uint8_t *done_TN, void *act_out_TN) {
    return rollout_policy_entry(hh, {"rollout_mlp_policy_sampled", kuka_rollout_mlp_policy_sampled, true}, T, pol, {obs_TN, reward_TN, done_TN, act_out_TN});
}

// srlhip_rollout_policy_summary: the plane call the arguments name (its PolicyCall: the Kuka launcher, `sample`) behind the plane calls'
// checks in their order, the new arguments' checks (api_rules.hpp: check_rollout_summary) right behind the ABI checks
int srlhip_rollout_policy_summary(srlhip_handle hh, int32_t T, const srlhip_linear_policy *linear, const srlhip_mlp_policy *mlp, int32_t sample,
                                  const srlhip_rollout_summary *out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    const char *name = kSummaryName;
    Verdict v = check_policy_act_which(linear != nullptr, mlp != nullptr);
    if (!v.code) v = mlp ? check_policy_abi(mlp) : check_policy_abi(linear);
    if (!v.code) v = check_rollout_summary(out);
    if (v.code) return refuse(h, name, v);
    int rc = policy_call_begin(h, name, T);
    if (rc) return rc;
    const PolicyView pv = mlp ? policy_view(*mlp) : policy_view(*linear);
    if ((v = check_policy_shape(pv)).code) return refuse(h, name, v);
    const KukaPolicyLaunch kuka = mlp ? (sample ? kuka_rollout_mlp_policy_sampled : kuka_rollout_mlp_policy) : (sample ? kuka_rollout_policy_sampled : kuka_rollout_policy);
    return rollout_policy(h, T, {name, kuka, sample != 0}, pv, RolloutPlanes{}, out);
}

// srlhip_policy_act: the struct checks and messages of the fused rollouts in their order, its own argument checks between them, none
// of the rollouts' refusals by env kind or observation mode — the call never looks at the env state
int srlhip_policy_act(srlhip_handle hh, const srlhip_linear_policy *linear, const srlhip_mlp_policy *mlp, int32_t sample, const float *obs,
                      int32_t obs_dim, const uint8_t *done_prev, uint8_t *frozen, void *act_out, double *score_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    const char *name = "policy_act";
    Verdict v = check_policy_act_which(linear != nullptr, mlp != nullptr);
    if (!v.code) v = mlp ? check_policy_abi(mlp) : check_policy_abi(linear);
    if (v.code) return refuse(h, name, v);
    int rc = policy_call_begin(h, name, 1);
    if (rc) return rc;
    const PolicyView pv = mlp ? policy_view(*mlp) : policy_view(*linear);
    const srlhip_config &c = h->cfg;
    v = check_policy_shape(pv);
    if (!v.code) v = check_policy_act_shape(obs_dim, sample != 0, pv.mlp);
    if (!v.code) v = check_policy_pointers(pv);
    if (!v.code) v = check_policy_act_planes(c, pv, sample != 0, obs != nullptr, act_out != nullptr, frozen != nullptr);
    if (v.code) return refuse(h, name, v);
    if ((rc = set_device(h))) return rc;               // (parks a resident kernel)
    // none_nan: a frozen env's continuous row is the family's `None` — NaNs for Kuka, zeros for MobileRobot
    return policy_act_launch(h, policy_args(pv), sample != 0, obs_dim, (int)policy_outputs(c), !is_mobile(c.env_kind), obs, done_prev, frozen, act_out, score_out);
}

// srlhip_sample_actions: a pending step, then the planes and the config (api_rules.hpp: check_sample_actions)
int srlhip_sample_actions(srlhip_handle hh, const double *scores, const uint8_t *frozen, int32_t *act_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    const char *name = "sample_actions";
    int rc = policy_call_begin(h, name, 1);
    if (rc) return rc;
    const srlhip_config &c = h->cfg;
    const Verdict v = check_sample_actions(c, scores != nullptr, act_out != nullptr);
    if (v.code) return refuse(h, name, v);
    if ((rc = set_device(h))) return rc;               // (parks a resident kernel)
    return sample_actions_launch(h, num_actions_of(c), scores, frozen, act_out);
}

// srlhip_cnn_policy_act: the struct, a pending step, then the planes and the config (api_rules.hpp: check_cnn_policy_abi, check_cnn_policy_act)
int srlhip_cnn_policy_act(srlhip_handle hh, const srlhip_cnn_policy *pol, int32_t sample, const uint8_t *images, const uint8_t *done_prev,
                          uint8_t *frozen, void *act_out, float *score_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    const char *name = "cnn_policy_act";
    Verdict v = check_cnn_policy_abi(pol);
    if (v.code) return refuse(h, name, v);
    int rc = policy_call_begin(h, name, 1);
    if (rc) return rc;
    const srlhip_config &c = h->cfg;
    v = check_cnn_policy_act(c, pol->freeze_after_done != 0, sample != 0, images != nullptr, act_out != nullptr, frozen != nullptr);
    if (v.code) return refuse(h, name, v);
    if ((rc = set_device(h))) return rc;               // (parks a resident kernel)
    return cnn_policy_act_launch(h, pol->params, pol->per_env != 0, pol->freeze_after_done != 0, sample != 0, (int)policy_outputs(c), !is_mobile(c.env_kind),
                                 images, done_prev, frozen, act_out, score_out);
}

// srlhip_pixel_policy_act: the struct, a pending step, then the planes and the config (api_rules.hpp: check_pixel_policy_abi, check_pixel_policy_act)
int srlhip_pixel_policy_act(srlhip_handle hh, const srlhip_pixel_policy *pol, const uint8_t *images, const uint8_t *done_prev, uint8_t *frozen,
                            void *act_out, double *score_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    const char *name = "pixel_policy_act";
    Verdict v = check_pixel_policy_abi(pol);
    if (v.code) return refuse(h, name, v);
    int rc = policy_call_begin(h, name, 1);
    if (rc) return rc;
    const srlhip_config &c = h->cfg;
    v = check_pixel_policy_act(c, pol->paired != 0, pol->freeze_after_done != 0, images != nullptr, act_out != nullptr, frozen != nullptr);
    if (v.code) return refuse(h, name, v);
    if ((rc = set_device(h))) return rc;               // (parks a resident kernel)
    return pixel_policy_act_launch(h, pol->weights, pol->delta, pol->noise, pol->paired != 0, pol->freeze_after_done != 0, (int)policy_outputs(c),
                                   !is_mobile(c.env_kind), images, done_prev, frozen, act_out, score_out);
}

int64_t srlhip_cnn_param_count(int32_t channels, int32_t img_h, int32_t img_w, int32_t outputs) {
    if ((channels != 3 && channels != 6) || !cnn_side_ok(img_h) || !cnn_side_ok(img_w) || outputs < 1 || outputs > 8) return 0;
    return (int64_t)cnn_param_count(channels, img_h, img_w, outputs);
}

int srlhip_get_state(srlhip_handle hh, int32_t field, void *out) {
    if (!hh || !out) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    void *d; size_t elem; int count;
    if ((rc = field_lookup(h, field, &d, &elem, &count))) return rc;
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (h->ep_host && (field == SRLHIP_F_LAST_RETURN || field == SRLHIP_F_LAST_LENGTH)) {        // mapped host block (create)
        memcpy(out, field == SRLHIP_F_LAST_LENGTH ? (const void *)episode_lengths(h->ep_host, (size_t)h->n) : episode_returns(h->ep_host), elem * (size_t)h->n);
        return 0;
    }
    SRL_HIP_CHECK(h, hipMemcpy(out, d, elem * count * (size_t)h->n, hipMemcpyDeviceToHost));
    return 0;
}

int srlhip_set_state(srlhip_handle hh, int32_t field, const void *in) {
    if (!hh || !in) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    void *d; size_t elem; int count;
    if ((rc = field_lookup(h, field, &d, &elem, &count))) return rc;
    h->snap_valid = false;                 // (MobileRobot: the rollout's chained snapshot no longer equals the live state)
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (h->ep_host && (field == SRLHIP_F_LAST_RETURN || field == SRLHIP_F_LAST_LENGTH)) {
        memcpy(field == SRLHIP_F_LAST_LENGTH ? (void *)episode_lengths(h->ep_host, (size_t)h->n) : episode_returns(h->ep_host), in, elem * (size_t)h->n);
        return 0;
    }
    SRL_HIP_CHECK(h, hipMemcpy(d, in, elem * count * (size_t)h->n, hipMemcpyHostToDevice));
    if (field == SRLHIP_F_KUKA_Q || field == SRLHIP_F_KUKA_GRIPPER_Q) return kuka_refresh(h);        // derived planes: sin/cos of q, gripper position
    return 0;
}

int srlhip_device_ptr(srlhip_handle hh, int32_t field, void **dptr) {
    if (!hh || !dptr) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    size_t elem; int count;
    return field_lookup(h, field, dptr, &elem, &count);
}

int srlhip_render(srlhip_handle hh, void *img_out) {
    if (!hh || !img_out) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    const size_t bytes = frame_bytes(h->cfg) * h->n;
    void *d_img = img_out;
    if (!h->cfg.io_device) { if ((rc = ensure(h, h->st[ST_OBS], bytes))) return rc; d_img = h->st[ST_OBS].p; }
    if ((rc = raster_render(h, d_img))) return rc;
    if (!h->cfg.io_device) {
        SRL_HIP_CHECK(h, hipMemcpyAsync(img_out, d_img, bytes, hipMemcpyDeviceToHost, h->stream));
        SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

int srlhip_render_jpeg(srlhip_handle hh, int32_t quality, void *blob_out, int64_t blob_cap, int64_t *offsets_out, int32_t *overflow_out) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!blob_out || !offsets_out || !overflow_out || blob_cap < 0) return h->fail(SRLHIP_EINVAL, "render_jpeg: null buffer");
    if (quality < 1 || quality > 100) return h->fail(SRLHIP_EINVAL, "render_jpeg: quality must be in 1..100");
    if (h->step_pending) return h->fail(SRLHIP_EINVAL, "render_jpeg: a srlhip_step_async is pending (call srlhip_step_wait first)");
    int rc = set_device(h);                            // (parks a resident kernel)
    if (rc) return rc;
    const JpegScratch S = jpeg_scratch(h->cfg, (size_t)h->n, blob_cap);
    const size_t ns = S.ns;
    if ((rc = ensure(h, h->st[ST_JPEG], S.bytes(h->cfg.io_device != 0)))) return rc;
    uint8_t *d = static_cast<uint8_t *>(h->st[ST_JPEG].p);
    if ((rc = raster_render(h, d))) return rc;
    uint8_t *d_blob = h->cfg.io_device ? static_cast<uint8_t *>(blob_out) : d + S.blob_at;
    int64_t *d_off = h->cfg.io_device ? offsets_out : reinterpret_cast<int64_t *>(d + S.off_at);
    int32_t *d_ovf = h->cfg.io_device ? overflow_out : reinterpret_cast<int32_t *>(d + S.ovf_at);
    if ((rc = jpeg_encode_launch(d, h->n, h->cfg.img_h, h->cfg.img_w, S.ch, quality, d_blob, S.cap, d_off, d_ovf, h->stream)))
        return h->fail(rc, "render_jpeg: frames of 8..1024 pixels a side only, or the launch failed");
    if (!h->cfg.io_device) {
        SRL_HIP_CHECK(h, hipMemcpyAsync(offsets_out, d_off, 8 * (ns + 1), hipMemcpyDeviceToHost, h->stream));
        SRL_HIP_CHECK(h, hipMemcpyAsync(overflow_out, d_ovf, 4 * ns, hipMemcpyDeviceToHost, h->stream));
        SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
        const int64_t used = offsets_out[ns];
        if (used < 0 || used > blob_cap) return h->fail(SRLHIP_EHIP, "render_jpeg: the encoder reported an impossible size");
        if (used) SRL_HIP_CHECK(h, hipMemcpy(blob_out, d_blob, (size_t)used, hipMemcpyDeviceToHost));
    }
    return 0;
}

int srlhip_episode_stats(srlhip_handle hh, double *last_return, int32_t *last_length, int32_t *n_finished) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->n;
    if (h->ep_host) {          // host-pointer handle: the records already are in host memory
        if (last_return) memcpy(last_return, episode_returns(h->ep_host), 8 * n);
        if (last_length) memcpy(last_length, episode_lengths(h->ep_host, n), 4 * n);
    } else {
        if (last_return) SRL_HIP_CHECK(h, hipMemcpy(last_return, h->stats.last_return, 8 * n, hipMemcpyDeviceToHost));
        if (last_length) SRL_HIP_CHECK(h, hipMemcpy(last_length, h->stats.last_length, 4 * n, hipMemcpyDeviceToHost));
    }
    if (n_finished) SRL_HIP_CHECK(h, hipMemcpy(n_finished, h->stats.n_finished, 4 * n, hipMemcpyDeviceToHost));
    return 0;
}

int srlhip_episode_records(srlhip_handle hh, const double **last_return, const int32_t **last_length) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h->ep_host) return h->fail(SRLHIP_EINVAL, "episode_records: host-pointer handles only (cfg.io_device = 0); device-pointer handles use srlhip_episode_stats_device");
    if (last_return) *last_return = episode_returns(h->ep_host);
    if (last_length) *last_length = episode_lengths(h->ep_host, (size_t)h->n);
    return 0;
}

int srlhip_episode_stats_device(srlhip_handle hh, float *d_last_return, int32_t *d_last_length, int32_t *d_n_finished) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    hipLaunchKernelGGL(episode_stats_k, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->stats, h->n, d_last_return,
                       d_last_length, d_n_finished);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

int srlhip_kuka_default_model(srlhip_kuka_model *m) {
    if (!m) return SRLHIP_EINVAL;
    kuka_default_model(reinterpret_cast<double *>(m));
    return 0;
}

int srlhip_set_kuka_model(srlhip_handle hh, const srlhip_kuka_model *m) {
    if (!hh || !m) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (is_mobile(h->cfg.env_kind)) return h->fail(SRLHIP_EINVAL, "set_kuka_model: not a Kuka handle");
    int rc = set_device(h);
    if (rc) return rc;
    if (const Verdict v = check_kuka_model(*m); v.code) return h->fail(v.code, v.msg);
    return kuka_set_model(h, reinterpret_cast<const double *>(m));
}

int srlhip_kuka_tree_default_model(srlhip_kuka_tree_model *m) {
    if (!m) return SRLHIP_EINVAL;
    kuka_default_tree_model(reinterpret_cast<double *>(m));
    return 0;
}

int srlhip_set_kuka_tree_model(srlhip_handle hh, const srlhip_kuka_tree_model *m) {
    if (!hh || !m) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (is_mobile(h->cfg.env_kind)) return h->fail(SRLHIP_EINVAL, "set_kuka_tree_model: not a Kuka handle");
    if (h->cfg.kuka_model != SRLHIP_KUKA_MODEL_FULL) return h->fail(SRLHIP_EINVAL, "set_kuka_tree_model: the handle was created with the lumped model");
    if (const Verdict v = check_kuka_tree_model(*m); v.code) return h->fail(v.code, v.msg);
    return kuka_set_tree_model(h, reinterpret_cast<const double *>(m));
}

int srlhip_kuka_kernel(srlhip_handle hh) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (is_mobile(h->cfg.env_kind)) return SRLHIP_EINVAL;
    return kuka_uses_group_kernel(h);
}

int srlhip_selftest_group_primitives(int32_t device_id, const double *q7, double *out, int32_t out_doubles) {
    if (!q7 || !out) return SRLHIP_EINVAL;
    if (hipSetDevice(device_id) != hipSuccess) return SRLHIP_EHIP;
    return kuka_group_probe(q7, out, out_doubles);
}

int srlhip_selftest_rng(int32_t device_id, int32_t generator, int32_t stream, int32_t n_envs, int32_t stride, const uint32_t *keys,
                        const int32_t *key_len, const uint8_t *mask, const uint64_t *state_in, const int32_t *script, int32_t n_ops,
                        const double *args, int32_t n_args, const int32_t *skip, uint64_t *out, int64_t out_words, uint64_t *state_out,
                        int64_t state_words) {
    if (hipSetDevice(device_id) != hipSuccess) return SRLHIP_EHIP;
    return rng_probe_run(generator, stream, n_envs, stride, keys, key_len, mask, state_in, script, n_ops, args, n_args, skip, out, out_words,
                         state_out, state_words);
}

int srlhip_sync(srlhip_handle hh) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int srlhip_copy_async(srlhip_handle hh, void *dst, const void *src, size_t bytes) {
    if (!hh || (bytes && (!dst || !src))) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    int rc = set_device(h);
    if (rc) return rc;
    if (bytes) SRL_HIP_CHECK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
    return 0;
}

int srlhip_stream(srlhip_handle hh, void **hip_stream) {
    if (!hh || !hip_stream) return SRLHIP_EINVAL;
    *hip_stream = reinterpret_cast<Handle *>(hh)->stream;
    return 0;
}

// ---- HIP graphs: capture whatever the caller enqueues on the handle's stream between begin and end (device-pointer
// calls of this library, srlhip_encoder_forward on the same stream, ...) and replay it with one launch per step.
struct srlhip_graph { hipGraph_t graph; hipGraphExec_t exec; };

int srlhip_graph_begin(srlhip_handle hh) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h->cfg.io_device) return h->fail(SRLHIP_EINVAL, "graph capture needs io_device = 1 (host-pointer calls synchronise)");
    int rc = set_device(h);
    if (rc) return rc;
    h->prefetch_valid = false;             // a captured synthetic-agent rollout moves the action-stream counters on the device at every replay
    h->snap_valid = false;
    SRL_HIP_CHECK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    return 0;
}

int srlhip_graph_end(srlhip_handle hh, srlhip_graph_handle *out) {
    if (!hh || !out) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    *out = nullptr;
    hipGraph_t g = nullptr;
    SRL_HIP_CHECK(h, hipStreamEndCapture(h->stream, &g));
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return h->fail(SRLHIP_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    }
    srlhip_graph *sg = new (std::nothrow) srlhip_graph();
    if (!sg) { (void)hipGraphExecDestroy(ex); (void)hipGraphDestroy(g); return h->fail(SRLHIP_ENOMEM, "graph handle"); }
    sg->graph = g; sg->exec = ex;
    *out = sg;
    return 0;
}

int srlhip_graph_launch(srlhip_handle hh, srlhip_graph_handle g) {
    if (!hh || !g) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    h->prefetch_valid = false;             // (see srlhip_graph_begin: the action plane drawn ahead belongs to counters the replay has consumed)
    h->snap_valid = false;                 // ... and the replay moved the live state
    SRL_HIP_CHECK(h, hipGraphLaunch(g->exec, h->stream));
    return 0;
}

int srlhip_graph_destroy(srlhip_graph_handle g) {
    if (!g) return SRLHIP_OK;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return SRLHIP_OK;
}

int srlhip_timing_begin(srlhip_handle hh) {
    if (!hh) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    SRL_HIP_CHECK(h, hipEventRecord(h->ev_begin, h->stream));
    return 0;
}

int srlhip_timing_end(srlhip_handle hh, float *elapsed_ms) {
    if (!hh || !elapsed_ms) return SRLHIP_EINVAL;
    Handle *h = reinterpret_cast<Handle *>(hh);
    SRL_HIP_CHECK(h, hipEventRecord(h->ev_end, h->stream));
    SRL_HIP_CHECK(h, hipEventSynchronize(h->ev_end));
    SRL_HIP_CHECK(h, hipEventElapsedTime(elapsed_ms, h->ev_begin, h->ev_end));
    return 0;
}

}  // extern "C"
