// mobile.hip — the MobileRobot family (MobileRobotGymEnv, 1D, 2Target, LineTarget) for gfx950 (MI355X).
//
// Replaces, for a whole batch of envs per launch:
//   reset   mobile_robot_env.py:159-222 (+ variants: 1D :58-74, 2Target :35-67, LineTarget :56-64) — only the RNG draws and the
//           state init; every pybullet call on this path is scene loading / rendering.
//   step    mobile_robot_env.py:235-280, _reward :345-363, _termination :336-343
//           (2Target reward :162-181, LineTarget reward :108-125, 1D step :108-147)
//
// One lane per env, structure-of-arrays state (env index fastest: a wavefront's 64 loads / stores of a field are one coalesced
// 512-byte row).  Arithmetic is float64 with -ffp-contract=off, the reference's numpy f64; the only fused op is the explicit fma
// chain of np.linalg.norm's ddot (step_env).  ~40 flops per env-step, no LDS, no MFMA: every kernel here is bound by launch and
// memory latency or by the issue stream of one wavefront's recurrence (measurements: profiles/NOTES.md sections I, Y, AD, AE, AM).
//
// One definition each of reset_env / step_env / observe (the env), EpisodeLane (Monitor's accounting), store_step (an output row),
// gather_actions (actions from a plane) and policy_input / policy_action (a policy's action) serves every kernel below:
//
//   kernel                    actions come from                          RNG modes            entry point
//   mobile_reset_k            —                                          host, Philox, MT     srlhip_reset
//   mobile_sample_actions_k   (draws the synthetic agent's [T][N] plane, Philox stream 1 of the env, in every device RNG mode)
//   mobile_rollout_k          a [T][N] plane: the caller's or sampled    host (T = 1), Philox, MT   srlhip_step, srlhip_rollout
//   mobile_rollout_ep_k       the same plane, episodes on separate lanes Philox + auto_reset, T >= 32   srlhip_rollout
//   mobile_rollout_policy_k   a linear policy of the env's observation   Philox, MT           srlhip_rollout_policy
//   mobile_rollout_mlp_k      a one-hidden-layer MLP of it, 16 lanes/env Philox, MT           srlhip_rollout_mlp_policy
//   mobile_rollout_mlp_k<.., SAMPLE>  the same, action drawn from its softmax  Philox, MT        srlhip_rollout_mlp_policy_sampled
//   mobile_rollout_policy_k<.., SAMPLE>  the linear policy, action drawn from its softmax  Philox, MT  srlhip_rollout_policy_sampled
//   mobile_persist_k          the host's mapped plane, one step per token Philox, MT          srlhip_set_persistent + srlhip_step
//
// Bit identity (all of it tested): mobile_rollout_k is oracle/mobile_oracle.c, step for step, in every RNG mode.
// mobile_rollout_ep_k leaves the outputs, final state, counters and episode fields mobile_rollout_k leaves for the same plane.
// The two policy kernels replayed through mobile_rollout_k with their recorded actions as a given plane reproduce themselves, and
// their scores are numpy's float64 expressions (tests/policy_exact.py).  mobile_persist_k is T = 1 launches of mobile_rollout_k.
// A T-step launch equals T single-step launches, episode fields included (tests/test_gpu_mobile_episode_fields.py).
#include <type_traits>

#include "internal.hpp"
#include "policy_act.hpp"

namespace srl {

namespace {
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;

// np.linalg.norm(v, 2) == sqrt(ddot(v, v)); OpenBLAS accumulates with FMA: see step_env.

struct MobileEnv {
    double x, y, tx, ty, t2x, t2y;
    int32_t counter, cur;
};

__device__ __forceinline__ void load_env(const MobileState &s, int e, MobileEnv &m) {
    m.x = s.pos_x[e]; m.y = s.pos_y[e]; m.tx = s.tgt_x[e]; m.ty = s.tgt_y[e];
    m.t2x = s.tgt2_x[e]; m.t2y = s.tgt2_y[e]; m.counter = s.counter[e]; m.cur = s.cur_target[e];
}
__device__ __forceinline__ void store_env(const MobileState &s, int e, const MobileEnv &m) {
    s.pos_x[e] = m.x; s.pos_y[e] = m.y; s.tgt_x[e] = m.tx; s.tgt_y[e] = m.ty;
    s.tgt2_x[e] = m.t2x; s.tgt2_y[e] = m.t2y; s.counter[e] = m.counter; s.cur_target[e] = m.cur;
}

// Random sources ---------------------------------------------------------------
struct HostRng {                 // SRLHIP_RNG_HOST: caller pre-drew everything
    const double *rand; int i; double noise;
    __device__ double uniform(double, double) { return rand[i++]; }
    __device__ double normal(double, double) { return noise; }
};
struct PhiloxRng {               // SRLHIP_RNG_PHILOX
    Philox p;
    __device__ double uniform(double lo, double hi) { return p.uniform(lo, hi); }
    // scale == 0 draws nothing: counter streams need no alignment with numpy
    __device__ double normal(double loc, double scale) { return scale == 0.0 ? loc : p.normal(loc, scale); }
};
struct MtRng {                   // SRLHIP_RNG_MT19937: np_random itself
    Mt19937 m;
    __device__ double uniform(double lo, double hi) { return m.uniform(lo, hi); }
    __device__ double normal(double loc, double scale) { return m.normal(loc, scale); }
};

template <int MODE> struct RngSel;
template <> struct RngSel<SRLHIP_RNG_HOST> { using type = HostRng; };
template <> struct RngSel<SRLHIP_RNG_PHILOX> { using type = PhiloxRng; };
template <> struct RngSel<SRLHIP_RNG_MT19937> { using type = MtRng; };

template <int MODE>
__device__ __forceinline__ void rng_load(typename RngSel<MODE>::type &r, const RngState &rs, int e, int n,
                                         const double *host_rand, int rand_stride, const double *noise) {
    if constexpr (MODE == SRLHIP_RNG_HOST) {
        r.rand = host_rand ? host_rand + (int64_t)e * rand_stride : nullptr;
        r.i = 0;
        r.noise = noise ? noise[e] : 0.0;
    } else if constexpr (MODE == SRLHIP_RNG_PHILOX) {
        r.p.k0 = rs.key[e]; r.p.k1 = rs.key[n + e]; r.p.ctr = rs.ctr[e]; r.p.stream = 0;
    } else {
        r.m.load(rs.mt, e);
    }
}
template <int MODE>
__device__ __forceinline__ void rng_store(const typename RngSel<MODE>::type &r, const RngState &rs, int e) {
    if constexpr (MODE == SRLHIP_RNG_PHILOX) rs.ctr[e] = r.p.ctr;
    else if constexpr (MODE == SRLHIP_RNG_MT19937) r.m.store(rs.mt, e);
}

// reset: mobile_robot_env.py:166-181 and the variant overrides -------------------
template <class R>
__device__ __forceinline__ void reset_env(const MobileParams &p, R &rng, MobileEnv &m) {
    const double max_x = 4.0, max_y = 4.0;
    m.cur = 0;
    m.x = max_x / 2 + rng.uniform(-max_x / 3, max_x / 3);
    m.y = 0.0;
    if (p.kind != SRLHIP_ENV_MOBILE_1D) m.y = max_y / 2 + rng.uniform(-max_y / 3, max_y / 3);
    const double margin = 0.1 * max_x;
    m.tx = 0.9 * max_x; m.ty = 0.0; m.t2x = 0.0; m.t2y = 0.0;
    if (p.kind == SRLHIP_ENV_MOBILE_1D) {
        if (p.random_target) m.tx = rng.uniform(0 + margin, max_x - margin);
    } else if (p.kind == SRLHIP_ENV_MOBILE_LINE) {
        if (p.random_target) m.tx = rng.uniform(0 + margin, max_x - margin);
        m.ty = max_x;
    } else {
        m.ty = max_y * 3 / 4;
        if (p.random_target) {
            m.tx = rng.uniform(0 + margin, max_x - margin);
            m.ty = rng.uniform(0 + margin, max_y - margin);
        }
        if (p.kind == SRLHIP_ENV_MOBILE_2TARGET) {
            m.t2x = 0.1 * max_x; m.t2y = max_y * 3 / 4;
            if (p.random_target) {
                m.t2x = rng.uniform(0 + margin, max_x - margin);
                m.t2y = rng.uniform(0 + margin, max_y - margin);
            }
        }
    }
    m.counter = 0;
}

// getSRLState for ground_truth: getGroundTruth() - getTargetPos() (srl_env.py:39-42)
__device__ __forceinline__ void observe(const MobileParams &p, const MobileEnv &m, float &o0, float &o1) {
    double tx = m.cur ? m.t2x : m.tx, ty = m.cur ? m.t2y : m.ty;
    if (p.kind == SRLHIP_ENV_MOBILE_LINE) {          // 1-vector target broadcast over (x, y)
        double t = tx - 0.2;
        o0 = (float)(m.x - t); o1 = (float)(m.y - t);
    } else {
        o0 = (float)(m.x - tx); o1 = (float)(m.y - ty);
    }
}

// step: mobile_robot_env.py:235-280 --------------------------------------------
// KIND / DISC / SHAPE >= 0: env kind / action type / shaped reward known at compile time (rollout kernels); -1: read from the params.
// (SHAPE matters: with a run-time flag the compiler evaluates the shaped reward's float64 square root — a reciprocal-square-root
//  estimate and ten dependent FMAs — in every step and selects afterwards.)
template <int KIND = -1, int DISC = -1, int SHAPE = -1>
__device__ __forceinline__ void step_env(const MobileParams &pp, MobileEnv &m, int a, float a0, float a1, double dv,
                                         double &reward, bool &done) {
    struct { int32_t kind, is_discrete, shape_reward; } p = {KIND >= 0 ? KIND : pp.kind, DISC >= 0 ? DISC : pp.is_discrete,
                                                             SHAPE >= 0 ? SHAPE : pp.shape_reward};
    double dx = 0.0, dy = 0.0;
    if (p.is_discrete) {
        if (p.kind == SRLHIP_ENV_MOBILE_1D) {
            dx = a == 0 ? -dv : a == 1 ? dv : 0.0;
        } else {
            dx = a == 0 ? -dv : a == 1 ? dv : 0.0;
            dy = a == 2 ? -dv : a == 3 ? dv : 0.0;
        }
    } else {
        // float32 Box action * python-float dv: numpy keeps float32 (value-based casting)
        float fdv = (float)dv;
        dx = (double)(fmaxf(fminf(a0, 1.0f), -1.0f) * fdv);
        dy = (double)(fmaxf(fminf(a1, 1.0f), -1.0f) * fdv);
    }
    const double px = m.x, py = m.y;
    m.x = m.x + dx;
    if (p.kind != SRLHIP_ENV_MOBILE_1D) m.y = m.y + dy;
    // collision with the arena walls: x first, `break` on the first violation
    const double margin_x = 0.1 + (0.325 * 2) / 2, margin_y = 0.1 + 0.2 / 2;
    bool bumped = false;
    if (m.x < margin_x || m.x > 4 - margin_x) {
        bumped = true;
    } else if (p.kind != SRLHIP_ENV_MOBILE_1D && (m.y < margin_y || m.y > 4 - margin_y)) {
        bumped = true;
    }
    if (bumped) { m.x = px; m.y = py; }
    m.counter += 1;
    // _reward
    double tx = m.cur ? m.t2x : m.tx, ty = m.cur ? m.t2y : m.ty;
    double distance = 0.0;
    bool within;
    if (p.kind == SRLHIP_ENV_MOBILE_LINE) {
        distance = fabs((tx - 0.2) - m.x);
        within = distance <= 0.1;
    } else {
        // np.linalg.norm = sqrt(ddot): sqrt is correctly rounded and monotonic, so `sqrt(s2) <= 0.4` holds exactly when
        // s2 <= the largest double whose rounded square root is <= 0.4.  The sparse reward only needs that predicate;
        // the square root itself (a ~25-instruction dependent chain in f64) is taken only for the shaped reward.
        constexpr double kSqMax04 = 0x1.47ae147ae147cp-3;
        const double ex = tx - m.x, ey = ty - m.y;
        const double s2 = p.kind == SRLHIP_ENV_MOBILE_1D ? fma(ex, ex, 0.0) : fma(ey, ey, fma(ex, ex, 0.0));
        if (p.shape_reward) { distance = sqrt(s2); within = distance <= 0.4; }
        else within = s2 <= kSqMax04;
    }
    reward = 0.0;
    if (within) {
        reward = 1.0;
        if (p.kind == SRLHIP_ENV_MOBILE_2TARGET && m.cur < 1) m.cur += 1;
    }
    if (bumped) reward = -1.0;
    if (p.shape_reward) reward = -distance;
    done = m.counter > 250;                           // terminated is never set (:336-343)
}

// Register copy of one env's episode accounting (EpisodeStats: bench.Monitor) for the length of a launch.  What follows an ended
// episode — a reset, a frozen policy — stays with the caller.
struct EpisodeLane {
    double ep_ret = 0.0, last_ret = 0.0, last_reward = 0.0;
    int32_t ep_len = 0, last_len = 0, n_fin = 0, n_fin0 = 0;
    __device__ __forceinline__ void load(const EpisodeStats &st, int e) {
        ep_ret = st.ep_return[e]; ep_len = st.ep_length[e]; n_fin = n_fin0 = st.n_finished[e];
    }
    __device__ __forceinline__ void add(double reward) { ep_ret += reward; ep_len += 1; last_reward = reward; }     // a step that ends no episode
    // a step; on_end() — the caller's reset, its frozen flag — runs inside the branch that closes the episode.  (One branch: with a
    // returned flag and a second `if` at the call site, mobile_rollout_k's 16-step chunks were unrolled by 8 only and their action
    // arrays went to scratch — profiles/NOTES.md section AM.)
    template <class F>
    __device__ __forceinline__ void step(double reward, bool done, F &&on_end) {
        add(reward);
        if (done) { last_ret = ep_ret; last_len = ep_len; n_fin += 1; ep_ret = 0.0; ep_len = 0; on_end(); }
    }
    __device__ __forceinline__ bool ended() const { return n_fin != n_fin0; }     // an episode ended since load()
    // Monitor's record at system scope, for a host that reads it while the launch is still running (the step signal, the resident kernel)
    __device__ __forceinline__ void publish(const EpisodeStats &st, int e) const {
        __hip_atomic_store(st.last_return + e, last_ret, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(st.last_length + e, last_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // Monitor's record of the last finished episode (last_return, last_length) is written only when an episode ended in this launch
    // and is never read: on host-pointer handles those two planes are mapped host memory — srlhip_episode_records — and a read or an
    // unconditional write-back would cross PCIe in every launch.  LAST = false: the caller has publish()ed every record already.
    template <bool LAST = true>
    __device__ __forceinline__ void store(const EpisodeStats &st, int e) const {
        st.ep_return[e] = ep_ret; st.ep_length[e] = ep_len;
        if (LAST && ended()) { st.last_return[e] = last_ret; st.last_length[e] = last_len; }
        st.n_finished[e] = n_fin; st.last_reward[e] = last_reward;
    }
};

// One row of the streamed [T][n] output planes: the observation (1D: one float, otherwise one 8-byte store per lane — a wavefront's row
// is 512 contiguous bytes), the reward, done.  CHECKED: a null plane is skipped.
template <bool CHECKED>
__device__ __forceinline__ void store_step(const MobileParams &p, int64_t row, float o0, float o1, double reward, bool done,
                                           float *__restrict__ obs, float *__restrict__ rew, uint8_t *__restrict__ done_out) {
    if (!CHECKED || obs) {
        if (p.kind == SRLHIP_ENV_MOBILE_1D) __builtin_nontemporal_store(o0, obs + row);
        else __builtin_nontemporal_store(f32x2{o0, o1}, reinterpret_cast<f32x2 *>(obs + 2 * row));
    }
    if (!CHECKED || rew) __builtin_nontemporal_store((float)reward, rew + row);
    if (!CHECKED || done_out) __builtin_nontemporal_store((uint8_t)done, done_out + row);
}

template <int MODE>
__global__ void __launch_bounds__(kBlock)
mobile_reset_k(MobileParams p, MobileState s, RngState rs, EpisodeStats st, const uint8_t *mask,
               const double *host_rand, int rand_stride, float *obs) {
    int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.n) return;
    if (mask && !mask[e]) return;
    typename RngSel<MODE>::type rng;
    rng_load<MODE>(rng, rs, e, p.n, host_rand, rand_stride, nullptr);
    MobileEnv m;
    load_env(s, e, m);
    reset_env(p, rng, m);
    store_env(s, e, m);
    rng_store<MODE>(rng, rs, e);
    st.ep_return[e] = 0.0; st.ep_length[e] = 0;
    if (obs) {
        float o0, o1;
        observe(p, m, o0, o1);
        if (p.kind == SRLHIP_ENV_MOBILE_1D) obs[e] = o0;
        else reinterpret_cast<float2 *>(obs)[e] = make_float2(o0, o1);
    }
}

// Synthetic random-agent action (rl_baselines/random_agent.py:36) from Philox stream 1 of the env.  Discrete: action i is word i % 4 of
// block i / 4 (multiply-shift into [0, m]) — four actions per Philox block, drawn block by block in sample_plane_entry;
// continuous: one block per action (two float64 uniforms).  oracle/mobile_oracle.c draws the same way.  `actr` counts ACTIONS.
__device__ __forceinline__ int discrete_from_word(const MobileParams &p, uint32_t w) {
    const uint32_t m = p.kind == SRLHIP_ENV_MOBILE_1D ? 1u : 3u;
    return (int)(uint32_t)(((uint64_t)w * ((uint64_t)m + 1)) >> 32);
}
__device__ __forceinline__ float2 sample_continuous_action(uint32_t k0, uint32_t k1, uint64_t actr) {
    Philox ph; ph.k0 = k0; ph.k1 = k1; ph.stream = 1; ph.ctr = actr;
    uint32_t o[4];
    ph.block(o);
    return make_float2((float)(-1.0 + 2.0 * Philox::to_double(o[0], o[1])), (float)(-1.0 + 2.0 * Philox::to_double(o[2], o[3])));
}

// All T x N synthetic actions of a rollout at once, into a [T][N] action plane whose row 0 is action base[e] + offset of env e's stream.
// The plane is covered by `plane_rows` rows of `bpr` workgroups — continuous actions: row t, one block per entry; discrete actions: row q
// is the q-th Philox BLOCK the env's T actions touch (they start anywhere inside their first block: T / 4 + 1 blocks at most), the thread
// writes the up to four entries it yields.  Workgroup `sb` finds its row without an integer division (a 64-bit i / n and i % n per entry
// cost three times the Philox block they index): row = trunc(sb * (1 / bpr)) in float64, off by at most one, corrected.
struct PlaneMap { uint32_t bpr; double inv_bpr; };
inline PlaneMap plane_map(int64_t n) { PlaneMap m; m.bpr = (uint32_t)((n + kBlock - 1) / kBlock); m.inv_bpr = 1.0 / (double)m.bpr; return m; }
inline int64_t plane_rows(const MobileParams &p, int T) { return p.is_discrete ? (int64_t)(T + 3) / 4 + 1 : (int64_t)T; }
__device__ __forceinline__ void sample_plane_entry(const MobileParams &p, const uint32_t *key, const uint64_t *base, uint64_t offset, uint32_t sb,
                                                   const PlaneMap &pm, int T, void *__restrict__ act) {
    int32_t t = (int32_t)((double)sb * pm.inv_bpr);
    int32_t r = (int32_t)sb - t * (int32_t)pm.bpr;
    if (r < 0) { t -= 1; r += (int32_t)pm.bpr; } else if (r >= (int32_t)pm.bpr) { t += 1; r -= (int32_t)pm.bpr; }
    const int64_t e64 = (int64_t)r * kBlock + threadIdx.x;
    if (e64 >= p.n) return;
    const int e = (int)e64;
    if (p.is_discrete) {
        if (t > (T + 3) / 4) return;
        const uint64_t first = base[e] + offset;                    // the env's action index of plane row 0
        Philox ph; ph.k0 = key[e]; ph.k1 = key[p.n + e]; ph.stream = 1; ph.ctr = (first >> 2) + (uint64_t)t;
        const int64_t row0 = (int64_t)(ph.ctr * 4 - first);         // plane row of the block's word 0 (-3 .. T + 3)
        if (row0 >= T) return;
        uint32_t o[4]; ph.block(o);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int64_t row = row0 + w;
            if (row >= 0 && row < T) static_cast<int32_t *>(act)[row * p.n + e] = discrete_from_word(p, o[w]);
        }
        return;
    }
    if (t >= T) return;
    static_cast<float2 *>(act)[(int64_t)t * p.n + e] = sample_continuous_action(key[e], key[p.n + e], base[e] + offset + (uint64_t)t);
}
__global__ void __launch_bounds__(kBlock)
mobile_sample_actions_k(MobileParams p, RngState rs, int T, PlaneMap pm, void *__restrict__ act) {
    sample_plane_entry(p, rs.key, rs.act_ctr, 0, blockIdx.x, pm, T, act);
}

// The actions of kChunk consecutive steps of env e from a [T][n] plane.  They are fetched a chunk at a time because on gfx9 loads and
// stores share one in-order counter (vmcnt): waiting for a load also drains every output store issued before it, so one wait per
// kChunk steps instead of one per step keeps the streamed stores in flight.  Rows past t_last are clamped (fetched, never used).
// (ai / af are the caller's two plain arrays: inside one struct they are not promoted to registers.)
constexpr int kChunk = 16;
__device__ __forceinline__ void gather_actions(const MobileParams &p, const void *__restrict__ actions, int t0, int t_last, int e,
                                               int (&ai)[kChunk], float2 (&af)[kChunk]) {
    const int32_t *act_i = static_cast<const int32_t *>(actions);
    const float2 *act_f = static_cast<const float2 *>(actions);
#pragma unroll
    for (int k = 0; k < kChunk; k++) {
        const int64_t r = (int64_t)min(t0 + k, t_last) * p.n + e;
        if (p.is_discrete) ai[k] = act_i[r]; else af[k] = act_f[r];
    }
    // one full drain per chunk (vmcnt(0), expcnt / lgkmcnt untouched): afterwards no step of the chunk waits on memory
    __builtin_amdgcn_s_waitcnt(0x0F70);
}
__device__ __forceinline__ void chunk_action(const MobileParams &p, const int (&ai)[kChunk], const float2 (&af)[kChunk], int k,
                                             int &a, float &a0, float &a1) {
    a = p.is_discrete ? ai[k] : 0;
    a0 = p.is_discrete ? 0.f : af[k].x; a1 = p.is_discrete ? 0.f : af[k].y;
}

// One launch == T consecutive VecEnv steps; T == 1 with plain stores is the per-step entry point, T > 1 the fused
// rollout.  Actions always come from the [T][N] plane (the caller's, or the one mobile_sample_actions_k just filled:
// `advance_actr` then moves the env's action-stream counter past the T consumed blocks).
template <int MODE, int KIND, int DISC>
__global__ void __launch_bounds__(kBlock)
mobile_rollout_k(MobileParams p, MobileState s, RngState rs, EpisodeStats st, int T, const void *__restrict__ actions,
                 const double *__restrict__ noise, float *__restrict__ obs, float *__restrict__ rew,
                 uint8_t *__restrict__ done_out, int advance_actr, PersistArgs sig) {
    int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.n) return;
    if (KIND >= 0) p.kind = KIND;                 // compile-time constants from here on
    if (DISC >= 0) p.is_discrete = DISC;
    typename RngSel<MODE>::type rng;
    rng_load<MODE>(rng, rs, e, p.n, nullptr, 0, noise);
    MobileEnv m;
    load_env(s, e, m);
    EpisodeLane ep;
    ep.load(st, e);
    for (int t0 = 0; t0 < T; t0 += kChunk) {
        int ai[kChunk]; float2 af[kChunk];
        gather_actions(p, actions, t0, T - 1, e, ai, af);
#pragma unroll
        for (int k = 0; k < kChunk; k++) {
            const int t = t0 + k;
            if (t >= T) continue;                     // (uniform) tail of the last chunk
            const int64_t row = (int64_t)t * p.n + e;
            int a; float a0, a1;
            chunk_action(p, ai, af, k, a, a0, a1);
            double dv = 0.1 + rng.normal(0.0, 0.0);       // DELTA_POS + N(0, NOISE_STD = 0): drawn, value 0
            double reward; bool done;
            step_env<KIND, DISC>(p, m, a, a0, a1, dv, reward, done);
            ep.step(reward, done, [&] { if (p.auto_reset) reset_env(p, rng, m); });
            float o0, o1;
            observe(p, m, o0, o1);
            store_step<true>(p, row, o0, o1, reward, done, obs, rew, done_out);
        }
    }
    if (sig.done) {
        // early completion signal of a single-step launch (step_signal.hpp): per eighth of the grid the last WAVEFRONT to arrive reports
        if (ep.ended()) ep.publish(st, e);           // Monitor's record: the host reads it right after the step
        const int g8 = (int)blockIdx.x & 7;
        const int real = strided_real(g8, (p.n + 63) / 64, kBlock / 64);      // wavefronts with a live lane in the workgroups of this eighth
        const uint32_t xcc = xcd_id();
        uint32_t *cnt = eighth_counter(sig.count, g8);
        const bool first = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0;       // the wavefront's first ACTIVE lane
        if (first) step_signal_tag(cnt, xcc);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
        uint32_t last = 0;
        if (first) last = signal_arrive(cnt, real, sig.start_seq);
        if (__builtin_amdgcn_readfirstlane(last)) {
            signal_writeback();
            if (first) step_signal_post(sig, cnt, g8);
        }
    }
    store_env(s, e, m);
    rng_store<MODE>(rng, rs, e);
    if (advance_actr) rs.act_ctr[e] += (uint64_t)T;
    ep.store(st, e);
}

// What the two policy kernels share: the statistics of the observation normalisation (frozen for the call), a policy's input
// x = clip((o - mean) / sd) in float64, rounded to float32 as the reference's observation is, and the action taken from A float64 scores.
template <int D>
__device__ __forceinline__ void policy_stats(const PolicyArgs &pol, double (&mean)[D], double (&sd)[D]) {
#pragma unroll
    for (int d = 0; d < D; d++) { mean[d] = pol.normalize ? pol.mean[d] : 0.0; sd[d] = pol.normalize ? pol.std[d] : 1.0; }
}
template <int D>
__device__ __forceinline__ void policy_input(const float *o, const PolicyArgs &pol, const double (&mean)[D], const double (&sd)[D], float (&x)[D]) {
#pragma unroll
    for (int d = 0; d < D; d++) {
        x[d] = o[d];
        if (pol.normalize) x[d] = (float)fmin(fmax(((double)o[d] - mean[d]) / sd[d], -pol.clip), pol.clip);
    }
}
// discrete: the strict arg-max (`a`; -1, the reference's `None`, once frozen); continuous: the first two scores as float32 (a0, a1; a zero
// row once frozen: MobileRobot's step has no continuous `None`).  The action goes to row `row` of act_out when there is one.
template <int DISC, int A>
__device__ __forceinline__ void policy_action(const double (&score)[A], bool frozen, int64_t row, void *__restrict__ act_out, int &a, float &a0, float &a1) {
    a = 0; a0 = 0.f; a1 = 0.f;
    if (DISC) {
        double best = score[0];
#pragma unroll
        for (int k = 1; k < A; k++) if (score[k] > best) { best = score[k]; a = k; }       // strict: the lowest index wins a tie
        if (frozen) a = -1;
        if (act_out) __builtin_nontemporal_store(a, static_cast<int32_t *>(act_out) + row);
    } else {
        a0 = frozen ? 0.f : (float)score[0]; a1 = frozen ? 0.f : (float)score[1];
        if (act_out) __builtin_nontemporal_store(f32x2{a0, a1}, reinterpret_cast<f32x2 *>(act_out) + row);
    }
}

// srlhip_rollout_policy_summary (contract: include/srlhip.h): what a learner keeps of a fused policy rollout, formed where each step's
// outputs are — the return up to the env's first done of the call, the live-step count and the first two moments of the live
// observations.  One env's whole call runs in one lane of either policy kernel (the MLP kernel's lead lane), so the sums live in that
// lane and take their terms in ascending t.  Every product is rounded before it is added (this unit is built with -ffp-contract=off;
// the pragma says so here too): a sequential float64 loop over the planes reproduces the bits.
template <int D>
struct SummaryLane {
    double ret = 0.0, s[D], q[D];
    int32_t len = 0;
    bool seen = false;                                   // latched: a row of this call reported done
    __device__ __forceinline__ SummaryLane() {
#pragma unroll
        for (int d = 0; d < D; d++) { s[d] = 0.0; q[d] = 0.0; }
    }
    // row t as the plane call would have written it: o after the step (and its auto-reset), the float32 reward, done
    __device__ __forceinline__ void add(const float *o, double reward, bool done) {
#pragma clang fp contract(off)
        if (seen) return;
        if (!done) ret = ret + (double)(float)reward;   // the reporting step is not counted
#pragma unroll
        for (int d = 0; d < D; d++) {
            const double x = (double)o[d], xx = x * x;
            s[d] = s[d] + x;
            q[d] = q[d] + xx;
        }
        len += 1;
        seen = done;
    }
    __device__ __forceinline__ void store(const SummaryOut &out, int e) const {
        out.ret[e] = ret;
        if (out.length) out.length[e] = len;
        if (out.obs_sum) {
#pragma unroll
            for (int d = 0; d < D; d++) { out.obs_sum[(int64_t)e * D + d] = s[d]; out.obs_sqsum[(int64_t)e * D + d] = q[d]; }
        }
    }
};

// srlhip_rollout_policy: the third action source.  The action of every step is a linear map of the env's own current observation
// (the ARS policy: one env per perturbed policy), so the recurrence cannot be cut into segments: the sequential form, one lane per
// env.  Weights, mean and std sit in registers before the loop and nothing is loaded inside it — the streamed stores are never
// waited for (mobile_rollout_k's chunked vmcnt wait exists for its action plane only).  step_env / reset_env / observe are the
// ones every other kernel uses: with the recorded actions as a GIVEN plane mobile_rollout_k reproduces this kernel bit for bit.
// SAMPLE = true: srlhip_rollout_policy_sampled — the discrete action is drawn from the softmax of the A scores (contract:
// include/srlhip.h) with policy_act.hpp's selection, the text srlhip_sample_actions runs on a score plane: the lane forms its A weights
// itself (A calls of the device library's float64 exp) and draws u from the env's action stream, one block per step.
// SUMMARY = true: srlhip_rollout_policy_summary — the same steps, no plane written, `sum` stored once after the last step.
template <int MODE, int KIND, int DISC, bool SAMPLE = false, bool SUMMARY = false>
__global__ void __launch_bounds__(kBlock)
mobile_rollout_policy_k(MobileParams p, MobileState s, RngState rs, EpisodeStats st, int T, PolicyArgs pol,
                        float *__restrict__ obs, float *__restrict__ rew, uint8_t *__restrict__ done_out, void *__restrict__ act_out, SummaryOut sum) {
    static_assert(!SAMPLE || DISC, "only discrete actions are sampled");
    constexpr int D = KIND == SRLHIP_ENV_MOBILE_1D ? 1 : 2;
    constexpr int A = DISC ? (KIND == SRLHIP_ENV_MOBILE_1D ? 2 : 4) : 2;
    int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.n) return;
    p.kind = KIND; p.is_discrete = DISC;
    typename RngSel<MODE>::type rng;
    rng_load<MODE>(rng, rs, e, p.n, nullptr, 0, nullptr);
    MobileEnv m;
    load_env(s, e, m);
    double W[D][A], mean[D], sd[D];
    const double *w = static_cast<const double *>(pol.w) + (pol.per_env ? (int64_t)e * (D * A) : 0);
#pragma unroll
    for (int d = 0; d < D; d++) {
#pragma unroll
        for (int a = 0; a < A; a++) W[d][a] = w[d * A + a];
    }
    policy_stats<D>(pol, mean, sd);
    EpisodeLane ep;
    ep.load(st, e);
    float o[2];
    observe(p, m, o[0], o[1]);
    Philox draw = {};                                   // SAMPLE: the env's action stream (stream 1), at the counter the call found
    if constexpr (SAMPLE) { draw.k0 = rs.key[e]; draw.k1 = rs.key[p.n + e]; draw.stream = 1; draw.ctr = rs.act_ctr[e]; }
    bool frozen = false;
    SummaryLane<D> sl;
    (void)sl;
    for (int t = 0; t < T; t++) {
        const int64_t row = (int64_t)t * p.n + e;
        float x[D];
        policy_input<D>(o, pol, mean, sd, x);
        double score[A];
#pragma unroll
        for (int d = 0; d < D; d++) {
#pragma unroll
            for (int a = 0; a < A; a++) score[a] = d == 0 ? (double)x[0] * W[0][a] : score[a] + (double)x[d] * W[d][a];
        }
        int a; float a0, a1;
        if constexpr (SAMPLE) {
            double sw[A];
            act_softmax_weights(score, A, sw);
            const int drawn = act_softmax_pick(sw, A, draw.double01());      // one block per step: a frozen env's draw is discarded, not skipped
            a = frozen ? -1 : drawn; a0 = 0.f; a1 = 0.f;
            if (act_out) __builtin_nontemporal_store(a, static_cast<int32_t *>(act_out) + row);
        } else policy_action<DISC, A>(score, frozen, row, act_out, a, a0, a1);
        double dv = 0.1 + rng.normal(0.0, 0.0);       // DELTA_POS + N(0, NOISE_STD = 0): drawn, value 0
        double reward; bool done;
        step_env<KIND, DISC>(p, m, a, a0, a1, dv, reward, done);
        ep.step(reward, done, [&] {
            reset_env(p, rng, m);                     // (the entry point requires auto_reset)
            if (pol.freeze) frozen = true;            // from the NEXT step on
        });
        observe(p, m, o[0], o[1]);
        if constexpr (SUMMARY) sl.add(o, reward, done);
        else store_step<true>(p, row, o[0], o[1], reward, done, obs, rew, done_out);
    }
    store_env(s, e, m);
    rng_store<MODE>(rng, rs, e);
    if constexpr (SAMPLE) rs.act_ctr[e] = draw.ctr;   // c0 + T, whatever happened in between
    ep.store(st, e);
    if constexpr (SUMMARY) sl.store(sum, e);
}

// srlhip_rollout_mlp_policy: the action of every step is a one-hidden-layer ReLU MLP of the env's own current observation (the CMA-ES
// policy: one env per candidate).  P = H D + H + A H + A <= 704 float32 values per env do not fit one lane, so a GROUP of 16 lanes (a
// DPP row) works on one env: lane l keeps the hidden units l, l + 16, ... (at most 8: H <= 128; units >= H are zeros) with their fc_in
// rows, biases and fc_out columns in VGPRs — at most 8 (D + 1 + A) = 56 floats — and lane 0 fc_out's bias.  Nothing is loaded inside
// the step loop (see mobile_rollout_policy_k: the streamed stores are never waited for).  The env itself lives in the group's lead
// lane only (the MT19937 state is regenerated in place in memory: redundant copies of an env would race on it): each step the lead
// lane's observation is broadcast over the row, every lane forms its hidden units and A partial scores in float64, the partials are
// summed over the row by a four-stage DPP butterfly (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror: each
// stage adds two values that both lanes of a pair hold, so every lane ends with the same bits, in an order that never changes),
// and the lead lane takes the action and steps.  Lanes of envs >= n shadow env n - 1 without stepping or storing: every lane of a
// running wavefront stays active for the row operations.  step_env / reset_env / observe are the shared ones.
constexpr int kMlpLanes = 16, kMlpUnits = 8;

template <int CTRL> __device__ __forceinline__ double dpp_f64(double x) {
    const long long v = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double row_sum16(double x) {
    x += dpp_f64<0xB1>(x);        // quad_perm [1,0,3,2]
    x += dpp_f64<0x4E>(x);        // quad_perm [2,3,0,1]
    x += dpp_f64<0x141>(x);       // row_half_mirror
    x += dpp_f64<0x140>(x);       // row_mirror
    return x;
}
__device__ __forceinline__ float row_lead_f32(float x) {      // lane 0 of the row (row_newbcast:0)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x150, 0xf, 0xf, false));
}

// srlhip_rollout_mlp_policy_sampled: the discrete action drawn from the softmax of the A scores (contract: include/srlhip.h).  After
// row_sum16 every lane of the row holds all A scores bit for bit, so the work goes ACROSS the row: every lane takes the maximum, lane
// k < A the one exp(score_k - m) (the device library's float64 exp: ~100 instructions, once per step instead of A times in the lead
// lane), the A weights come back over the row by DPP (row_newbcast:k), and the lead lane — which alone has drawn u — adds them up in
// index order and counts the partial sums z = u * c_{A-1} has passed.  Every lane of the row must be active up to the broadcasts.
template <int K> __device__ __forceinline__ double row_bcast_f64(double x) { return dpp_f64<0x150 + K>(x); }      // lane K of the row
template <int A>
__device__ __forceinline__ void softmax_weights(const double (&score)[A], int l, double (&w)[A]) {
    double m = score[0], own = score[0];
#pragma unroll
    for (int k = 1; k < A; k++) { m = score[k] > m ? score[k] : m; own = l == k ? score[k] : own; }
    const double e = exp(own - m);                  // lanes >= A repeat lane 0's: never read
    w[0] = row_bcast_f64<0>(e); w[1] = row_bcast_f64<1>(e);
    if constexpr (A == 4) { w[2] = row_bcast_f64<2>(e); w[3] = row_bcast_f64<3>(e); }
}
// the inverse CDF, branch-free: how many of c_0 .. c_{A-2} z has reached (the last index takes whatever rounding leaves)
template <int A>
__device__ __forceinline__ int softmax_pick(const double (&w)[A], double u) {
    double c[A];
    c[0] = w[0];
#pragma unroll
    for (int k = 1; k < A; k++) c[k] = c[k - 1] + w[k];
    const double z = u * c[A - 1];
    int a = 0;
#pragma unroll
    for (int k = 0; k < A - 1; k++) a += z >= c[k] ? 1 : 0;
    return a;
}

// SAMPLE = false: srlhip_rollout_mlp_policy (the strict argmax / the continuous row); true: srlhip_rollout_mlp_policy_sampled
// SUMMARY = true: srlhip_rollout_policy_summary — the sums sit in the lead lane, which alone steps the env (SummaryLane)
template <int MODE, int KIND, int DISC, bool SAMPLE = false, bool SUMMARY = false>
__global__ void __launch_bounds__(kBlock)
mobile_rollout_mlp_k(MobileParams p, MobileState s, RngState rs, EpisodeStats st, int T, PolicyArgs pol,
                     float *__restrict__ obs, float *__restrict__ rew, uint8_t *__restrict__ done_out, void *__restrict__ act_out, SummaryOut sum) {
    static_assert(!SAMPLE || DISC, "only discrete actions are sampled");
    constexpr int D = KIND == SRLHIP_ENV_MOBILE_1D ? 1 : 2;
    constexpr int A = DISC ? (KIND == SRLHIP_ENV_MOBILE_1D ? 2 : 4) : 2;
    const int tid = blockIdx.x * kBlock + threadIdx.x, l = tid & (kMlpLanes - 1);
    if ((tid & ~63) / kMlpLanes >= p.n) return;        // a whole wavefront past the last env
    const bool valid = tid / kMlpLanes < p.n, lead = valid && l == 0;
    const int e = valid ? tid / kMlpLanes : p.n - 1;
    p.kind = KIND; p.is_discrete = DISC;
    const int H = pol.hidden;
    float W1[kMlpUnits][D], B1[kMlpUnits], W2[A][kMlpUnits], B2[A];
    const float *w = static_cast<const float *>(pol.w) + (pol.per_env ? (int64_t)e * (H * D + H + A * H + A) : 0);
#pragma unroll
    for (int u = 0; u < kMlpUnits; u++) {
        const int j = l + kMlpLanes * u;
        const bool on = j < H;
        const int jc = on ? j : 0;                     // clamped: every lane loads (inside the env's parameter block) and selects
#pragma unroll                                         // afterwards — a load under a branch would be waited for one by one
        for (int d = 0; d < D; d++) { const float x = w[jc * D + d]; W1[u][d] = on ? x : 0.f; }
        { const float x = w[H * D + jc]; B1[u] = on ? x : 0.f; }
#pragma unroll
        for (int a = 0; a < A; a++) { const float x = w[H * D + H + a * H + jc]; W2[a][u] = on ? x : 0.f; }
    }
#pragma unroll
    for (int a = 0; a < A; a++) { const float x = w[H * D + H + A * H + a]; B2[a] = l == 0 ? x : 0.f; }
    double mean[D], sd[D];
    policy_stats<D>(pol, mean, sd);
    typename RngSel<MODE>::type rng = {};
    MobileEnv m = {};
    EpisodeLane ep;
    float o[2] = {0.f, 0.f};
    Philox draw = {};                                   // SAMPLE: the env's action stream (stream 1), at the counter the call found
    if (lead) {
        rng_load<MODE>(rng, rs, e, p.n, nullptr, 0, nullptr);
        load_env(s, e, m);
        ep.load(st, e);
        observe(p, m, o[0], o[1]);
        if constexpr (SAMPLE) { draw.k0 = rs.key[e]; draw.k1 = rs.key[p.n + e]; draw.stream = 1; draw.ctr = rs.act_ctr[e]; }
    }
    bool frozen = false;
    SummaryLane<D> sl;
    (void)sl;
    for (int t = 0; t < T; t++) {
        double score[A];
#pragma unroll
        for (int a = 0; a < A; a++) score[a] = (double)B2[a];
        float od[D], x[D];
#pragma unroll
        for (int d = 0; d < D; d++) od[d] = row_lead_f32(o[d]);
        policy_input<D>(od, pol, mean, sd, x);
#pragma unroll
        for (int u = 0; u < kMlpUnits; u++) {
            double hu = (double)B1[u];
#pragma unroll
            for (int d = 0; d < D; d++) hu += (double)W1[u][d] * (double)x[d];
            hu = hu > 0.0 ? hu : 0.0;
#pragma unroll
            for (int a = 0; a < A; a++) score[a] += (double)W2[a][u] * hu;
        }
#pragma unroll
        for (int a = 0; a < A; a++) score[a] = row_sum16(score[a]);
        double sw[A];
        (void)sw;
        if constexpr (SAMPLE) softmax_weights<A>(score, l, sw);
        if (lead) {
            const int64_t row = (int64_t)t * p.n + e;
            int a; float a0, a1;
            if constexpr (SAMPLE) {
                const int drawn = softmax_pick<A>(sw, draw.double01());      // one block per step: a frozen env's draw is discarded, not skipped
                a = frozen ? -1 : drawn; a0 = 0.f; a1 = 0.f;
                if (act_out) __builtin_nontemporal_store(a, static_cast<int32_t *>(act_out) + row);
            } else policy_action<DISC, A>(score, frozen, row, act_out, a, a0, a1);
            double dv = 0.1 + rng.normal(0.0, 0.0);       // DELTA_POS + N(0, NOISE_STD = 0): drawn, value 0
            double reward; bool done;
            step_env<KIND, DISC>(p, m, a, a0, a1, dv, reward, done);
            ep.step(reward, done, [&] {
                reset_env(p, rng, m);                     // (the entry point requires auto_reset)
                if (pol.freeze) frozen = true;            // from the NEXT step on
            });
            observe(p, m, o[0], o[1]);
            if constexpr (SUMMARY) sl.add(o, reward, done);
            else store_step<true>(p, row, o[0], o[1], reward, done, obs, rew, done_out);
        }
    }
    if (!lead) return;
    store_env(s, e, m);
    rng_store<MODE>(rng, rs, e);
    if constexpr (SAMPLE) rs.act_ctr[e] = draw.ctr;   // c0 + T, whatever happened in between
    ep.store(st, e);
    if constexpr (SUMMARY) sl.store(sum, e);
}

// Persistent stepping (srlhip_set_persistent; the protocol is step_signal.hpp's): ONE launch stays resident with every env's state in
// registers; every lane reads its action from the mapped plane, steps and stores its outputs straight to the host's mapped planes, the
// last wavefront of each eighth of the grid (workgroups b = g mod 8) reports.  Where an eighth does not sit on one XCD the outputs are
// written through instead (system-scope stores: slow, correct).  Same step code as mobile_rollout_k: bit-identical.
template <int MODE, int KIND, int DISC>
__global__ void __launch_bounds__(kBlock)
mobile_persist_k(MobileParams p, MobileState s, RngState rs, EpisodeStats st, const void *actions, float *obs, float *rew, uint8_t *done_out, PersistArgs pa) {
    __shared__ uint32_t tok_s, verdict_s;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = e < p.n;
    const int ee = valid ? e : p.n - 1;
    p.kind = KIND; p.is_discrete = DISC;
    const uint32_t xcc = xcd_id();
    if (threadIdx.x == 0) persist_register(pa, xcc);
    typename RngSel<MODE>::type rng;
    rng_load<MODE>(rng, rs, ee, p.n, nullptr, 0, nullptr);
    MobileEnv m;
    load_env(s, ee, m);
    EpisodeLane ep;
    ep.load(st, ee);
    ep.last_reward = st.last_reward[ee];               // (a resident kernel may park before it has taken a step)
    // start barrier: every workgroup has registered -> 1: direct outputs, 2: written-through outputs, 3: told to stop while waiting
    if (threadIdx.x == 0) {
        uint32_t verdict = 0;
        uint32_t *vw = pa.ctrl + (kWordVerdict - kWordCtrl);
        if (blockIdx.x == 0) {
            for (;;) {
                const uint32_t reg = __hip_atomic_load(pa.ctrl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((reg & 0xffffu) == gridDim.x) { verdict = ((reg >> 16) || pa.force_staged) ? 2u : 1u; break; }
                if (__hip_atomic_load(pa.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { verdict = 3u; break; }
                __builtin_amdgcn_s_sleep(8);
            }
            __hip_atomic_store(vw, verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            while (!(verdict = __hip_atomic_load(vw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) __builtin_amdgcn_s_sleep(8);
        }
        verdict_s = verdict;
    }
    __syncthreads();
    const uint32_t verdict = verdict_s;
    const bool direct = verdict == 1u;
    const int g8 = (int)blockIdx.x & 7;
    const int real = strided_real(g8, (p.n + 63) / 64, kBlock / 64);          // wavefronts with a live lane in the workgroups of this eighth
    const bool first = valid && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0;     // (lanes of a wavefront are valid from lane 0 up)
    uint32_t my_seq = pa.start_seq, k = 0;
    const int od = p.kind == SRLHIP_ENV_MOBILE_1D ? 1 : 2;
    while (verdict != 3u) {
        if (threadIdx.x == 0) {
            uint32_t token;
            if (blockIdx.x == 0) {
                uint32_t sq = my_seq, stop = 0, spins = 0;
                for (;;) {
                    const uint64_t w = __hip_atomic_load(reinterpret_cast<const uint64_t *>(pa.seq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    sq = (uint32_t)w; stop = (uint32_t)(w >> 32);
                    if (sq != my_seq || stop || ++spins >= pa.spin_limit) break;
                    __builtin_amdgcn_s_sleep(8);
                }
                token = sq != my_seq ? sq : kPersistPark;
                if (token == kPersistPark) __hip_atomic_store(pa.parked, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                for (int x = 0; x < 8; x++) __hip_atomic_store(pa.relay + x * kPersistWordStride, token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                const uint32_t *rw = pa.relay + (blockIdx.x & 7) * kPersistWordStride;
                while ((token = __hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == my_seq) __builtin_amdgcn_s_sleep(8);
            }
            tok_s = token;
        }
        __syncthreads();
        const uint32_t token = tok_s;
        __syncthreads();                                   // everybody has read the token before thread 0 writes the next one
        if (token == kPersistPark) break;
        my_seq = token; k += 1;
        if (valid) {
            int a = 0; float a0 = 0.f, a1 = 0.f;
            if (p.is_discrete) a = __hip_atomic_load(static_cast<const int32_t *>(actions) + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else {
                a0 = __hip_atomic_load(static_cast<const float *>(actions) + 2 * e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                a1 = __hip_atomic_load(static_cast<const float *>(actions) + 2 * e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            double dv = 0.1 + rng.normal(0.0, 0.0);       // DELTA_POS + N(0, NOISE_STD = 0): drawn, value 0
            double reward; bool done;
            step_env<KIND, DISC>(p, m, a, a0, a1, dv, reward, done);
            ep.step(reward, done, [&] {
                if (p.auto_reset) reset_env(p, rng, m);
                ep.publish(st, e);                        // Monitor's record, with the step
            });
            float o0, o1;
            observe(p, m, o0, o1);
            if (direct) {                                  // (per-env planes in the host's mapped memory: not store_step's streamed rows)
                if (od == 1) obs[e] = o0; else { obs[2 * e] = o0; obs[2 * e + 1] = o1; }
                rew[e] = (float)reward; done_out[e] = (uint8_t)done;
            } else {
                __hip_atomic_store(obs + od * e, o0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (od == 2) __hip_atomic_store(obs + 2 * e + 1, o1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(rew + e, (float)reward, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(done_out + e, (uint8_t)done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
        uint32_t last = 0;
        if (first) last = signal_arrive(eighth_counter(pa.count, g8), real, k);
        if (__builtin_amdgcn_readfirstlane(last)) {
            signal_writeback();
            if (first) persist_post(pa, g8, my_seq);
        }
    }
    if (!valid) return;
    store_env(s, e, m);
    rng_store<MODE>(rng, rs, e);
    ep.store<false>(st, e);                                // every record was published with its step
}

// Episode-parallel rollout (Philox mode with auto-reset).  In the MobileRobot family an episode always lasts exactly
// 251 steps (`done = counter > 250`, `terminated` is never set: mobile_robot_env.py:336-343) and a reset consumes a
// fixed number of counter-based draws, so the state an env has right after its k-th reset inside a rollout is a pure
// function of (key, counter + (k-1) * draws): the T-step rollout of one env splits into independent segments — the
// rest of its running episode, then whole episodes — which run on separate lanes.  At the 4096-env BASELINE size a
// 2048-step rollout becomes 4096 x 10 lanes of <= 251 steps instead of 4096 lanes of 2048 steps: the recurrence is the
// only sequential thing on this path, and this cuts it ~8x.  Outputs, final state, counters and episode statistics
// are bit-identical to mobile_rollout_k (tests/test_gpu_mobile.py).  Lane (j, e) = segment j of env e; the waves of a
// segment slot store whole [t][e..e+63] rows when their envs' episode clocks agree (they do after a common reset).
constexpr int kEpisodeSteps = 251;

// Everything a segment lane reads from the per-env state.  The lanes of one env are NOT guaranteed to be co-resident
// (beyond ~0.5 M lanes later blocks are dispatched after earlier ones retire), and the lane that finishes an env's rollout
// overwrites its state: the segments therefore read this snapshot, taken by mobile_snapshot_k in stream order right
// before the launch, and only write the live state (MobileSnapSet, internal.hpp: the kernel reads one set; the lane that leaves an
// env's final state ALSO writes it into the other one, which the next launch will read — an all-null set: nowhere).
// The synthetic agent's NEXT action plane, drawn by the workgroups of a rollout launch beyond its segment lanes (the rollout itself
// is a latency-bound recurrence on 10 x N lanes: the chip has room) so that the following rollout starts without a sampler launch:
// block base[e] + T + t of env e's action stream (base = the counters in the snapshot: the live ones move when the rollout ends).
struct NextPlane { void *act; const uint64_t *base; int ep_blocks; PlaneMap pm; };

__global__ void __launch_bounds__(kBlock)
mobile_snapshot_k(int n, MobileState s, RngState rs, EpisodeStats st, MobileSnapSet d) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    d.actr[e] = rs.act_ctr[e];
    d.s.pos_x[e] = s.pos_x[e]; d.s.pos_y[e] = s.pos_y[e]; d.s.tgt_x[e] = s.tgt_x[e]; d.s.tgt_y[e] = s.tgt_y[e];
    d.s.tgt2_x[e] = s.tgt2_x[e]; d.s.tgt2_y[e] = s.tgt2_y[e]; d.s.counter[e] = s.counter[e]; d.s.cur_target[e] = s.cur_target[e];
    d.ctr[e] = rs.ctr[e]; d.ep_return[e] = st.ep_return[e]; d.ep_length[e] = st.ep_length[e];
}

template <int KIND, int DISC, int SHAPE, int PLANES>      // PLANES: 0 check every output plane, 1 obs / reward / done present, 2 those and act_out
__global__ void __launch_bounds__(kBlock)
mobile_rollout_ep_k(MobileParams p, MobileState s, MobileSnapSet snap, RngState rs, EpisodeStats st, int T, int draws_per_reset, int smax,
                    const void *__restrict__ actions, float *__restrict__ obs, float *__restrict__ rew,
                    uint8_t *__restrict__ done_out, int advance_actr, NextPlane next, void *__restrict__ act_out, MobileSnapSet snap_out) {
    p.kind = KIND; p.is_discrete = DISC; p.shape_reward = SHAPE;            // compile-time constants from here on
    if ((int)blockIdx.x >= next.ep_blocks) {                               // spare workgroups: the next rollout's action plane
        sample_plane_entry(p, rs.key, next.base, (uint64_t)T, blockIdx.x - (uint32_t)next.ep_blocks, next.pm, T, next.act);
        return;
    }
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(gid % p.n), j = (int)(gid / p.n);
    if (j >= smax) return;
    const int c0 = snap.s.counter[e];
    const int L0 = c0 <= kEpisodeSteps - 1 ? kEpisodeSteps - c0 : 1;       // steps until the running episode ends
    const int t_lo = j == 0 ? 0 : L0 + kEpisodeSteps * (j - 1);
    if (t_lo >= T) return;
    const int t_end = L0 + kEpisodeSteps * j;                             // the step after this segment's episode ends
    const int t_hi = t_end < T ? t_end : T;
    const bool last = t_hi == T;                                          // this lane leaves the env's final state
    const int n_completed = T >= L0 ? 1 + (T - L0) / kEpisodeSteps : 0;   // episodes of env e that finish inside the rollout
    PhiloxRng rng;
    rng.p.k0 = rs.key[e]; rng.p.k1 = rs.key[p.n + e]; rng.p.stream = 0;
    const uint64_t ctr0 = snap.ctr[e];
    MobileEnv m;
    // this SEGMENT's accounting: at most one episode ends in it, so last_ret / last_len are the segment's own finished episode, and
    // the env's count of finished episodes is arithmetic (n_completed), not a lane's count
    EpisodeLane ep;
    if (j == 0) {
        load_env(snap.s, e, m);
        rng.p.ctr = ctr0;
        ep.ep_ret = snap.ep_return[e]; ep.ep_len = snap.ep_length[e];
    } else {
        rng.p.ctr = ctr0 + (uint64_t)(j - 1) * (uint64_t)draws_per_reset;
        reset_env(p, rng, m);                                              // the reset the previous segment ends with
    }
    const int32_t *act_i = static_cast<const int32_t *>(actions);
    const float2 *act_f = static_cast<const float2 *>(actions);
    int t_start = t_lo;
    // Fast loop: whole chunks of INTERIOR steps.  Inside a segment `done` can only fire at the step that ends its episode
    // (t_end - 1), so every earlier step needs no reset; with all four output planes present (ALL) and every lane of the wavefront
    // holding a full chunk, a chunk is one straight-line block: no per-step predicate, no reset body to branch around, no plane
    // checks — the scheduler overlaps one step's conversions and stores with the next step's dependent chain.  Ragged clocks, the
    // last partial chunk and the episode-ending step go through the general loop below.
    if constexpr (PLANES > 0) {
        // The actions of the NEXT chunk are requested before this chunk's steps: loads and stores retire in order on one counter
        // (vmcnt), so a load issued ahead of the chunk's 3-4 x kFast stores is awaited with those stores still in flight (the compiler
        // counts them: the block is straight-line) instead of exposing a full memory round trip per chunk.  8 + 32 operations stay
        // below the counter's 63.
        constexpr int kFast = 8;
        const int t_int_end = t_end - 1 < t_hi ? t_end - 1 : t_hi;       // interior steps: [t_lo, t_int_end)
        int ai[kFast]; float2 af[kFast];
        auto fetch = [&](int t0, int *di, float2 *df) {
#pragma unroll
            for (int k = 0; k < kFast; k++) {
                const int64_t r = (int64_t)min(t0 + k, t_hi - 1) * p.n + e;   // clamped: a prefetch past the segment is harmless
                if (p.is_discrete) di[k] = act_i[r]; else df[k] = act_f[r];
            }
        };
        auto chunk = [&](const int *ci, const float2 *cf) {
#pragma unroll
            for (int k = 0; k < kFast; k++) {
                const int64_t row = (int64_t)(t_start + k) * p.n + e;
                const int a = p.is_discrete ? ci[k] : 0;
                const float a0 = p.is_discrete ? 0.f : cf[k].x, a1 = p.is_discrete ? 0.f : cf[k].y;
                if constexpr (PLANES == 2) {
                    if (p.is_discrete) __builtin_nontemporal_store(a, static_cast<int32_t *>(act_out) + row);
                    else static_cast<float2 *>(act_out)[row] = make_float2(a0, a1);
                }
                const double dv = 0.1 + rng.normal(0.0, 0.0);
                double reward; bool done;
                step_env<KIND, DISC, SHAPE>(p, m, a, a0, a1, dv, reward, done);     // done is false here (interior step)
                ep.add(reward);
                float o0, o1;
                observe(p, m, o0, o1);
                store_step<false>(p, row, o0, o1, reward, false, obs, rew, done_out);
            }
            t_start += kFast;
        };
        if (__all(t_start + kFast <= t_int_end)) {
            fetch(t_start, ai, af);
            __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0) once, so that the loop header has nothing pending on either path
            do {
                int ni[kFast]; float2 nf[kFast];
                fetch(t_start + kFast, ni, nf);
                __builtin_amdgcn_sched_barrier(0);                         // keep the requests AHEAD of the chunk's stores
                chunk(ai, af);
                __builtin_amdgcn_sched_barrier(0);
                // the copies are the first use of the prefetched registers: the wait lands HERE, where what is pending is known
                // exactly (8 loads, then 32 stores) — at the loop header it would be merged with the entry path and drain everything
#pragma unroll
                for (int k = 0; k < kFast; k++) { ai[k] = ni[k]; af[k] = nf[k]; }
            } while (__all(t_start + kFast <= t_int_end));
        }
    }
    for (int t0 = t_start; t0 < t_hi; t0 += kChunk) {
        int ai[kChunk]; float2 af[kChunk];
        gather_actions(p, actions, t0, t_hi - 1, e, ai, af);
#pragma unroll
        for (int k = 0; k < kChunk; k++) {
            const int t = t0 + k;
            if (t < t_hi) {
                const int64_t row = (int64_t)t * p.n + e;
                int a; float a0, a1;
                chunk_action(p, ai, af, k, a, a0, a1);
                if (act_out) {                                             // the plane is internal: hand the actions taken to the caller
                    if (p.is_discrete) __builtin_nontemporal_store(a, static_cast<int32_t *>(act_out) + row);
                    else static_cast<float2 *>(act_out)[row] = make_float2(a0, a1);
                }
                const double dv = 0.1 + rng.normal(0.0, 0.0);              // DELTA_POS + N(0, NOISE_STD = 0): draws nothing
                double reward; bool done;
                step_env<KIND, DISC, SHAPE>(p, m, a, a0, a1, dv, reward, done);
                ep.step(reward, done, [&] { reset_env(p, rng, m); });
                float o0, o1;
                observe(p, m, o0, o1);
                store_step<true>(p, row, o0, o1, reward, done, obs, rew, done_out);
            }
        }
    }
    // The exit is not EpisodeLane::store: the fields of one env are left by different lanes.  (last_return / last_length: written when
    // an episode ended, never read — the rule stated there)
    if (t_end <= T && j == n_completed - 1) {        // the last episode that finished inside the rollout
        st.last_return[e] = ep.last_ret; st.last_length[e] = ep.last_len;
    }
    if (last) {
        store_env(s, e, m);
        rs.ctr[e] = rng.p.ctr;
        const uint64_t actr = rs.act_ctr[e] + (advance_actr ? (uint64_t)T : 0);
        if (advance_actr) rs.act_ctr[e] = actr;
        st.ep_return[e] = ep.ep_ret; st.ep_length[e] = ep.ep_len; st.last_reward[e] = ep.last_reward;
        st.n_finished[e] += n_completed;
        if (snap_out.ctr) {                  // the next launch's snapshot (this launch reads the other set)
            store_env(snap_out.s, e, m);
            snap_out.ctr[e] = rng.p.ctr; snap_out.actr[e] = actr; snap_out.ep_return[e] = ep.ep_ret; snap_out.ep_length[e] = ep.ep_len;
        }
    }
}

MobileParams params_of(const Handle *h) {
    MobileParams p;
    p.kind = h->cfg.env_kind; p.is_discrete = h->cfg.is_discrete; p.random_target = h->cfg.random_target;
    p.shape_reward = h->cfg.shape_reward; p.auto_reset = h->cfg.auto_reset; p.n = h->n;
    return p;
}

}  // namespace

namespace {

int alloc_state(Handle *h, MobileState &s) {
    const size_t n = (size_t)h->n;
    int rc = 0;
    (void)((rc = h->dalloc(&s.pos_x, n)) || (rc = h->dalloc(&s.pos_y, n)) || (rc = h->dalloc(&s.tgt_x, n)) ||
           (rc = h->dalloc(&s.tgt_y, n)) || (rc = h->dalloc(&s.tgt2_x, n)) || (rc = h->dalloc(&s.tgt2_y, n)) ||
           (rc = h->dalloc(&s.counter, n)) || (rc = h->dalloc(&s.cur_target, n)));
    return rc;
}

// Run-time configuration -> template arguments (internal.hpp: Const / dispatch_int).  Only the combinations a caller dispatches on
// exist in the library.
template <class F>
void dispatch_device_rng(int rng_mode, F &&f) { dispatch_int<SRLHIP_RNG_PHILOX, SRLHIP_RNG_MT19937>(rng_mode, f); }
template <class F>
void dispatch_env(const MobileParams &p, F &&f) {           // f(kind, is_discrete)
    dispatch_int<SRLHIP_ENV_MOBILE, SRLHIP_ENV_MOBILE_1D, SRLHIP_ENV_MOBILE_2TARGET, SRLHIP_ENV_MOBILE_LINE>(p.kind, [&](auto kind) {
        dispatch_int<0, 1>(p.is_discrete ? 1 : 0, [&](auto disc) { f(kind, disc); });
    });
}
// MobileRobot1D / 2Target take discrete actions only (srlhip_create refuses the other combination): not instantiated for the policy kernels
constexpr bool policy_combination(int kind, int disc) { return disc || (kind != SRLHIP_ENV_MOBILE_1D && kind != SRLHIP_ENV_MOBILE_2TARGET); }

}  // namespace

static int mobile_alloc(Handle *h) {
    int rc = alloc_state(h, h->mobile);
    if (rc) return rc;
    if (h->cfg.rng_mode == SRLHIP_RNG_PHILOX) {
        // snapshot planes of the episode-parallel rollout (launch_rollout_ep): allocated with the handle, never lazily — a
        // first rollout may sit inside srlhip_graph_begin / srlhip_graph_end, where hipMalloc is illegal
        const size_t n = (size_t)h->n;
        for (MobileSnapSet &d : h->snap)
            if ((rc = alloc_state(h, d.s)) || (rc = h->dalloc(&d.ep_return, n)) || (rc = h->dalloc(&d.ep_length, n)) ||
                (rc = h->dalloc(&d.ctr, n)) || (rc = h->dalloc(&d.actr, n)))
                return rc;
    }
    return 0;
}

static int mobile_reset(Handle *h, const uint8_t *d_mask, const double *d_host_rand, void *d_obs_plane) {
    float *d_obs = static_cast<float *>(d_obs_plane);
    h->snap_valid = false;
    MobileParams p = params_of(h);
    dim3 grid((h->n + kBlock - 1) / kBlock), block(kBlock);
    int stride = reset_rand_count(h->cfg);
    if (h->cfg.rng_mode == SRLHIP_RNG_HOST && !d_host_rand) return h->fail(SRLHIP_EINVAL, "reset: RNG_HOST needs host_rand");
    dispatch_int<SRLHIP_RNG_HOST, SRLHIP_RNG_PHILOX, SRLHIP_RNG_MT19937>(h->cfg.rng_mode, [&](auto mode) {
        hipLaunchKernelGGL(mobile_reset_k<decltype(mode)::value>, grid, block, 0, h->stream, p, h->mobile, h->rng, h->stats, d_mask,
                           d_host_rand, stride, d_obs);
    });
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

namespace {

template <int MODE>
void launch_rollout(Handle *h, const MobileParams &p, int T, const void *d_actions, const double *d_noise, float *d_obs,
                    float *d_rew, uint8_t *d_done, int advance_actr) {
    dim3 grid((h->n + kBlock - 1) / kBlock), block(kBlock);
    PersistArgs sig{};                          // the early completion signal of a single-step launch with the caller's actions (api.hip)
    if (h->step_signal.done && T == 1 && d_actions && !advance_actr) {
        sig = h->step_signal; h->step_signal_armed = true;
        h->signal_eighths = strided_eighths((int)grid.x);
    }
    dispatch_env(p, [&](auto kind, auto disc) {
        hipLaunchKernelGGL((mobile_rollout_k<MODE, decltype(kind)::value, decltype(disc)::value>), grid, block, 0, h->stream, p, h->mobile,
                           h->rng, h->stats, T, d_actions, d_noise, d_obs, d_rew, d_done, advance_actr, sig);
    });
}

// next_plane: where the spare workgroups put the following rollout's actions (null: none); act_out: the caller's action plane
// when `d_actions` is an internal one
int launch_rollout_ep(Handle *h, const MobileParams &p, int T, const void *d_actions, float *d_obs, float *d_rew,
                      uint8_t *d_done, int advance_actr, void *next_plane, void *act_out) {
    // two snapshot sets in turn: this launch reads set `cur` — written by the previous rollout launch's final-state lanes, or by
    // mobile_snapshot_k now when anything else has touched the state since — and writes the env's final state into the other one.
    // Inside a stream capture the copy kernel always runs and nothing is written ahead: a replayed graph must not depend on which set
    // the previous replay left behind.
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(h->stream, &capture);
    const bool chained = capture == hipStreamCaptureStatusNone;
    const int cur = h->snap_cur;
    const MobileSnapSet snap = h->snap[cur], snap_out = chained ? h->snap[cur ^ 1] : MobileSnapSet{};
    if (!h->snap_valid || !chained)
        hipLaunchKernelGGL(mobile_snapshot_k, dim3((h->n + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->n, h->mobile, h->rng, h->stats, snap);
    h->snap_cur = chained ? cur ^ 1 : cur;
    h->snap_valid = chained;
    const int smax = 1 + (T - 1 + kEpisodeSteps - 1) / kEpisodeSteps;     // first segment of one step + whole episodes
    const int64_t lanes = (int64_t)smax * h->n;
    const int ep_blocks = (int)((lanes + kBlock - 1) / kBlock);
    const PlaneMap pm = plane_map(h->n);
    const int64_t extra = next_plane ? plane_rows(p, T) * pm.bpr : 0;
    const NextPlane next{next_plane, snap.actr, ep_blocks, pm};
    dim3 grid((unsigned)(ep_blocks + extra)), block(kBlock);
    const int draws = reset_rand_count(h->cfg);
    const int planes = d_obs && d_rew && d_done ? (act_out ? 2 : 1) : 0;   // the fast loop stores without checking
    dispatch_env(p, [&](auto kind, auto disc) {
        dispatch_int<0, 1>(p.shape_reward ? 1 : 0, [&](auto shape) {
            dispatch_int<0, 1, 2>(planes, [&](auto pl) {
                hipLaunchKernelGGL((mobile_rollout_ep_k<decltype(kind)::value, decltype(disc)::value, decltype(shape)::value, decltype(pl)::value>),
                                   grid, block, 0, h->stream, p, h->mobile, snap, h->rng, h->stats, T, draws, smax, d_actions, d_obs, d_rew,
                                   d_done, advance_actr, next, act_out, snap_out);
            });
        });
    });
    return 0;
}

}  // namespace

static int mobile_rollout(Handle *h, int T, const void *d_actions, void *d_obs_plane, float *d_rew, uint8_t *d_done,
                          void *d_act_out) {
    float *d_obs = static_cast<float *>(d_obs_plane);
    MobileParams p = params_of(h);
    if (h->cfg.rng_mode != SRLHIP_RNG_PHILOX && h->cfg.rng_mode != SRLHIP_RNG_MT19937)
        return h->fail(SRLHIP_EINVAL, "rollout: needs a device RNG mode (PHILOX or MT19937)");
    int advance = 0;
    const bool ep_path = h->cfg.rng_mode == SRLHIP_RNG_PHILOX && p.auto_reset && T >= 32;
    if (!d_actions && ep_path && !getenv("SRLHIP_NO_ACTION_PREFETCH")) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(h->stream, &cap);
        if (cap == hipStreamCaptureStatusNone) {
            // synthetic agent, episode-parallel rollout: two internal action planes in turn.  This rollout reads the plane the
            // previous launch's spare workgroups filled (or fills one now), its own spare workgroups fill the other one.
            const size_t bytes = (size_t)T * h->n * (p.is_discrete ? 4 : 8);
            for (int b = 0; b < 2; b++)
                if (h->act_plane[b].cap < bytes) {           // regrown: a launch in flight may still read or fill the old plane
                    SRL_HIP_CHECK(h, hipStreamSynchronize(h->stream));
                    h->prefetch_valid = false;
                    int rc = ensure(h, h->act_plane[b], bytes);
                    if (rc) return rc;
                }
            int cur = 0;
            if (h->prefetch_valid && h->prefetch_T == T) cur = h->prefetch_buf;
            else {
                const PlaneMap pm = plane_map(h->n);
                hipLaunchKernelGGL(mobile_sample_actions_k, dim3((unsigned)(plane_rows(p, T) * pm.bpr)), dim3(kBlock), 0, h->stream,
                                   p, h->rng, T, pm, h->act_plane[0].p);
                SRL_HIP_CHECK(h, hipGetLastError());
            }
            int rc = launch_rollout_ep(h, p, T, h->act_plane[cur].p, d_obs, d_rew, d_done, 1, h->act_plane[cur ^ 1].p, d_act_out);
            if (rc) return rc;
            SRL_HIP_CHECK(h, hipGetLastError());
            h->prefetch_valid = true; h->prefetch_T = T; h->prefetch_buf = cur ^ 1;
            return 0;
        }
    }
    if (!d_actions) {
        h->prefetch_valid = false;              // this rollout moves the action-stream counters past what was drawn ahead
        // synthetic agent: draw the whole [T][N] action plane in parallel, into the caller's plane when there is one
        const size_t bytes = (size_t)T * h->n * (p.is_discrete ? 4 : 8);
        void *plane = d_act_out;
        if (!plane) {
            int rc = ensure(h, h->st[ST_NOISE], bytes);
            if (rc) return rc;
            plane = h->st[ST_NOISE].p;
        }
        const PlaneMap pm = plane_map(h->n);
        hipLaunchKernelGGL(mobile_sample_actions_k, dim3((unsigned)(plane_rows(p, T) * pm.bpr)), dim3(kBlock), 0, h->stream,
                           p, h->rng, T, pm, plane);
        SRL_HIP_CHECK(h, hipGetLastError());
        d_actions = plane;
        advance = 1;
    }
    // counter-based streams + fixed-length episodes: segments of the rollout run in parallel (mobile_rollout_ep_k)
    if (ep_path) {
        int rc = launch_rollout_ep(h, p, T, d_actions, d_obs, d_rew, d_done, advance, nullptr, nullptr);
        if (rc) return rc;
    } else {
        h->snap_valid = false;           // the sequential kernel moves the live state only
        dispatch_device_rng(h->cfg.rng_mode, [&](auto mode) {
            launch_rollout<decltype(mode)::value>(h, p, T, d_actions, nullptr, d_obs, d_rew, d_done, advance);
        });
    }
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

// srlhip_rollout_policy (pol.hidden == 0: one lane per env) / srlhip_rollout_mlp_policy (16 lanes per env) and, with `sample`, their
// sampled forms srlhip_rollout_policy_sampled / srlhip_rollout_mlp_policy_sampled
static int mobile_rollout_policy(Handle *h, int T, const PolicyArgs &pol, bool sample, KukaPolicyLaunch, void *d_obs_plane, float *d_rew, uint8_t *d_done, void *d_act_out,
                                 const SummaryOut *sum) {
    float *d_obs = static_cast<float *>(d_obs_plane);
    const MobileParams p = params_of(h);
    const std::string name = sum ? kSummaryName : sample ? (pol.hidden ? "rollout_mlp_policy_sampled" : "rollout_policy_sampled") : pol.hidden ? "rollout_mlp_policy" : "rollout_policy";
    if ((h->cfg.rng_mode != SRLHIP_RNG_PHILOX && h->cfg.rng_mode != SRLHIP_RNG_MT19937) || !p.auto_reset)
        return h->fail(SRLHIP_ENOTSUP, name + ": needs auto_reset and a device RNG mode (PHILOX or MT19937)");
    if (sample && !p.is_discrete)
        return h->fail(SRLHIP_ENOTSUP, name + ": only discrete actions are sampled");
    h->snap_valid = false;                      // the live state moves, the episode-parallel rollout's snapshot set does not
    if (sample) h->prefetch_valid = false;      // ... and the action-stream counters move past what the synthetic agent drew ahead
    dim3 grid(((int64_t)h->n * (pol.hidden ? kMlpLanes : 1) + kBlock - 1) / kBlock), block(kBlock);
    const SummaryOut so = sum ? *sum : SummaryOut{};
    const auto launch = [&](auto summary) {
        constexpr bool SUMMARY = decltype(summary)::value != 0;
        dispatch_device_rng(h->cfg.rng_mode, [&](auto mode) {
            dispatch_env(p, [&](auto kind, auto disc) {
                constexpr int MODE = decltype(mode)::value, KIND = decltype(kind)::value, DISC = decltype(disc)::value;
                if constexpr (policy_combination(KIND, DISC)) {
                    if constexpr (DISC == 1) {
                        if (sample) {
                            if (pol.hidden)
                                hipLaunchKernelGGL((mobile_rollout_mlp_k<MODE, KIND, 1, true, SUMMARY>), grid, block, 0, h->stream, p, h->mobile, h->rng, h->stats, T, pol,
                                                   d_obs, d_rew, d_done, d_act_out, so);
                            else
                                hipLaunchKernelGGL((mobile_rollout_policy_k<MODE, KIND, 1, true, SUMMARY>), grid, block, 0, h->stream, p, h->mobile, h->rng, h->stats, T,
                                                   pol, d_obs, d_rew, d_done, d_act_out, so);
                            return;
                        }
                    }
                    if (pol.hidden)
                        hipLaunchKernelGGL((mobile_rollout_mlp_k<MODE, KIND, DISC, false, SUMMARY>), grid, block, 0, h->stream, p, h->mobile, h->rng, h->stats, T, pol,
                                           d_obs, d_rew, d_done, d_act_out, so);
                    else
                        hipLaunchKernelGGL((mobile_rollout_policy_k<MODE, KIND, DISC, false, SUMMARY>), grid, block, 0, h->stream, p, h->mobile, h->rng, h->stats, T,
                                           pol, d_obs, d_rew, d_done, d_act_out, so);
                }
            });
        });
    };
    if (sum) launch(Const<1>{}); else launch(Const<0>{});
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

static int mobile_step(Handle *h, const void *d_actions, const double *d_noise, void *d_obs_plane, float *d_rew,
                       uint8_t *d_done) {
    if (h->cfg.rng_mode != SRLHIP_RNG_HOST) return mobile_rollout(h, 1, d_actions, d_obs_plane, d_rew, d_done, nullptr);
    float *d_obs = static_cast<float *>(d_obs_plane);
    h->snap_valid = false;
    MobileParams p = params_of(h);
    dim3 grid((h->n + kBlock - 1) / kBlock), block(kBlock);
    hipLaunchKernelGGL((mobile_rollout_k<SRLHIP_RNG_HOST, -1, -1>), grid, block, 0, h->stream, p, h->mobile, h->rng, h->stats,
                       1, d_actions, d_noise, d_obs, d_rew, d_done, 0, PersistArgs{});
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

// ---- persistent stepping, host side (api.hip: srlhip_set_persistent) --------------------------------------------------------------------
// the resident kernel of this handle: what the occupancy query asks about is what mobile_persist_start launches
static const void *mobile_persist_fn(const Handle *h, const MobileParams &p) {
    const void *fn = nullptr;
    dispatch_device_rng(h->cfg.rng_mode, [&](auto mode) {
        dispatch_env(p, [&](auto kind, auto disc) {
            fn = reinterpret_cast<const void *>(mobile_persist_k<decltype(mode)::value, decltype(kind)::value, decltype(disc)::value>);
        });
    });
    return fn;
}
// workgroups of the resident kernel (0: no persistent form for this handle); capacity: how many the device holds at once;
// eighths: which of the 8 `done` words it writes; grid: the workgroups it launches (all real)
static int mobile_persist_blocks(Handle *h, int *capacity, uint32_t *eighths, int *grid_out) {
    if (capacity) *capacity = 0;
    const srlhip_config &c = h->cfg;
    if (!(c.rng_mode == SRLHIP_RNG_PHILOX || c.rng_mode == SRLHIP_RNG_MT19937) || c.obs_mode == SRLHIP_OBS_RAW_PIXELS) return 0;
    const MobileParams p = params_of(h);
    const int grid = (h->n + kBlock - 1) / kBlock;
    int per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device_id) != hipSuccess) return 0;
    const void *fn = mobile_persist_fn(h, p);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlock, 0) != hipSuccess) return 0;
    if (capacity) *capacity = per_cu * prop.multiProcessorCount;
    if (eighths) *eighths = strided_eighths(grid);
    if (grid_out) *grid_out = grid;
    return (long long)per_cu * prop.multiProcessorCount >= grid ? grid : 0;
}
// (the kernel writes the host's planes)
static int mobile_persist_start(Handle *h, const void *d_actions, const PersistArgs &pa) {
    float *d_obs = reinterpret_cast<float *>(pa.host_out), *d_rew = reinterpret_cast<float *>(pa.host_out + pa.rew_dw);
    uint8_t *d_done = reinterpret_cast<uint8_t *>(pa.host_out + pa.done_dw);
    h->snap_valid = false; h->prefetch_valid = false;
    MobileParams p = params_of(h);
    const void *fn = mobile_persist_fn(h, p);
    if (!fn) return h->fail(SRLHIP_ENOTSUP, "persistent stepping: needs a device RNG mode (PHILOX or MT19937)");
    PersistArgs args_pa = pa;
    void *args[] = {&p, &h->mobile, &h->rng, &h->stats, &d_actions, &d_obs, &d_rew, &d_done, &args_pa};      // mobile_persist_k's parameters, in order
    SRL_HIP_CHECK(h, hipLaunchKernel(fn, dim3((h->n + kBlock - 1) / kBlock), dim3(kBlock), args, 0, h->stream));
    return 0;
}

static int mobile_field(Handle *h, int field, void **dptr, size_t *elem, int *count) {
    MobileState &s = h->mobile;
    *count = 1;
    switch (field) {
        case SRLHIP_F_POS_X: *dptr = s.pos_x; *elem = 8; return 0;
        case SRLHIP_F_POS_Y: *dptr = s.pos_y; *elem = 8; return 0;
        case SRLHIP_F_TARGET_X: *dptr = s.tgt_x; *elem = 8; return 0;
        case SRLHIP_F_TARGET_Y: *dptr = s.tgt_y; *elem = 8; return 0;
        case SRLHIP_F_TARGET2_X: *dptr = s.tgt2_x; *elem = 8; return 0;
        case SRLHIP_F_TARGET2_Y: *dptr = s.tgt2_y; *elem = 8; return 0;
        case SRLHIP_F_STEP_COUNT: *dptr = s.counter; *elem = 4; return 0;
        case SRLHIP_F_CUR_TARGET: *dptr = s.cur_target; *elem = 4; return 0;
    }
    return h->fail(SRLHIP_EINVAL, "unknown field for the MobileRobot family");
}

const EnvOps &mobile_env_ops() {
    static const EnvOps ops = {mobile_alloc, mobile_reset, mobile_step, mobile_rollout, mobile_rollout_policy, mobile_field, mobile_persist_blocks, mobile_persist_start};
    return ops;
}

}  // namespace srl
