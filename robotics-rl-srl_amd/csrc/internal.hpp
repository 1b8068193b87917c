// internal.hpp — handle layout shared by the C-ABI front end (api.hip) and the
// kernel translation units (mobile.hip, kuka.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/srlhip.h"
#include "rng.hpp"
#include "step_signal.hpp"

namespace srl {

// ---- per-env random-stream state (all modes allocated lazily) --------------
struct RngState {
    Mt19937View mt;        // RNG_MT19937
    uint32_t *key;         // [2][N] Philox key (seed lo, hi) — also the action stream in every mode
    uint64_t *ctr;         // [N] Philox block counter, env stream
    uint64_t *act_ctr;     // [N] Philox block counter, synthetic-agent action stream
};

// ---- episode accounting (bench.Monitor equivalent, environments/utils.py:54)
struct EpisodeStats {
    double *ep_return;       // running
    int32_t *ep_length;      // running
    double *last_return;     // of the most recently finished episode
    int32_t *last_length;
    int32_t *n_finished;
    double *last_reward;     // reward of the last step, uncast (f64)
};

// ---- MobileRobot family: SoA state, f64 exactly as the reference's numpy ---
struct MobileState {
    double *pos_x, *pos_y;       // robot_pos[:2]            (mobile_robot_env.py:97)
    double *tgt_x, *tgt_y;       // target_pos / button_pos[0]
    double *tgt2_x, *tgt2_y;     // button_pos[1]            (2Target only)
    int32_t *counter;            // _env_step_counter
    int32_t *cur_target;         // current_target           (2Target only)
};

struct MobileParams {
    int32_t kind, is_discrete, random_target, shape_reward, auto_reset;
    int32_t n;
};

// Everything mobile_rollout_ep_k's segment lanes read from the per-env state, as planes of their own (mobile.hip).  Passed to kernels
// BY VALUE.  An all-null set as a destination: write nowhere.
struct MobileSnapSet {
    MobileState s;
    uint64_t *ctr, *actr;        // rng.ctr, rng.act_ctr
    double *ep_return;           // stats.ep_return, stats.ep_length
    int32_t *ep_length;
};

struct Handle;

// mobile.hip
int mobile_alloc(Handle *h);
int mobile_reset(Handle *h, const uint8_t *d_mask, const double *d_host_rand, float *d_obs);
int mobile_step(Handle *h, const void *d_actions, const double *d_noise, float *d_obs, float *d_rew,
                uint8_t *d_done);
int mobile_rollout(Handle *h, int T, const void *d_actions, float *d_obs, float *d_rew, uint8_t *d_done,
                   void *d_act_out);
// srlhip_rollout_policy / srlhip_rollout_mlp_policy: the policy as the kernels take it (device pointers; mean / std null without
// normalisation).  hidden == 0: the linear policy, w = float64 [n][D][A] or [D][A]; hidden = H >= 1: the one-hidden-layer MLP,
// w = float32 [n][P] or [P], P = H D + H + A H + A.  Passed to kernels BY VALUE: the layout is part of their argument block.
struct PolicyArgs {
    const void *w;
    const double *mean, *std;
    double clip;
    int32_t per_env, freeze, normalize, hidden;
};
static_assert(sizeof(PolicyArgs) == 48 && offsetof(PolicyArgs, w) == 0 && offsetof(PolicyArgs, mean) == 8 && offsetof(PolicyArgs, std) == 16 &&
                  offsetof(PolicyArgs, clip) == 24 && offsetof(PolicyArgs, per_env) == 32 && offsetof(PolicyArgs, freeze) == 36 &&
                  offsetof(PolicyArgs, normalize) == 40 && offsetof(PolicyArgs, hidden) == 44,
              "PolicyArgs is a kernel argument: its layout is what the policy kernels were compiled against");
// mobile.hip: the linear or the MLP kernel family by pol.hidden; sample: the MLP's discrete action drawn from the softmax of its scores
int mobile_rollout_policy(Handle *h, int T, const PolicyArgs &pol, bool sample, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out);
// kuka_tree_policy.hip / kuka_tree_mlp.hip / kuka_tree_mlp_sample.hip (full model); d_hdr: the handle's 16-double policy header
int kuka_rollout_policy(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out);
int kuka_rollout_mlp_policy(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out);
int kuka_rollout_mlp_policy_sampled(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out);
int kuka_policy_header(Handle *h, double *d_hdr, const PolicyArgs &pol);      // kuka_tree_policy.hip: the one header kernel's launch
// policy_act.hip: srlhip_policy_act behind its argument checks — one launch on the handle's stream, no allocation, no synchronisation.
// D = floats per row of obs, A = scores per env; none_nan: a frozen env's continuous row is NaNs (Kuka), not zeros (MobileRobot)
int policy_act_launch(Handle *h, const PolicyArgs &pol, bool sample, int D, int A, bool none_nan, const float *d_obs, const uint8_t *d_done_prev,
                      uint8_t *d_frozen, void *d_act, double *d_score);
int mobile_field(Handle *h, int field, void **dptr, size_t *elem, int *count);
int mobile_reset_rand_count(const srlhip_config &c);
int mobile_persist_blocks(Handle *h, int *capacity, uint32_t *eighths);      // persistent stepping (mobile.hip)
int mobile_persist_start(Handle *h, const void *d_actions, float *d_obs, float *d_rew, uint8_t *d_done, const PersistArgs &pa);

// kuka.hip
int kuka_alloc(Handle *h);
void kuka_free(Handle *h);
int kuka_reset(Handle *h, const uint8_t *d_mask, const double *d_host_rand, void *d_obs);
int kuka_step(Handle *h, const void *d_actions, const double *d_noise, void *d_obs, float *d_rew,
              uint8_t *d_done);
int kuka_rollout(Handle *h, int T, const void *d_actions, void *d_obs, float *d_rew, uint8_t *d_done,
                 void *d_act_out);
int kuka_field(Handle *h, int field, void **dptr, size_t *elem, int *count);
int kuka_reset_rand_count(const srlhip_config &c);
int kuka_refresh(Handle *h);
int kuka_uses_group_kernel(const Handle *h);
int kuka_set_model(Handle *h, const double *table138);
void kuka_default_model(double *table138);
int kuka_set_tree_model(Handle *h, const double *table510);
void kuka_default_tree_model(double *table510);
int kuka_group_probe(const double *q7_host, double *out_host, int out_doubles);
// api.hip: the launch of srlhip_seed's MT19937 seeding kernel (digits [2][n], len [n]: device pointers; mask may be null)
hipError_t mt_seed_launch(const Mt19937View &v, int n, const uint8_t *d_mask, const uint32_t *d_digits, const int32_t *d_len, hipStream_t stream);
// rng_probe.hip: srlhip_selftest_rng (host pointers)
int rng_probe_run(int generator, int stream, int n, int stride, const uint32_t *keys, const int32_t *key_len, const uint8_t *mask,
                  const uint64_t *state_in, const int32_t *script, int n_ops, const double *args, int n_args, const int32_t *skip,
                  uint64_t *out, int64_t out_words, uint64_t *state_out, int64_t state_words);
int kuka_persist_blocks(Handle *h, int *capacity);   // persistent stepping: real workgroups of the resident kernel (0: this handle has no persistent form); capacity: how many the device holds at once
int kuka_persist_start(Handle *h, const void *d_actions, float *d_obs, float *d_rew, uint8_t *d_done, const PersistArgs &pa);

// raster.hip
int raster_render(Handle *h, void *d_img);
// What the rasteriser sees of a Kuka handle (filled by kuka.hip::kuka_raster_view, passed BY VALUE to raster.hip's kernels — one
// definition, so that the two translation units cannot drift apart): raw plane pointers (sq / cq: [7][n] ...), gj = the five gripper
// joints of the installed full-model table (parent, frame in the parent link, axis), grip = raster_grip_k's output planes
// ([42][n]: gripper capsule end points, then the arm's joint origins); has_tm = 0 on lumped handles.
struct RasterGripJoint { double parent, xyz[3], Rj[9], axis[3]; };
struct RasterKukaView { const double *sq, *cq, *bq, *bx, *by, *bz, *b2q, *b2x, *b2y, *objs, *rb, *gsq, *gcq; RasterGripJoint gj[5]; const float *grip; int64_t n; int32_t two, rand_objects, has_tm; };

// jpeg.hip: srlhip_jpeg_encode behind its argument checks: three launches on `stream`, no allocation, no synchronisation (0 or SRLHIP_E*)
int jpeg_encode_launch(const uint8_t *images_dev, int n, int img_h, int img_w, int n_channels, int quality, uint8_t *blob_dev,
                       int64_t cap_per_stream, int64_t *offsets_dev, int32_t *overflow_dev, hipStream_t stream);

struct KukaState;   // defined in kuka.hip

struct Handle {
    srlhip_config cfg;
    int n;
    hipStream_t stream;
    hipEvent_t ev_begin, ev_end;
    std::string err;
    RngState rng;
    EpisodeStats stats;
    MobileState mobile;
    // Two snapshot sets in turn.  A rollout launch reads set snap_cur — a lane may start after the lane that writes its env's final
    // state has retired, so the lanes never read the live state — and the lane that leaves an env's final state also writes it into the
    // other set, which the next launch reads: back-to-back rollouts need no mobile_snapshot_k launch.  snap_valid = set snap_cur equals
    // the live state (cleared by everything else that touches the state)
    MobileSnapSet snap[2] = {};
    int snap_cur = 0;
    bool snap_valid = false;
    // synthetic-agent rollouts of the MobileRobot family: the [T][N] action plane of the NEXT rollout is drawn by spare workgroups
    // of the current rollout's launch (mobile_rollout_ep_k), from the action-stream counters in the snapshot; two planes in turn
    void *act_plane[2] = {nullptr, nullptr};
    size_t act_plane_sz[2] = {0, 0};
    bool prefetch_valid = false;
    int prefetch_T = 0, prefetch_buf = 0;
    KukaState *kuka;
    double kuka_tmodel_host[510] = {0};   // host copy of the installed full-model table (srlhip_kuka_tree_model): the rasteriser's gripper joint frames
    std::vector<void *> allocs;      // everything hipMalloc'ed for this handle
    // staging buffers for io_device == 0
    void *st_actions, *st_noise, *st_obs, *st_rew, *st_done, *st_mask, *st_rand;
    size_t st_actions_sz, st_noise_sz, st_obs_sz, st_rew_sz, st_done_sz, st_mask_sz, st_rand_sz;
    // rasteriser: per fixed camera, the unit ray of every pixel + depth / colour of the static scenery behind it
    // (built lazily on the first render; lives in `allocs`)
    float4 *raster_rays[2];
    uint32_t *raster_bg[2];
    float *raster_grip = nullptr;         // [42][n] full Kuka model: the gripper capsules' end points, then the arm's joint origins (raster_grip_k, refreshed by every render)
    void *st_jpeg = nullptr;         // srlhip_render_jpeg on a host-pointer handle: blob, then offsets, then overflow flags (grow-only)
    size_t st_jpeg_sz = 0;
    void *pin_in, *pin_out;          // pinned host bounce buffers of srlhip_step (host-pointer mode)
    // host-pointer handles (io_device = 0): stats.last_return / last_length live in ONE mapped pinned host block ([n] f64, then [n] i32)
    // that the kernels address directly, so the per-step API reads an ended episode's (r, l) without a device copy (srlhip_episode_records)
    void *ep_host = nullptr;
    size_t pin_in_sz, pin_out_sz;
    bool step_pending = false;       // srlhip_step_async enqueued a step that srlhip_step_wait has not collected yet
    // persistent stepping (step_signal.hpp): the mapped control block (PersistHost) and the device words
    bool persist_on = false, persist_running = false, persist_step = false;
    void *persist_host = nullptr;
    uint32_t *persist_relay = nullptr;
    void *persist_stage = nullptr;
    uint32_t persist_seq = 0, persist_blocks = 0, persist_park_us = 2000;
    // early completion signal of single-step launches (host_step_begin / host_step_finish): step_signal.done is set while host_step_begin's
    // launch is under way; a launcher whose kernel supports the signal passes it on and arms it
    PersistArgs step_signal = {};
    bool step_signal_armed = false, signal_wait = false;
    uint32_t signal_seq = 0, signal_steps = 0, signal_fallbacks = 0;
    uint32_t signal_eighths = 0;     // which of the 8 `done` words the armed launch will write (set by the launcher)
    uint32_t persist_eighths = 0;    // which of the 8 `done` words the resident kernel writes
    int persist_reserved = 0;        // workgroups this handle holds in the per-device residency tally (api.hip)
    double *policy_hdr = nullptr;    // srlhip_rollout_policy on a Kuka handle: the scalars its kernel reads (allocated with the handle: the call may be captured)

    int fail(int code, const std::string &msg) { err = msg; return code; }
    template <class T>
    int dalloc(T **p, size_t count) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
        if (e != hipSuccess) return fail(SRLHIP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        e = hipMemsetAsync(q, 0, count * sizeof(T), stream);
        if (e != hipSuccess) return fail(SRLHIP_EHIP, std::string("hipMemset: ") + hipGetErrorString(e));
        allocs.push_back(q);
        *p = static_cast<T *>(q);
        return 0;
    }
};

#define SRL_HIP_CHECK(h, expr)                                                                     \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return (h)->fail(SRLHIP_EHIP, std::string(#expr ": ") + hipGetErrorString(e__));       \
    } while (0)

// Run-time configuration -> template arguments: f is a generic lambda that receives the matching value as a std::integral_constant
// and launches (or names) the instantiation it selects; only the values listed exist in the library.  Returns whether an arm matched
// — all the way down when f itself returns the bool of a nested dispatch.  A launcher answers false with SRLHIP_ENOTSUP: a value
// without an arm must not pass for a launch (hipGetLastError() after launching nothing reports success).
template <int V> using Const = std::integral_constant<int, V>;
template <class F, class C>
bool dispatch_arm_matched(F &f, C c) {
    if constexpr (std::is_void_v<decltype(f(c))>) { f(c); return true; }
    else return f(c);
}
template <int... Vs, class F>
bool dispatch_int(int v, F &&f) { return (((v == Vs) && dispatch_arm_matched(f, Const<Vs>{})) || ...); }

// a grow-only device buffer: at least `bytes` at *buf afterwards (contents are not kept; the caller orders the free against the stream)
inline int ensure(Handle *h, void **buf, size_t *cap, size_t bytes) {
    if (*cap >= bytes) return 0;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    SRL_HIP_CHECK(h, hipMalloc(buf, bytes));
    *cap = bytes;
    return 0;
}

inline int obs_dim_of(const srlhip_config &c) {
    switch (c.env_kind) {
        case SRLHIP_ENV_MOBILE_1D: return 1;
        case SRLHIP_ENV_MOBILE: case SRLHIP_ENV_MOBILE_2TARGET: case SRLHIP_ENV_MOBILE_LINE: return 2;
        case SRLHIP_ENV_KUKA_BUTTON: case SRLHIP_ENV_KUKA_MOVING: case SRLHIP_ENV_KUKA_2BUTTON: case SRLHIP_ENV_KUKA_RAND:
            return c.obs_mode == SRLHIP_OBS_JOINTS ? 14 : c.obs_mode == SRLHIP_OBS_JOINTS_POSITION ? 17 : 3;
    }
    return 0;
}
inline int num_actions_of(const srlhip_config &c) {
    if (!c.is_discrete) return 0;
    switch (c.env_kind) {
        case SRLHIP_ENV_MOBILE_1D: return 2;
        case SRLHIP_ENV_KUKA_BUTTON: case SRLHIP_ENV_KUKA_MOVING: case SRLHIP_ENV_KUKA_2BUTTON: case SRLHIP_ENV_KUKA_RAND: return 6;
        default: return 4;
    }
}
inline int action_dim_of(const srlhip_config &c) {
    if (c.is_discrete) return 1;
    if (c.env_kind >= SRLHIP_ENV_KUKA_BUTTON) return c.action_joints ? 7 : 3;
    return 2;
}

}  // namespace srl
