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
#include "api_rules.hpp"
#include "rng.hpp"
#include "step_signal.hpp"

namespace srl {

// ---- per-env random-stream state (all modes allocated lazily) --------------
struct RngState {
    Mt19937View mt = {};             // RNG_MT19937
    uint32_t *key = nullptr;         // [2][N] Philox key (seed lo, hi) — also the action stream in every mode
    uint64_t *ctr = nullptr;         // [N] Philox block counter, env stream
    uint64_t *act_ctr = nullptr;     // [N] Philox block counter, synthetic-agent action stream
};

// ---- episode accounting (bench.Monitor equivalent, environments/utils.py:54)
struct EpisodeStats {
    double *ep_return = nullptr;       // running
    int32_t *ep_length = nullptr;      // running
    double *last_return = nullptr;     // of the most recently finished episode
    int32_t *last_length = nullptr;
    int32_t *n_finished = nullptr;
    double *last_reward = nullptr;     // reward of the last step, uncast (f64)
};

// ---- MobileRobot family: SoA state, f64 exactly as the reference's numpy ---
struct MobileState {
    double *pos_x = nullptr, *pos_y = nullptr;       // robot_pos[:2]            (mobile_robot_env.py:97)
    double *tgt_x = nullptr, *tgt_y = nullptr;       // target_pos / button_pos[0]
    double *tgt2_x = nullptr, *tgt2_y = nullptr;     // button_pos[1]            (2Target only)
    int32_t *counter = nullptr;                      // _env_step_counter
    int32_t *cur_target = nullptr;                   // current_target           (2Target only)
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
// srlhip_rollout_policy_summary: the reduced outputs of a fused policy rollout (device pointers; include/srlhip.h has the contract).  The
// launchers below take a pointer to one: null is the plane call, non-null the summary call — no plane is written then, and a refusal
// carries the summary entry's name.  length, and obs_sum with obs_sqsum, may be null.
struct SummaryOut {
    double *ret;
    int32_t *length;
    double *obs_sum, *obs_sqsum;
};
constexpr const char *kSummaryName = "rollout_policy_summary";
// kuka_tree_policy.hip / kuka_tree_mlp.hip / kuka_tree_mlp_sample.hip / kuka_tree_policy_sample.hip (full model); d_hdr: the handle's 16-double policy header
int kuka_rollout_policy(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum);
int kuka_rollout_mlp_policy(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum);
int kuka_rollout_mlp_policy_sampled(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum);
int kuka_rollout_policy_sampled(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum);      // kuka_tree_policy_sample.hip
using KukaPolicyLaunch = int (*)(Handle *, int, const PolicyArgs &, double *, float *, float *, uint8_t *, void *, const SummaryOut *);
int kuka_policy_header(Handle *h, double *d_hdr, const PolicyArgs &pol, const SummaryOut *sum);      // kuka_tree_policy.hip: the one header kernel's launch

// What api.hip asks of an env family, one table per family (mobile.hip, kuka.hip); every pointer is a device pointer.
struct EnvOps {
    int (*alloc)(Handle *h);
    int (*reset)(Handle *h, const uint8_t *d_mask, const double *d_host_rand, void *d_obs);
    int (*step)(Handle *h, const void *d_actions, const double *d_noise, void *d_obs, float *d_rew, uint8_t *d_done);
    int (*rollout)(Handle *h, int T, const void *d_actions, void *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out);
    // the fused policy rollouts.  MobileRobot: the linear or the MLP kernel family by pol.hidden, with `sample` the discrete action
    // drawn from the softmax of its scores; Kuka: `kuka`, the launcher api.hip's PolicyCall names, on the handle's policy header
    // sum: null, or the outputs of srlhip_rollout_policy_summary (the four planes are null then)
    int (*rollout_policy)(Handle *h, int T, const PolicyArgs &pol, bool sample, KukaPolicyLaunch kuka, void *d_obs, float *d_rew, uint8_t *d_done, void *d_act_out,
                          const SummaryOut *sum);
    int (*field)(Handle *h, int field, void **dptr, size_t *elem, int *count);
    // persistent stepping: the real workgroups of the resident kernel (0: this handle has no persistent form); capacity: how many
    // workgroups of it the device holds at once; eighths: which of the 8 `done` words it writes; grid: the workgroups it launches
    int (*persist_blocks)(Handle *h, int *capacity, uint32_t *eighths, int *grid);
    // launch the resident kernel: MobileRobot's writes the host's planes (pa.host_out), the Kuka kernels take the staging copy
    // (Handle::persist_stage) and switch to the host's planes themselves; the reward / done planes start pa.rew_dw / pa.done_dw dwords in
    int (*persist_start)(Handle *h, const void *d_actions, const PersistArgs &pa);
};
const EnvOps &mobile_env_ops();      // mobile.hip
const EnvOps &kuka_env_ops();        // kuka.hip
// policy_act.hip: the finishing step's arguments (policy_act.hpp: ActFinish; its users include that header) as the three action launchers
// below fill them.  A sampled call moves the action-stream counters past what was drawn ahead: snap_valid and prefetch_valid fall here
struct ActFinish;
ActFinish act_finish_args(Handle *h, bool freeze, bool sample, int A, bool none_nan, const uint8_t *d_done_prev, uint8_t *d_frozen, void *d_act);
// policy_act.hip: srlhip_policy_act behind its argument checks — one launch on the handle's stream, no allocation, no synchronisation.
// D = floats per row of obs, A = scores per env; none_nan: a frozen env's continuous row is NaNs (Kuka), not zeros (MobileRobot)
int policy_act_launch(Handle *h, const PolicyArgs &pol, bool sample, int D, int A, bool none_nan, const float *d_obs, const uint8_t *d_done_prev,
                      uint8_t *d_frozen, void *d_act, double *d_score);
// policy_act.hip: srlhip_sample_actions behind its argument checks — one launch on the handle's stream, no allocation, no synchronisation.
// d_score: float64 [n][A], A = the handle's num_actions; d_frozen: uint8 [n] or null
int sample_actions_launch(Handle *h, int A, const double *d_score, const uint8_t *d_frozen, int32_t *d_act);
// cnn_policy.hip: srlhip_cnn_policy_act behind its argument checks — one launch on the handle's stream, no allocation, no synchronisation.
// The frame shape is the handle's config's; A = scores per env; none_nan as above
int cnn_policy_act_launch(Handle *h, const float *d_params, bool per_env, bool freeze, bool sample, int A, bool none_nan, const uint8_t *d_images,
                          const uint8_t *d_done_prev, uint8_t *d_frozen, void *d_act, float *d_score);
// pixel_policy.hip: srlhip_pixel_policy_act behind its argument checks — one launch on the handle's stream, no allocation, no synchronisation.  D = the handle's frame bytes; d_delta null
// unless paired; A, none_nan as above
int pixel_policy_act_launch(Handle *h, const double *d_weights, const double *d_delta, double noise, bool paired, bool freeze, int A, bool none_nan,
                            const uint8_t *d_images, const uint8_t *d_done_prev, uint8_t *d_frozen, void *d_act, double *d_score);

// kuka.hip
void kuka_free(Handle *h);
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

// Grow-only buffers of a handle (ensure / ensure_pinned: contents are not kept across a regrow).  Device memory ...
struct DevBuf { void *p = nullptr; size_t cap = 0; };
// ... and mapped, coherent pinned host memory
struct PinBuf { void *p = nullptr; size_t cap = 0; };
// staging buffers of the host-pointer calls (io_device == 0).  ST_NOISE: the MT19937 key lengths of srlhip_seed, the synthetic agent's
// action plane (mobile.hip); ST_RAND: reset draws, seed words, a policy's packed block; ST_JPEG: srlhip_render_jpeg's scratch
// (api_rules.hpp: JpegScratch; device-pointer handles: the frames).  srlhip_destroy frees the whole array.
enum StageBuf { ST_ACTIONS, ST_NOISE, ST_OBS, ST_REW, ST_DONE, ST_MASK, ST_RAND, ST_JPEG, ST_COUNT };
enum PinnedBuf { PIN_IN, PIN_OUT, PIN_COUNT };      // the two bounce buffers of srlhip_step (api_rules.hpp: StepLayout)

// Every member has its initial value here: srlhip_create fills in what it creates, srlhip_destroy releases whatever is set.
struct Handle {
    srlhip_config cfg = {};
    int n = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
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
    DevBuf act_plane[2];
    bool prefetch_valid = false;
    int prefetch_T = 0, prefetch_buf = 0;
    KukaState *kuka = nullptr;
    double kuka_tmodel_host[510] = {0};   // host copy of the installed full-model table (srlhip_kuka_tree_model): the rasteriser's gripper joint frames
    std::vector<void *> allocs;      // everything hipMalloc'ed for this handle
    DevBuf st[ST_COUNT];
    // rasteriser: per fixed camera, the unit ray of every pixel + depth / colour of the static scenery behind it
    // (built lazily on the first render; lives in `allocs`)
    float4 *raster_rays[2] = {nullptr, nullptr};
    uint32_t *raster_bg[2] = {nullptr, nullptr};
    float *raster_grip = nullptr;         // [42][n] full Kuka model: the gripper capsules' end points, then the arm's joint origins (raster_grip_k, refreshed by every render)
    PinBuf pin[PIN_COUNT];
    // host-pointer handles (io_device = 0): stats.last_return / last_length live in ONE mapped pinned host block (api_rules.hpp:
    // episode_returns / episode_lengths) that the kernels address directly, so the per-step API reads an ended episode's (r, l) without
    // a device copy (srlhip_episode_records)
    void *ep_host = nullptr;
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
    // srlhip_pixel_policy_act on a small population (raw-pixel device-pointer handles; allocated with the handle: the call may be captured):
    // the chunk sums of its split launch and one ticket word per work item (api_rules.hpp: kPixSplit*)
    double *pix_part = nullptr;
    uint32_t *pix_ticket = nullptr;
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

// a grow-only device buffer: at least `bytes` at b.p afterwards (contents are not kept; the caller orders the free against the stream)
inline int ensure(Handle *h, DevBuf &b, size_t bytes) {
    if (b.cap >= bytes) return 0;
    if (b.p) (void)hipFree(b.p);
    b = DevBuf{};
    SRL_HIP_CHECK(h, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return 0;
}

inline const EnvOps &env_ops(const Handle *h) { return is_mobile(h->cfg.env_kind) ? mobile_env_ops() : kuka_env_ops(); }

}  // namespace srl
