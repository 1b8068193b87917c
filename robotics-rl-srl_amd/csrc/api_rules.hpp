// api_rules.hpp — everything the C-ABI front end (api.hip) decides from a config or from caller data alone, as pure functions: shapes and
// byte counts, what srlhip_create accepts, the step buffers' plane offsets, the checks of host-pointer actions, model tables and policy
// structs, the scratch layouts.  Plain C++17, no HIP, no Handle: csrc/api_rules_hostcheck.cpp runs it on the CPU (plain and under the
// sanitizers), tests/test_api_rules_cpu.py holds every line it prints to the rules restated in Python.  Not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/srlhip.h"

namespace srl {

// a check's answer: code 0 = accepted (msg null), else the SRLHIP_E* code and the message (or, for the policy checks, its tail)
struct Verdict { int code; const char *msg; };
constexpr Verdict kAccepted{0, nullptr};

// ---- kinds and shapes -------------------------------------------------------------------------------------------------------------------
inline bool is_mobile(int kind) { return kind >= SRLHIP_ENV_MOBILE && kind <= SRLHIP_ENV_MOBILE_LINE; }
inline bool is_kuka(int kind) { return kind >= SRLHIP_ENV_KUKA_BUTTON && kind <= SRLHIP_ENV_LAST; }

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
// one rendered frame of one env: u8 [H][W][3], a second camera's three channels behind the first's with multi_view
inline size_t frame_bytes(const srlhip_config &c) { return (size_t)c.img_h * c.img_w * (c.multi_view ? 6 : 3); }
inline size_t obs_bytes_per_env(const srlhip_config &c) {
    return c.obs_mode == SRLHIP_OBS_RAW_PIXELS ? frame_bytes(c) : sizeof(float) * obs_dim_of(c);
}
// one [n] plane of actions: i32 indices, or f32 rows of action_dim
inline size_t action_bytes(const srlhip_config &c, size_t n) { return n * (c.is_discrete ? sizeof(int32_t) : sizeof(float) * action_dim_of(c)); }
// scores a policy produces per env
inline size_t policy_outputs(const srlhip_config &c) { return (size_t)(c.is_discrete ? num_actions_of(c) : action_dim_of(c)); }
// uniform draws one env's reset consumes (RNG_HOST: doubles per env in host_rand)
inline int reset_rand_count(const srlhip_config &c) {
    if (is_mobile(c.env_kind)) {
        const int base = c.env_kind == SRLHIP_ENV_MOBILE_1D ? 1 : 2;
        if (!c.random_target) return base;
        switch (c.env_kind) {
            case SRLHIP_ENV_MOBILE_1D: case SRLHIP_ENV_MOBILE_LINE: return base + 1;
            case SRLHIP_ENV_MOBILE_2TARGET: return base + 4;
            default: return base + 2;
        }
    }
    const int init = c.is_discrete ? 10 : 5;
    if (c.env_kind == SRLHIP_ENV_KUKA_2BUTTON) return (c.random_target ? 4 : 0) + 2 + init;   // kuka_2button_gym_env.py:55-70
    return (c.env_kind == SRLHIP_ENV_KUKA_MOVING ? 1 : 0) + (c.random_target ? 2 : 0) + (c.env_kind == SRLHIP_ENV_KUKA_RAND ? 20 : 0) + init;
}

// ---- config -----------------------------------------------------------------------------------------------------------------------------
// srlhip_default_config behind its argument check (env_kind is one of the eight)
inline void fill_default_config(int32_t env_kind, srlhip_config *cfg) {
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = (int32_t)sizeof *cfg;
    cfg->env_kind = env_kind;
    cfg->num_envs = 1;
    cfg->is_discrete = 1;
    cfg->force_down = 1;
    cfg->action_repeat = 1;
    cfg->obs_mode = SRLHIP_OBS_GROUND_TRUTH;
    cfg->img_h = cfg->img_w = 224;                                  // RENDER_HEIGHT/WIDTH
    cfg->rng_mode = SRLHIP_RNG_MT19937;
    cfg->auto_reset = 1;
    cfg->max_distance = is_kuka(env_kind) ? 0.8 : 1.6;              // ctor defaults
    if (env_kind == SRLHIP_ENV_KUKA_2BUTTON) { cfg->max_distance = 2.0; cfg->force_down = 0; }   // kuka_2button_gym_env.py:29
    // every Kuka env integrates the full arm + gripper model on the tree lane-group kernel (Kuka2Button: its two-button form)
    cfg->kuka_model = is_kuka(env_kind) ? SRLHIP_KUKA_MODEL_FULL : SRLHIP_KUKA_MODEL_LUMPED;
}

// what srlhip_create refuses before it touches a device, in the order it refuses it
inline Verdict check_config(const srlhip_config &c) {
    if (c.struct_size != (int32_t)sizeof(srlhip_config)) return {SRLHIP_EINVAL, "create: srlhip_config.struct_size mismatch (ABI)"};
    if (c.num_envs <= 0) return {SRLHIP_EINVAL, "create: num_envs must be positive"};
    if (!is_mobile(c.env_kind) && !is_kuka(c.env_kind)) return {SRLHIP_EINVAL, "create: unknown env_kind"};
    if (c.rng_mode < SRLHIP_RNG_HOST || c.rng_mode > SRLHIP_RNG_MT19937) return {SRLHIP_EINVAL, "create: unknown rng_mode"};
    if (c.auto_reset && c.rng_mode == SRLHIP_RNG_HOST) return {SRLHIP_EINVAL, "create: auto_reset needs a device RNG mode"};
    // mobile_robot_1D_env.py:44, mobile_robot_2target_env.py:128-129 raise ValueError
    if (!c.is_discrete && (c.env_kind == SRLHIP_ENV_MOBILE_1D || c.env_kind == SRLHIP_ENV_MOBILE_2TARGET))
        return {SRLHIP_ENOTSUP, "Only discrete actions is supported"};
    if (is_mobile(c.env_kind) && c.obs_mode != SRLHIP_OBS_GROUND_TRUTH && c.obs_mode != SRLHIP_OBS_RAW_PIXELS)
        return {SRLHIP_EINVAL, "create: MobileRobot envs support ground_truth / raw_pixels only"};
    // every obs_mode: srlhip_render() also serves ground-truth handles (dataset_generator --img-size), and the rasteriser's
    // LDS band holds one image row of at most 2048 pixels
    if (c.img_h < 8 || c.img_w < 8 || c.img_h > 1024 || c.img_w > 1024) return {SRLHIP_EINVAL, "create: img_h / img_w must be in [8, 1024]"};
    if (is_kuka(c.env_kind) && c.kuka_model != SRLHIP_KUKA_MODEL_LUMPED && c.kuka_model != SRLHIP_KUKA_MODEL_FULL)
        return {SRLHIP_EINVAL, "create: unknown kuka_model"};
    if (c.info_bits != 0 && c.info_bits != 1) return {SRLHIP_EINVAL, "create: info_bits must be 0 or 1"};
    if (is_kuka(c.env_kind) && c.action_repeat < 1) return {SRLHIP_EINVAL, "create: action_repeat must be >= 1"};
    return kAccepted;
}

// ---- the host-pointer step's buffers ----------------------------------------------------------------------------------------------------
// Small steps (ground-truth observations of a few thousand envs: < 1 MiB each way) are ZERO-COPY: the kernel reads the actions from
// and writes obs / reward / done to mapped pinned host memory over PCIe, so a step is one launch + one stream sync (measured ~10 us
// faster per 4096-env step than enqueueing an H2D and a D2H copy).  Larger steps (images, very large batches): one pinned bounce
// buffer each way -> one H2D and one D2H DMA transfer.
// in: [actions | pad to 16 | noise f64 [n]]; out: [obs | pad to 16 | reward f32 [n] | done u8 [n]].  The ONE definition of these offsets:
// the host's copies, the staging buffers and the resident kernel (PersistArgs::rew_dw / done_dw) all address the planes through it.
struct StepLayout { size_t ob, ab, in_noise, in_total, out_rew, out_done, out_total; bool pixels, zero_copy; };
constexpr size_t kZeroCopyMaxBytes = (size_t)1 << 20;
inline size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
inline StepLayout step_layout(const srlhip_config &c, size_t n, bool zero_copy_enabled) {
    StepLayout L;
    L.ob = obs_bytes_per_env(c) * n; L.ab = action_bytes(c, n);
    L.in_noise = pad16(L.ab); L.in_total = L.in_noise + sizeof(double) * n;
    L.out_rew = pad16(L.ob); L.out_done = L.out_rew + 4 * n; L.out_total = L.out_done + n;
    L.pixels = c.obs_mode == SRLHIP_OBS_RAW_PIXELS;
    L.zero_copy = zero_copy_enabled && !c.io_device && !L.pixels && L.out_total <= kZeroCopyMaxBytes;
    return L;
}

// ---- caller data ------------------------------------------------------------------------------------------------------------------------
// Host-pointer calls validate what the kernels cannot afford to: the full-model Kuka kernels are compiled with -fno-honor-nans, so a NaN
// or an infinity in a continuous action or in host-drawn noise would propagate through the step unchecked (the reference's
// np.clip / pybullet would raise or saturate).  Device-pointer callers own their buffers' contents.
// This header is also seen by those -fno-honor-nans units (through internal.hpp), and an inline function has ONE copy per library,
// whichever unit's the linker keeps: the classification reads the exponent bits, which no floating-point flag can fold away.
inline bool finite_f32(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return (u & 0x7f800000u) != 0x7f800000u; }
inline bool nan_f32(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return (u & 0x7fffffffu) > 0x7f800000u; }
inline bool finite_f64(double x) { uint64_t u; memcpy(&u, &x, sizeof u); return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
inline bool all_finite_f32(const float *p, size_t count) { for (size_t i = 0; i < count; i++) if (!finite_f32(p[i])) return false; return true; }
inline bool all_finite_f64(const double *p, size_t count) { for (size_t i = 0; i < count; i++) if (!finite_f64(p[i])) return false; return true; }
// Continuous actions of a Kuka handle, rows of `dim`: every row all finite, or all NaN (the reference's `None`, include/srlhip.h).
// One pass; a partly NaN row and any infinity fail.
inline bool kuka_rows_ok(const float *p, size_t rows, int dim) {
    for (size_t r = 0; r < rows; r++, p += dim) {
        int fin = 0, nan = 0;
        for (int j = 0; j < dim; j++) { fin += finite_f32(p[j]) ? 1 : 0; nan += nan_f32(p[j]) ? 1 : 0; }
        if (fin != dim && nan != dim) return false;
    }
    return true;
}
// the host-pointer check of a continuous action plane: MobileRobot takes finite values only (its step has no `None` branch for
// continuous actions: `action[0]` on None raises), Kuka finite or NaN rows
inline bool continuous_actions_ok(const srlhip_config &c, const float *p, size_t rows) {
    const int dim = action_dim_of(c);
    return is_mobile(c.env_kind) ? all_finite_f32(p, rows * (size_t)dim) : kuka_rows_ok(p, rows, dim);
}
// Discrete actions, copied and range-checked in one pass (all n are copied either way): the reference indexes a per-action list
// (`[-dv, dv, 0, 0, 0, 0][action]`) — an IndexError in its worker; -1 is its `None` action.  (Checked on the host so that the per-step
// Python path needs no reductions over the batch.)
inline bool copy_discrete_checked(const int32_t *src, int32_t *dst, size_t n, int32_t top) {
    int32_t bad = 0;
    for (size_t i = 0; i < n; i++) { const int32_t a = src[i]; dst[i] = a; bad |= (a < -1) | (a >= top); }
    return !bad;
}

// srlhip_set_kuka_model's table.  (static, like the next one: the negated comparisons are what refuses a NaN, so the copy api.hip calls
// must be the one compiled with api.hip's flags)
static inline Verdict check_kuka_model(const srlhip_kuka_model &m) {
    for (int i = 0; i < 7; i++)
        if (!(m.mass[i] > 0.0) || !(m.inertia[i][0] > 0.0) || !(m.inertia[i][1] > 0.0) || !(m.inertia[i][2] > 0.0) || !(m.joint_lower[i] < m.joint_upper[i]))
            return {SRLHIP_EINVAL, "set_kuka_model: masses and principal inertias must be positive, joint_lower < joint_upper"};
    return kAccepted;
}
// srlhip_set_kuka_tree_model's table
static inline Verdict check_kuka_tree_model(const srlhip_kuka_tree_model &m) {
    const int nd = (int)m.nd, ns = (int)m.nsphere;
    if (nd != 12 || ns < 0 || ns > 16 || (int)m.max_generic_rows < 0 || (int)m.max_generic_rows > 6 || (int)m.ee_link != 6 || (int)m.grip_link < 0 || (int)m.grip_link >= nd)
        return {SRLHIP_EINVAL, "set_kuka_tree_model: 12 DoFs, <= 16 spheres, end effector = link 6, max_generic_rows <= 6 (the lane group's row bank)"};
    for (int i = 0; i < nd; i++) {
        const srlhip_kuka_tree_joint &J = m.j[i];
        const double a2 = J.axis[0] * J.axis[0] + J.axis[1] * J.axis[1] + J.axis[2] * J.axis[2];
        if (!((int)J.parent < i && (int)J.parent >= -1) || !(J.mass > 0) || !(J.inertia[0] > 0 && J.inertia[3] > 0 && J.inertia[5] > 0) ||
            !(a2 > 0.999999 && a2 < 1.000001) || !(J.max_force > 0) || !(J.kp > 0))
            return {SRLHIP_EINVAL, "set_kuka_tree_model: parents before children, positive masses / inertias / motor gains, unit axes"};
        if (i < 7 && ((int)J.parent != i - 1)) return {SRLHIP_EINVAL, "set_kuka_tree_model: DoFs 0..6 must be the serial arm"};
    }
    const int detail = (int)m.solver_detail;
    if (m.solver_detail != (double)detail || detail < 0 || detail > (SRLHIP_KUKA_DETAIL_ALT_SWEEP | SRLHIP_KUKA_DETAIL_BODY_ORDER | SRLHIP_KUKA_DETAIL_FRICTION2) ||
        !(m.contact_erp >= 0.0 && m.contact_erp <= 1.0) || !(m.limit_erp >= 0.0 && m.limit_erp <= 1.0) || !(m.linear_slop >= 0.0 && m.linear_slop <= 0.01))
        return {SRLHIP_EINVAL, "set_kuka_tree_model: solver_detail is a mask of SRLHIP_KUKA_DETAIL_* bits, erp values in [0, 1], linear_slop in [0, 0.01]"};
    for (int k = 0; k < ns; k++)
        if ((int)m.s[k].link < 0 || (int)m.s[k].link >= nd || !(m.s[k].r > 0)) return {SRLHIP_EINVAL, "set_kuka_tree_model: bad sphere"};
    return kAccepted;
}

// ---- policy structs ---------------------------------------------------------------------------------------------------------------------
// One set of checks for srlhip_rollout_policy, srlhip_rollout_mlp_policy(_sampled) and srlhip_policy_act; every message is a tail, the
// entry point prefixes its name.  The order in which an entry point walks them is api.hip's (the comment above PolicyCall).
// 1. the struct is there and is this ABI's (nothing else of it is read before)
inline Verdict check_policy_abi(const srlhip_linear_policy *p) {
    if (!p) return {SRLHIP_EINVAL, "null policy"};
    if (p->struct_size != (int32_t)sizeof(srlhip_linear_policy)) return {SRLHIP_EINVAL, "srlhip_linear_policy.struct_size mismatch (ABI)"};
    return kAccepted;
}
inline Verdict check_policy_abi(const srlhip_mlp_policy *p) {
    if (!p) return {SRLHIP_EINVAL, "null policy"};
    if (p->struct_size != (int32_t)sizeof(srlhip_mlp_policy)) return {SRLHIP_EINVAL, "srlhip_mlp_policy.struct_size mismatch (ABI)"};
    return kAccepted;
}
// what the two structs have in common, once their ABI check has passed; hidden == 0: the linear policy
struct PolicyView {
    const char *what;              // what the struct calls its parameter block: "weights" / "params"
    const void *w;
    const double *mean, *std;
    double clip;
    int32_t per_env, freeze, normalize, hidden, reserved;
    bool mlp;
};
inline PolicyView policy_view(const srlhip_linear_policy &p) {
    return {"weights", p.weights, p.obs_mean, p.obs_std, p.clip_obs, p.per_env, p.freeze_after_done, p.normalize, 0, 0, false};
}
inline PolicyView policy_view(const srlhip_mlp_policy &p) {
    return {"params", p.params, p.obs_mean, p.obs_std, p.clip_obs, p.per_env, p.freeze_after_done, p.normalize, p.hidden, p.reserved, true};
}
// 2. the MLP's shape fields
inline Verdict check_policy_shape(const PolicyView &v) {
    if (v.mlp && (v.hidden < 1 || v.hidden > 128)) return {SRLHIP_EINVAL, "hidden must be in 1..128"};
    if (v.mlp && v.reserved != 0) return {SRLHIP_EINVAL, "reserved must be 0"};
    return kAccepted;
}
// 3. the pointers
inline Verdict check_policy_pointers(const PolicyView &v) {
    if (!v.w) return {SRLHIP_EINVAL, v.mlp ? "null params" : "null weights"};
    if (v.normalize && (!v.mean || !v.std)) return {SRLHIP_EINVAL, "normalize needs obs_mean and obs_std"};
    return kAccepted;
}
// parameters per policy: float64 [D][A] / float32 P = H D + H + A H + A
inline size_t policy_param_count(const srlhip_config &c, const PolicyView &v) {
    const size_t D = (size_t)obs_dim_of(c), A = policy_outputs(c), H = (size_t)v.hidden;
    return v.mlp ? H * D + H + A * H + A : D * A;
}
// 4. the fused rollouts only: what has no policy kernel is refused by name (the handle stays as it was).  sample: srlhip_rollout_mlp_policy_sampled
inline Verdict check_rollout_policy_config(const srlhip_config &c, bool sample) {
    if (c.rng_mode == SRLHIP_RNG_HOST) return {SRLHIP_ENOTSUP, "RNG_HOST is not supported (needs a device RNG mode)"};
    if (!c.auto_reset) return {SRLHIP_ENOTSUP, "needs auto_reset"};
    if (c.obs_mode == SRLHIP_OBS_RAW_PIXELS) return {SRLHIP_ENOTSUP, "raw_pixels observations are not supported (ground_truth only)"};
    if (c.obs_mode == SRLHIP_OBS_JOINTS) return {SRLHIP_ENOTSUP, "the joints observation mode is not supported (ground_truth only)"};
    if (c.obs_mode == SRLHIP_OBS_JOINTS_POSITION) return {SRLHIP_ENOTSUP, "the joints_position observation mode is not supported (ground_truth only)"};
    if (c.env_kind == SRLHIP_ENV_KUKA_RAND) return {SRLHIP_ENOTSUP, "KukaRandButtonGymEnv is not supported"};
    if (!is_mobile(c.env_kind) && c.kuka_model != SRLHIP_KUKA_MODEL_FULL) return {SRLHIP_ENOTSUP, "the lumped Kuka model is not supported"};
    if (sample && !c.is_discrete) return {SRLHIP_ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"};
    return kAccepted;
}
// 5. the fused rollouts on a host-pointer handle: the values (wcount parameters of 8 or 4 bytes, mean / std [D])
inline Verdict check_policy_values(const PolicyView &v, size_t wcount, size_t D) {
    if (!(v.mlp ? all_finite_f32(static_cast<const float *>(v.w), wcount) : all_finite_f64(static_cast<const double *>(v.w), wcount)))
        return {SRLHIP_EINVAL, v.mlp ? "non-finite params" : "non-finite weights"};
    if (v.normalize) {
        if (!all_finite_f64(v.mean, D)) return {SRLHIP_EINVAL, "non-finite obs_mean"};
        for (size_t d = 0; d < D; d++)
            if (!(finite_f64(v.std[d]) && v.std[d] > 0.0)) return {SRLHIP_EINVAL, "obs_std entries must be finite and > 0"};
    }
    return kAccepted;
}
// srlhip_policy_act's own argument checks, in its order around the shared ones: (a) before the ABI checks, (b) after the shape checks,
// (c) after the pointer checks.  have_*: the pointer is not null
inline Verdict check_policy_act_which(bool have_linear, bool have_mlp) {
    if (have_linear == have_mlp) return {SRLHIP_EINVAL, "pass exactly one of the linear and the MLP policy"};
    return kAccepted;
}
inline Verdict check_policy_act_shape(int32_t obs_dim, bool sample, bool mlp) {
    if (obs_dim < 1 || obs_dim > 1024) return {SRLHIP_EINVAL, "obs_dim must be in 1..1024"};
    if (sample && !mlp) return {SRLHIP_EINVAL, "only an MLP policy's actions are sampled"};
    return kAccepted;
}
inline Verdict check_policy_act_planes(const srlhip_config &c, const PolicyView &v, bool sample, bool have_obs, bool have_act, bool have_frozen) {
    if (!have_obs || !have_act) return {SRLHIP_EINVAL, "null obs or act_out"};
    if (v.freeze && !have_frozen) return {SRLHIP_EINVAL, "freeze_after_done needs the frozen plane"};
    if (!c.io_device) return {SRLHIP_ENOTSUP, "device-pointer handles only (io_device = 1)"};
    if (sample && !c.is_discrete) return {SRLHIP_ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"};
    return kAccepted;
}

// srlhip_rollout_policy_summary's own argument checks (tails; the entry point prefixes "rollout_policy_summary: "), in its order around
// the shared ones: which policy — check_policy_act_which — before the ABI checks, the output struct right behind them; the config
// rules are the plane calls' (check_rollout_policy_config / check_rollout_policy_sampled_config by `sample` and the policy kind)
inline Verdict check_rollout_summary(const srlhip_rollout_summary *out) {
    if (!out) return {SRLHIP_EINVAL, "null out"};
    if (out->struct_size != (int32_t)sizeof(srlhip_rollout_summary)) return {SRLHIP_EINVAL, "srlhip_rollout_summary.struct_size mismatch (ABI)"};
    if (out->reserved != 0) return {SRLHIP_EINVAL, "reserved must be 0"};
    if (!out->ret) return {SRLHIP_EINVAL, "null ret"};
    if ((out->obs_sum != nullptr) != (out->obs_sqsum != nullptr)) return {SRLHIP_EINVAL, "obs_sum and obs_sqsum come together (both or neither)"};
    return kAccepted;
}

// ---- the linear policy's sampled forms ----------------------------------------------------------------------------------------------------
// srlhip_rollout_policy_sampled: what srlhip_rollout_policy refuses, in its order, then the continuous action modes (tails; the entry
// point prefixes "rollout_policy_sampled: ").  The struct and pointer checks in front of it are the shared ones above.
inline Verdict check_rollout_policy_sampled_config(const srlhip_config &c) {
    if (const Verdict v = check_rollout_policy_config(c, false); v.code) return v;
    if (!c.is_discrete) return {SRLHIP_ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"};
    return kAccepted;
}
// srlhip_sample_actions (tails; the entry point prefixes "sample_actions: "): the planes, then what the handle's config rules out — nothing
// of the env kind, the model or the observation mode: the call never looks at the env state
inline Verdict check_sample_actions(const srlhip_config &c, bool have_scores, bool have_act) {
    if (!have_scores || !have_act) return {SRLHIP_EINVAL, "null scores or act_out"};
    if (!c.io_device) return {SRLHIP_ENOTSUP, "device-pointer handles only (io_device = 1)"};
    if (!c.is_discrete) return {SRLHIP_ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"};
    return kAccepted;
}

// ---- srlhip_cnn_policy_act: the CNN's shapes and argument checks --------------------------------------------------------------------------
// The reference's CNNPolicyPytorch (cma_es.py:259-300) on an [H][W][C] frame: conv 5x5 s2 p2 C->8, conv 3x3 s2 p1 8->16, conv 3x3 s2 p1
// 16->32, each behind it batch-norm, ReLU and a 2x2 max-pool (floor), then a linear layer F -> A.  conv: (x + 2 pad - k) / 2 + 1.
constexpr int kCnnMinSide = 43, kCnnMaxSide = 224;      // 43: the smallest side whose third conv plane is 2x2 (pool output non-empty)
constexpr int kCnnCh1 = 8, kCnnCh2 = 16, kCnnCh3 = 32;
struct CnnShape {
    int C, H, W;
    int hc[3], wc[3];              // the conv planes
    int hp[3], wp[3];              // the pooled planes
    int F;                         // 32 hp[2] wp[2]: the linear layer's inputs, channel-major
};
inline CnnShape cnn_shape(int C, int H, int W) {
    CnnShape s{};
    s.C = C; s.H = H; s.W = W;
    s.hc[0] = (H + 4 - 5) / 2 + 1; s.wc[0] = (W + 4 - 5) / 2 + 1;
    for (int l = 0; l < 3; l++) {
        if (l) { s.hc[l] = (s.hp[l - 1] + 2 - 3) / 2 + 1; s.wc[l] = (s.wp[l - 1] + 2 - 3) / 2 + 1; }
        s.hp[l] = s.hc[l] / 2; s.wp[l] = s.wc[l] / 2;
    }
    s.F = kCnnCh3 * s.hp[2] * s.wp[2];
    return s;
}
// the offsets of the eleven blocks of one parameter vector, nn.Module.parameters() order, and their total P
struct CnnParamLayout { size_t w1, g1, b1, w2, g2, b2, w3, g3, b3, fcw, fcb, total; };
inline CnnParamLayout cnn_param_layout(int C, int H, int W, int A) {
    CnnParamLayout L;
    size_t o = 0;
    L.w1 = o; o += (size_t)kCnnCh1 * C * 25; L.g1 = o; o += kCnnCh1; L.b1 = o; o += kCnnCh1;
    L.w2 = o; o += (size_t)kCnnCh2 * kCnnCh1 * 9; L.g2 = o; o += kCnnCh2; L.b2 = o; o += kCnnCh2;
    L.w3 = o; o += (size_t)kCnnCh3 * kCnnCh2 * 9; L.g3 = o; o += kCnnCh3; L.b3 = o; o += kCnnCh3;
    L.fcw = o; o += (size_t)A * cnn_shape(C, H, W).F; L.fcb = o; o += (size_t)A;
    L.total = o;
    return L;
}
inline size_t cnn_param_count(int C, int H, int W, int A) { return cnn_param_layout(C, H, W, A).total; }
inline bool cnn_side_ok(int side) { return side >= kCnnMinSide && side <= kCnnMaxSide; }
// srlhip_cnn_policy_act's checks in their order (tails; the entry point prefixes "cnn_policy_act: "): the struct, then the planes and
// what the handle's config rules out
inline Verdict check_cnn_policy_abi(const srlhip_cnn_policy *p) {
    if (!p) return {SRLHIP_EINVAL, "null policy"};
    if (p->struct_size != (int32_t)sizeof(srlhip_cnn_policy)) return {SRLHIP_EINVAL, "srlhip_cnn_policy.struct_size mismatch (ABI)"};
    if (p->reserved != 0) return {SRLHIP_EINVAL, "reserved must be 0"};
    if (!p->params) return {SRLHIP_EINVAL, "null params"};
    return kAccepted;
}
inline Verdict check_cnn_policy_act(const srlhip_config &c, bool freeze, bool sample, bool have_images, bool have_act, bool have_frozen) {
    if (!have_images || !have_act) return {SRLHIP_EINVAL, "null images or act_out"};
    if (freeze && !have_frozen) return {SRLHIP_EINVAL, "freeze_after_done needs the frozen plane"};
    if (!c.io_device) return {SRLHIP_ENOTSUP, "device-pointer handles only (io_device = 1)"};
    if (c.obs_mode != SRLHIP_OBS_RAW_PIXELS) return {SRLHIP_ENOTSUP, "raw_pixels observations only (the policy reads the handle's frames)"};
    if (!cnn_side_ok(c.img_h) || !cnn_side_ok(c.img_w)) return {SRLHIP_ENOTSUP, "img_h and img_w must be in 43..224 (below 43 the third pooled plane is empty)"};
    if (sample && !c.is_discrete) return {SRLHIP_ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"};
    return kAccepted;
}

// ---- srlhip_pixel_policy_act: ARS's linear policy on the frame -----------------------------------------------------------------------------
// Work items (pairs, or envs when unpaired) below kPixSplitItems give every chunk of rows a workgroup of its own (pixel_policy.hip); the
// handle then holds the chunk sums of at most kPixSplitWgs workgroups, kPixSplitSlot doubles each, and one ticket word per item
constexpr int kPixSplitItems = 256, kPixSplitWgs = 2048, kPixSplitSlot = 16;
inline bool pix_split(int items, int chunks) { return chunks > 1 && items < kPixSplitItems && (int64_t)items * chunks <= kPixSplitWgs; }
// the checks in their order (tails; the entry point prefixes "pixel_policy_act: "): the struct, then the planes and what the handle's
// config rules out
inline Verdict check_pixel_policy_abi(const srlhip_pixel_policy *p) {
    if (!p) return {SRLHIP_EINVAL, "null policy"};
    if (p->struct_size != (int32_t)sizeof(srlhip_pixel_policy)) return {SRLHIP_EINVAL, "srlhip_pixel_policy.struct_size mismatch (ABI)"};
    if (p->reserved != 0) return {SRLHIP_EINVAL, "reserved must be 0"};
    if (!p->weights) return {SRLHIP_EINVAL, "null weights"};
    if (p->paired && !p->delta) return {SRLHIP_EINVAL, "paired needs delta"};
    if (!p->paired && p->delta) return {SRLHIP_EINVAL, "delta must be null unless paired"};
    return kAccepted;
}
inline Verdict check_pixel_policy_act(const srlhip_config &c, bool paired, bool freeze, bool have_images, bool have_act, bool have_frozen) {
    if (!have_images || !have_act) return {SRLHIP_EINVAL, "null images or act_out"};
    if (paired && c.num_envs % 2 != 0) return {SRLHIP_EINVAL, "paired needs an even num_envs (env 2k and 2k + 1 share delta[k])"};
    if (freeze && !have_frozen) return {SRLHIP_EINVAL, "freeze_after_done needs the frozen plane"};
    if (!c.io_device) return {SRLHIP_ENOTSUP, "device-pointer handles only (io_device = 1)"};
    if (c.obs_mode != SRLHIP_OBS_RAW_PIXELS) return {SRLHIP_ENOTSUP, "raw_pixels observations only (the policy reads the handle's frames)"};
    return kAccepted;
}

// ---- srlhip_render_jpeg's scratch buffer ------------------------------------------------------------------------------------------------
// the frames; on a host-pointer handle also offsets i64 [ns + 1], overflow i32 [ns] and the blob's ns slots of `cap` bytes
struct JpegScratch {
    int ch;                        // channels per env: 3, or 6 = two streams
    size_t ns;                     // streams
    int64_t cap;                   // bytes per stream of the caller's blob
    size_t frames, off_at, ovf_at, blob_at;
    size_t bytes(bool io_device) const { return io_device ? frames : blob_at + (size_t)cap * ns; }
};
inline JpegScratch jpeg_scratch(const srlhip_config &c, size_t n, int64_t blob_cap) {
    JpegScratch s;
    s.ch = c.multi_view ? 6 : 3;
    s.ns = n * (size_t)(s.ch / 3);
    s.cap = blob_cap / (int64_t)s.ns;
    s.frames = pad16(frame_bytes(c) * n);
    s.off_at = s.frames; s.ovf_at = s.off_at + 8 * (s.ns + 1); s.blob_at = pad16(s.ovf_at + 4 * s.ns);
    return s;
}

// ---- the episode-record block of a host-pointer handle ----------------------------------------------------------------------------------
// Monitor's (r, l) of the last finished episode in ONE mapped block: last_return f64 [n], then last_length i32 [n]
inline size_t episode_block_bytes(size_t n) { return 12 * n; }
inline double *episode_returns(void *block) { return static_cast<double *>(block); }
inline int32_t *episode_lengths(void *block, size_t n) { return reinterpret_cast<int32_t *>(static_cast<uint8_t *>(block) + 8 * n); }

}  // namespace srl
