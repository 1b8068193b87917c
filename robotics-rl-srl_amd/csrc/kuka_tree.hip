// kuka_tree.hip — lane-group kernels of the FULL Kuka model (kuka_tree.hpp: 12-DoF arm + gripper tree, per-link contact spheres,
// friction rows): rollout / step, reset, settle + start-state table, refresh after srlhip_set_state.  Launch geometry of the
// lane-group family: 16 lanes = one DPP row per env, one wavefront (4 envs) per workgroup — a 4096-env batch is 1024 wavefronts,
// one per SIMD of the MI355X.  The model is a table in HBM read once per launch into per-lane registers (srlhip_kuka_tree_model).
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

namespace {
__global__ void __launch_bounds__(kGroupBlock) kuka_tree_table_k(const TreeModel *m, double *ttable) {
    TLane L;
    tree::lane_init(L, m);
    if (threadIdx.x < grp::GL) tree::lane_store(L, ttable);
}

// 500 settle steps (kuka_button_gym_env.py:242-247): every group of the wavefront integrates the same env, group 0 publishes
__global__ void __launch_bounds__(kGroupBlock) kuka_tree_settle_k(KukaParams p, KukaState s) {
    using namespace grp;
    __shared__ double scratch_all[kGroupEnvs][kTS];
    __shared__ double tab[tree::kLaneTableDoubles];
    LaneId L; build_lane_table(L, s.ttable, tab);
    Env e = {};
    GState g;
    tree::tinitial(e, g, tab);
    const double zero[3] = {0, 0, 0};
    for (int i = 0; i < kNSettleSteps; i++) tree::tphysics_step(e, g, tab, p.cfg, scratch_all[threadIdx.x / GL], zero, p.cfg.action_joints != 0, L.q0, 0.0);
    if (threadIdx.x < GL) tree::tpack_start(e, g, s.tsettled);
}
// table of the 6^5 (2^5) possible episode start states: one lane group per state
__global__ void __launch_bounds__(kGroupBlock) kuka_tree_starts_k(KukaParams p, KukaState s) {
    using namespace grp;
    __shared__ double scratch_all[kGroupEnvs][kTS];
    const int idx_raw = blockIdx.x * kGroupEnvs + (int)(threadIdx.x / GL);
    const bool valid = idx_raw < s.nstarts;
    const int idx = valid ? idx_raw : s.nstarts - 1;
    __shared__ double tab[tree::kLaneTableDoubles];
    LaneId L; build_lane_table(L, s.ttable, tab);
    Env e = {};
    GState g;
    tree::tunpack_start(e, g, s.tsettled);
    e.bx = kButtonX; e.by = kButtonY; e.bz = L.base_z;
    tree::tfk(tree::lane_view(tab), g);
    const int base = p.cfg.is_discrete ? 6 : 2;
    int rem = idx;
    double motor[3];
    for (int k = 0; k < kNInitActions; k++) {
        init_action_motor(p.cfg, rem % base, motor);
        tree::tphysics_step(e, g, tab, p.cfg, scratch_all[threadIdx.x / GL], motor, false, L.q0, 0.0);
        rem /= base;
    }
    if (valid) tree::tpack_start(e, g, s.tstarts + (int64_t)idx * kTStart);
}
// after srlhip_set_state(KUKA_Q / GRIPPER_Q): refresh the cached sin / cos and the gripper position
__global__ void __launch_bounds__(kGroupBlock) kuka_tree_refresh_k(KukaParams p, KukaState s) {
    using namespace grp;
    const int64_t n = p.n;
    const int e_raw = blockIdx.x * kGroupEnvs + (int)(threadIdx.x / GL);
    const bool valid = e_raw < p.n;
    const int e = valid ? e_raw : p.n - 1;
    __shared__ double tab[tree::kLaneTableDoubles];
    LaneId L; build_lane_table(L, s.ttable, tab);
    Env v = {};
    GState g;
    tload(s, n, e, L, v, g, p.cfg.two != 0);
    tree::trefresh(tree::lane_view(tab), g, v);
    tstore(s, n, e, L, v, g, valid, p.cfg.two != 0);
}

}  // namespace

// (the host copy of the installed table is part of every Handle; the value means something on full-model handles only, and only they come here)
static double solver_detail_of(const Handle *h) { return reinterpret_cast<const TreeModel *>(h->kuka_tmodel_host)->solver_detail; }

// Which kernel: kuka_tree_select.hpp (tree_select_launch).  Two overrides, read here: SRLHIP_KUKA_SPEC=0 keeps the generic instantiation
// where the configuration-specialised one applies (tests compare the two), once per process; SRLHIP_KUKA_OCC=0|1 forces the one- or the
// two-wavefront variant (tests run both on small batches), at every call.
// (Why the two-wavefront variant is the default only from 65536 envs up: kuka_tree_occ.hip.  Round 5: where the specialised
//  one-wavefront instantiation applies it is the faster one at every size measured — 65536 envs 1.73e8 against 1.66e8, 131072 1.74e8
//  against 1.72e8 env-steps/s, profiles/r05_nsweep_kuka.jsonl — so the default takes the variant only where that one does not apply.)
int kuka_tree_launch(Handle *h, const KukaParams &p, int T, const void *d_actions, const double *d_noise, float *obs, float *d_rew,
                     uint8_t *d_done, void *d_act_out) {
    static const bool spec_allowed = [] { const char *v = getenv("SRLHIP_KUKA_SPEC"); return !v || atoi(v) != 0; }();
    const char *force = getenv("SRLHIP_KUKA_OCC");
    const TreeSelect s = tree_select_launch(h->cfg, h->n, d_actions != nullptr, T, obs != nullptr, solver_detail_of(h), h->step_signal.done != nullptr,
                                            force ? (force[0] == '1' ? 1 : 0) : -1, spec_allowed);
    if (s.family == TREE_RB) return kuka_tree_rb_launch(h, p, s, T, d_actions, d_noise, obs, d_rew, d_done, d_act_out);      // free bodies: kuka_tree_rb.hip
    if (s.family == TREE_OCC) return kuka_tree_occ_launch(h, p, s, T, d_actions, d_noise, obs, d_rew, d_done, d_act_out);
    const TreeIo io = {T, d_actions, d_noise, obs, d_rew, d_done, d_act_out};
    int rc = 0;
    bool hit;
    if (s.family == TREE_SPEC)      // (MT19937: the reference's own streams, HipVecEnv's default)
        hit = dispatch_rollout_device_rng(s.mode, [&](auto mode) {
            return dispatch_int<0, 1>(s.given, [&](auto given) { rc = tree_rollout_launch<0, 1>(h, p, mode, Const<0>{}, given, Const<1>{}, s.arm_signal, io); });
        });
    else
        hit = dispatch_rollout_rng(s.mode, [&](auto mode) {
            return dispatch_tree_arm(s.joints, s.nb, [&](auto joints, auto nb) {
                return dispatch_int<0, 1>(s.given, [&](auto given) { rc = tree_rollout_launch(h, p, mode, joints, given, nb, s.arm_signal, io); });
            });
        });
    return hit ? rc : h->fail(SRLHIP_ENOTSUP, "rollout: no instantiation for this Kuka configuration");
}

// ---- persistent stepping (step_signal.hpp; srlhip_set_persistent) -------------------------------------------------------------------
// Which resident kernel, if any: kuka_tree_select.hpp (tree_select_persist).  The grid must be CO-RESIDENT: a workgroup that waits for
// the host in a loop never makes room for one that has not started.  So the kernel whose occupancy decides whether the grid fits and the
// kernel that is launched must be the same one: both come out of this one dispatch on the selected tuple: specialised, generic Cartesian,
// generic joint-space actions, Kuka2Button — f(mode, joints, nb, spec).
template <class F>
static bool dispatch_persist(const Handle *h, F &&f) {
    if (!h->kuka) return false;
    const TreeSelect s = tree_select_persist(h->cfg, solver_detail_of(h));
    if (s.family == TREE_NONE) return false;
    const auto go = [&](auto joints, auto nb, auto spec) { return dispatch_rollout_device_rng(s.mode, [&](auto mode) { f(mode, joints, nb, spec); }); };
    if (s.family == TREE_SPEC) return go(Const<0>{}, Const<1>{}, Const<1>{});
    if (s.nb == 1 && !s.joints) return go(Const<0>{}, Const<1>{}, Const<0>{});
    if (s.nb == 1 && s.joints) return go(Const<1>{}, Const<1>{}, Const<0>{});
    if (s.nb == 2 && !s.joints) return go(Const<0>{}, Const<2>{}, Const<0>{});
    return false;
}
int kuka_tree_persist_blocks(Handle *h, int *capacity) {
    if (capacity) *capacity = 0;
    const void *fn = nullptr;
    dispatch_persist(h, [&](auto mode, auto joints, auto nb, auto spec) {
        fn = reinterpret_cast<const void *>(kuka_tree_rollout_k<decltype(mode)::value, decltype(joints)::value != 0, true, decltype(nb)::value, 0, decltype(spec)::value, 1>);
    });
    if (!fn) return 0;
    const int real = (h->n + kGroupEnvs - 1) / kGroupEnvs, grid = contiguous_grid(real);
    int per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->cfg.device_id) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kGroupBlock, 0) != hipSuccess) return 0;
    if (capacity) *capacity = per_cu * prop.multiProcessorCount;       // workgroups of this kernel the device holds at once
    return (long long)per_cu * prop.multiProcessorCount >= grid ? real : 0;
}
int kuka_tree_persist_launch(Handle *h, const KukaParams &p, const void *d_actions, float *obs, float *d_rew, uint8_t *d_done, const PersistArgs &pa) {
    const TreeIo io = {0, d_actions, nullptr, obs, d_rew, d_done, nullptr};
    int rc = 0;
    const bool hit = dispatch_persist(h, [&](auto mode, auto joints, auto nb, auto spec) {
        rc = tree_rollout_launch<0, decltype(spec)::value, 1>(h, p, mode, joints, Const<1>{}, nb, false, io, pa);
    });
    return hit ? rc : h->fail(SRLHIP_ENOTSUP, "persistent stepping: no instantiation for this configuration");
}

int kuka_tree_reset(Handle *h, const KukaParams &p, const uint8_t *d_mask, const double *d_host_rand, int stride, float *obs) {
    if (h->cfg.env_kind == SRLHIP_ENV_KUKA_RAND) return kuka_tree_rb_reset(h, p, d_mask, d_host_rand, stride, obs);
    const bool two = h->cfg.env_kind == SRLHIP_ENV_KUKA_2BUTTON;
    int rc = 0;
    const bool hit = dispatch_reset_rng(h->cfg.rng_mode, [&](auto mode) {
        return dispatch_tree_arm(!two && tree_joint_actions(h->cfg), two ? 2 : 1, [&](auto joints, auto nb) {
            rc = tree_reset_launch<0>(h, p, mode, joints, nb, d_mask, d_host_rand, stride, obs);
        });
    });
    return hit ? rc : h->fail(SRLHIP_ENOTSUP, "reset: no instantiation for this Kuka configuration");
}

int kuka_tree_settle(Handle *h, const KukaParams &p) {
    hipLaunchKernelGGL(kuka_tree_table_k, dim3(1), dim3(kGroupBlock), 0, h->stream, h->kuka->tmodel, h->kuka->ttable);
    SRL_HIP_CHECK(h, hipGetLastError());
    hipLaunchKernelGGL(kuka_tree_settle_k, dim3(1), dim3(kGroupBlock), 0, h->stream, p, *h->kuka);
    SRL_HIP_CHECK(h, hipGetLastError());
    if (h->kuka->nstarts > 0) {
        hipLaunchKernelGGL(kuka_tree_starts_k, dim3((h->kuka->nstarts + kGroupEnvs - 1) / kGroupEnvs), dim3(kGroupBlock), 0, h->stream, p, *h->kuka);
        SRL_HIP_CHECK(h, hipGetLastError());
    }
    return 0;
}

int kuka_tree_refresh(Handle *h, const KukaParams &p) {
    hipLaunchKernelGGL(kuka_tree_refresh_k, dim3((h->n + kGroupEnvs - 1) / kGroupEnvs), dim3(kGroupBlock), 0, h->stream, p, *h->kuka);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

}  // namespace srl
