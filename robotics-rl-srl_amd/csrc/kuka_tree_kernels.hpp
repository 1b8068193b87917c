// kuka_tree_kernels.hpp — the rollout / reset kernel templates of the full-model lane-group stepper, shared by the translation units that
// instantiate them: kuka_tree.hip (every Kuka env) and kuka_tree_rb.hip (KukaRandButtonGymEnv: RB = 1, the free bodies of
// kuka_tree.hpp's free-body section ride on lanes 0..10).  Launch geometry of the lane-group family: 16 lanes = one DPP row per env,
// one wavefront (4 envs) per workgroup — a 4096-env batch is 1024 wavefronts, one per SIMD of the MI355X.
#pragma once
#include "kuka_device.hpp"
#include "kuka_tree.hpp"
#include "kuka_tree_select.hpp"

namespace srl {
using namespace kuka;

namespace {
using tree::TLane;
using tree::NJ;
constexpr int kTS = tree::kTreeScratchDoubles, kTStart = tree::kTreeStartDoubles;

// the wavefront's lane-constant table in LDS (kuka_tree.hpp: lane_store / lane_view).  It is derived from the model table ONCE per
// model (kuka_tree_table_k -> KukaState::ttable in HBM: the ancestor / descendant walks cost ~0.1 ms, far too much for the
// single-step launches of the per-step API); a launch only copies its 5.6 KB.
struct LaneId { int l; bool jnt; double q0, base_z; };
__device__ __forceinline__ void build_lane_table(LaneId &L, const double *ttable, double *tab) {
    // every load of the copy in flight before the first wait (a rolled copy loop waits out one global-memory round trip per 512
    // bytes: eleven of them, ~7 us of a 38-us single-step launch)
    constexpr int kCopyIters = (tree::kLaneTableDoubles + kGroupBlock - 1) / kGroupBlock;
    double row[kCopyIters];
#pragma unroll
    for (int k = 0; k < kCopyIters; k++) { const int i = (int)threadIdx.x + k * kGroupBlock; row[k] = i < tree::kLaneTableDoubles ? ttable[i] : 0.0; }
#pragma unroll
    for (int k = 0; k < kCopyIters; k++) { const int i = (int)threadIdx.x + k * kGroupBlock; if (i < tree::kLaneTableDoubles) tab[i] = row[k]; }
    __syncthreads();
    L.l = (int)(threadIdx.x & (grp::GL - 1)); L.jnt = L.l < NJ;
    L.q0 = tab[tree::LT_Q0 * grp::GL + L.l]; L.base_z = tab[tree::LT_COUNT * grp::GL + tree::LS_BASEZ];
}
// env scalars replicated on the row, the own joint per joint lane
__device__ __forceinline__ void tload(const KukaState &s, int64_t n, int e, const LaneId &L, Env &v, grp::GState &g, bool two) {
#pragma unroll
    for (int k = 0; k < 3; k++) { v.ee[k] = s.d[(D_EE + k) * n + e]; v.bpos[k] = s.d[(D_BPOS + k) * n + e]; v.grip[k] = s.d[(D_GRIP + k) * n + e]; }
    v.bq = s.d[D_BQ * n + e]; v.bqd = s.d[D_BQD * n + e]; v.bx = s.d[D_BX * n + e]; v.by = s.d[D_BY * n + e];
    v.bz = s.d[D_BZ * n + e]; v.bspeed = s.d[D_BSPEED * n + e];
    v.motor_on = s.i[I_MOTOR * n + e]; v.contact_button = s.i[I_CB * n + e]; v.contact_table = s.i[I_CT * n + e];
    v.counter = s.i[I_COUNTER * n + e]; v.n_contacts = s.i[I_NCONTACT * n + e]; v.n_outside = s.i[I_NOUT * n + e];
    v.terminated = s.i[I_TERM * n + e]; v.ikx = s.i[I_IKX * n + e];
    if (two) {                               // Kuka2ButtonGymEnv: second glider, goal switching
        v.b2q = s.d[D_B2Q * n + e]; v.b2qd = s.d[D_B2QD * n + e]; v.b2x = s.d[D_B2X * n + e]; v.b2y = s.d[D_B2Y * n + e];
        v.goal_id = s.i[I_GOAL * n + e]; v.n_contacts2 = s.i[I_NCONTACT2 * n + e]; v.contact_body1 = 0; v.contact_body2 = 0;
    }
    const int j = L.jnt ? L.l : 0;
    g.q = s.d[tree_plane(D_Q, D_GQ, j) * n + e]; g.qd = s.d[tree_plane(D_QD, D_GQD, j) * n + e];
    g.sq = s.d[tree_plane(D_SQ, D_GSQ, j) * n + e]; g.cq = s.d[tree_plane(D_CQ, D_GCQ, j) * n + e];
    if (!L.jnt) { g.q = 0.0; g.qd = 0.0; g.sq = 0.0; g.cq = 1.0; }
}
__device__ __forceinline__ void tstore(const KukaState &s, int64_t n, int e, const LaneId &L, const Env &v, const grp::GState &g, bool valid, bool two) {
    if (valid && L.jnt) {
        s.d[tree_plane(D_Q, D_GQ, L.l) * n + e] = g.q; s.d[tree_plane(D_QD, D_GQD, L.l) * n + e] = g.qd;
        s.d[tree_plane(D_SQ, D_GSQ, L.l) * n + e] = g.sq; s.d[tree_plane(D_CQ, D_GCQ, L.l) * n + e] = g.cq;
    }
    if (valid && L.l == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { s.d[(D_EE + k) * n + e] = v.ee[k]; s.d[(D_BPOS + k) * n + e] = v.bpos[k]; s.d[(D_GRIP + k) * n + e] = v.grip[k]; }
        s.d[D_BQ * n + e] = v.bq; s.d[D_BQD * n + e] = v.bqd; s.d[D_BX * n + e] = v.bx; s.d[D_BY * n + e] = v.by;
        s.d[D_BZ * n + e] = v.bz; s.d[D_BSPEED * n + e] = v.bspeed;
        s.i[I_MOTOR * n + e] = v.motor_on; s.i[I_CB * n + e] = v.contact_button; s.i[I_CT * n + e] = v.contact_table;
        s.i[I_COUNTER * n + e] = v.counter; s.i[I_NCONTACT * n + e] = v.n_contacts; s.i[I_NOUT * n + e] = v.n_outside;
        s.i[I_TERM * n + e] = v.terminated; s.i[I_IKX * n + e] = v.ikx;
        if (two) {
            s.d[D_B2Q * n + e] = v.b2q; s.d[D_B2QD * n + e] = v.b2qd; s.d[D_B2X * n + e] = v.b2x; s.d[D_B2Y * n + e] = v.b2y;
            s.i[I_GOAL * n + e] = v.goal_id; s.i[I_NCONTACT2 * n + e] = v.n_contacts2;
        }
    }
}

// KukaRandButton free bodies: lane k < 11 owns body k.  Dynamic state in the rb planes [(6 k + c)][n] (x y z vx vy vz); the reset draws
// (x, y, kept) of the ten distractors in the objs planes (srlhip_get_state KUKA_OBJECTS), from which the type hash and the kick
// direction derive.
__device__ __forceinline__ void tload_body(const KukaState &s, int64_t n, int e, int l, tree::RBody &B) {
    const int k = l < tree::kRbN ? l : 0;
#pragma unroll
    for (int c = 0; c < 3; c++) { B.x[c] = s.rb[(6 * k + c) * n + e]; B.v[c] = s.rb[(6 * k + 3 + c) * n + e]; }
    const int ko = l < 10 ? l : 0;
    B.ox = s.objs[(3 * ko) * n + e]; B.oy = s.objs[(3 * ko + 1) * n + e];
    B.on = l < 10 ? s.objs[(3 * ko + 2) * n + e] != 0.0 : l == 10;
    B.type = l < 10 ? tree::rb_type_of(B.ox, B.oy) : l == 10 ? 3 : 2;
    if (l >= 10) { B.ox = 0.0; B.oy = 0.0; }
}
__device__ __forceinline__ void tstore_body(const KukaState &s, int64_t n, int e, int l, const tree::RBody &B, bool valid) {
    if (valid && l < tree::kRbN) {
#pragma unroll
        for (int c = 0; c < 3; c++) { s.rb[(6 * l + c) * n + e] = B.x[c]; s.rb[(6 * l + 3 + c) * n + e] = B.v[c]; }
    }
}

// T consecutive VecEnv steps per launch.  GIVEN: the caller supplies the actions (a compile-time switch: a possible action load
// inside the step loop makes every step wait for the previous step's output stores — gfx9 counts loads and stores together).
// SPEC = 1: the reference's DEFAULT KukaButtonGymEnv configuration (discrete actions, static button, ground-truth observation, force_down,
// action_repeat 1, sparse reward, auto-reset: kuka_button_gym_env.py:93-98 ctor defaults) AND the model table's default solver details
// (solver_detail = 0) as compile-time constants — the run-time
// configuration tests of the env logic and of the step's branches fold away (the host selects it only for a handle with exactly
// this configuration, kuka_tree_select.hpp: tree_spec_config).
// PERSIST = 1 (srlhip_set_persistent; GIVEN actions; the protocol is step_signal.hpp's): the loop does not count to T — before every step
// the wavefront waits for the host's next sequence number, reads its actions from the SAME mapped row every step, writes its outputs
// straight to the host's mapped planes (on a placement where that is not valid: to a staging copy that the last wavefront of its eighth
// of the grid copies out), publishes Monitor's record of an episode that ended right away; it leaves the loop (and writes the state back
// like any rollout) when workgroup 0 relays the park token.  While it waits it already runs the action-independent half of the next
// step (tree::tphysics_pre).
// (timeline build of persistent stepping, profiles/probes/persist_timeline.py: -DSRL_PERSIST_PROF; 100 MHz device-wide clock, the stamps of
//  a workgroup's LAST step, 8 per workgroup, behind the relay / counter words)
#if defined(SRL_PERSIST_PROF) && defined(__HIP_DEVICE_COMPILE__)
#define SRL_PSTAMP(k) do { if (threadIdx.x == 0) reinterpret_cast<uint64_t *>(pa.relay + kWordStamps)[bid * kStampsPerBlock + (k)] = wall_clock64(); } while (0)
#else
#define SRL_PSTAMP(k) do { } while (0)
#endif

// persistent stepping: one wavefront copies an env range of the three output planes staging -> mapped host planes.  The staging copy was
// written through by wavefronts of every XCD: agent-scope loads (sc1), ALL of them in flight before the first store — 16 bytes per lane
// where the range is 16-byte aligned (always for obs / reward: ranges start at a multiple of 4 envs), dwords for the rest.
struct PersistSeg { const uint32_t *src; uint32_t *dst; int count; };      // (dwords)
__device__ __forceinline__ void persist_copy(const PersistSeg (&seg)[3]) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int kQ = 9;                                                    // 16-byte pieces in flight per lane: 9 KB per pass
    int n4[3];                                                               // 16-byte pieces of each segment (0: not aligned)
#pragma unroll
    for (int k = 0; k < 3; k++)
        n4[k] = ((reinterpret_cast<uintptr_t>(seg[k].src) | reinterpret_cast<uintptr_t>(seg[k].dst)) & 15) == 0 ? seg[k].count / 4 : 0;
    const int pieces = n4[0] + n4[1] + n4[2];
    for (int base = 0; base < pieces; base += kQ * kGroupBlock) {
        u32x4 w[kQ];
        const uint32_t *sp[kQ];
        int64_t off[kQ];
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            int g = base + q * kGroupBlock + (int)threadIdx.x;
            const bool on = g < pieces;
            g = on ? g : 0;
            const int k = g < n4[0] ? 0 : g < n4[0] + n4[1] ? 1 : 2;
            const int idx = g - (k == 0 ? 0 : k == 1 ? n4[0] : n4[0] + n4[1]);
            sp[q] = seg[k].src + (int64_t)idx * 4;
            off[q] = on ? (seg[k].dst + (int64_t)idx * 4) - seg[k].src - (int64_t)idx * 4 : 0;   // dst - src of the piece's segment; 0 = skip
            // (unconditional — a lane past the end re-reads piece 0 — so that no select sits between the load and the wait below)
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(w[q]) : "v"(sp[q]) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < kQ; q++)
            if (off[q]) *reinterpret_cast<u32x4 *>(const_cast<uint32_t *>(sp[q]) + off[q]) = w[q];
    }
    // what is left: unaligned segments whole, the last count % 4 dwords of aligned ones
#pragma unroll
    for (int k = 0; k < 3; k++)
        for (int i = n4[k] * 4 + (int)threadIdx.x; i < seg[k].count; i += kGroupBlock)
            seg[k].dst[i] = __hip_atomic_load(seg[k].src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// sum of x over the env's 16-lane row, lane 0 first: the same bits in every lane
__device__ __forceinline__ double mlp_row_sum(double x) {
    using namespace grp;
    double acc = bcast<0>(x);
    fmac_bcast<1>(acc, x, 1.0); fmac_bcast<2>(acc, x, 1.0); fmac_bcast<3>(acc, x, 1.0); fmac_bcast<4>(acc, x, 1.0); fmac_bcast<5>(acc, x, 1.0);
    fmac_bcast<6>(acc, x, 1.0); fmac_bcast<7>(acc, x, 1.0); fmac_bcast<8>(acc, x, 1.0); fmac_bcast<9>(acc, x, 1.0); fmac_bcast<10>(acc, x, 1.0);
    fmac_bcast<11>(acc, x, 1.0); fmac_bcast<12>(acc, x, 1.0); fmac_bcast<13>(acc, x, 1.0); fmac_bcast<14>(acc, x, 1.0); fmac_bcast<15>(acc, x, 1.0);
    return acc;
}

// The sampled policies' selection (contract: include/srlhip.h, srlhip_rollout_mlp_policy_sampled): the action drawn from the softmax of
// the six scores, which every lane of the env's row holds bit for bit.  Lane k < 6 owns exp(sc[k] - m), the six weights come back over
// the row, every lane adds them up in index order and counts the partial sums z = u c_5 has reached — the result is the same in all 16
// lanes, as the step needs it.  u is the block at counter c0 + t of the env's action stream, formed by every lane (80 integer
// instructions next to a 50 k-cycle step) from the key and the counter the prologue loaded: those four words are all the sampling
// keeps live across the step.  A frozen env draws too.
template <class S>
__device__ __forceinline__ int row_softmax_draw(const S &sc, int l, const Philox &act, int t) {
    using namespace grp;
    double m = sc[0], own = sc[0];
#pragma unroll
    for (int k = 1; k < 6; k++) { m = sc[k] > m ? sc[k] : m; own = l == k ? sc[k] : own; }
    const double wl = exp(own - m);
    double c[6];
    c[0] = bcast<0>(wl);
    c[1] = c[0] + bcast<1>(wl); c[2] = c[1] + bcast<2>(wl); c[3] = c[2] + bcast<3>(wl); c[4] = c[3] + bcast<4>(wl); c[5] = c[4] + bcast<5>(wl);
    Philox q = act;
    q.ctr = act.ctr + (uint64_t)t;
    const double z = q.double01() * c[5];
    int a = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) a += z >= c[k] ? 1 : 0;
    return a;
}

// POLICY = 1 (srlhip_rollout_policy; kuka_tree_policy.hip): the third action source — a linear policy of the env's own current
// ground-truth observation.  `actions` is then the float64 weight plane ([n][3][A] or [3][A]) and `noise` the 10-double header
// kuka_policy_hdr_k wrote (per_env, freeze, normalize, clip, mean[3], std[3]).  Lane a < A of the env's row keeps column a of the
// env's weights in VGPRs (LDS is full: 40 712 B per wavefront = four wavefronts per CU), mean / std sit in every lane; all of it is
// loaded before the prologue's vmcnt wait, nothing inside the loop.  At the loop top every lane forms the observation from the row's
// replicated env scalars and its own score; the row's scores are broadcast (DPP row_newbcast) and every lane takes the same strict
// argmax (lowest lane wins a tie), or lane j's score becomes ca[j].
// POLICY = 2 (srlhip_rollout_mlp_policy; kuka_tree_mlp.hip): a one-hidden-layer ReLU MLP of the same observation.  `actions` is the
// float32 parameter plane ([n][P] or [P], P = 3 H + H + A H + A in nn.Module.parameters() order) and `noise` the 11-double header
// kuka_policy_hdr_k wrote (the ten above, then H).  Lane l of the env's row owns the hidden units l, l + 16, ... (at most 8: H <= 128)
// and holds their fc_in rows, biases and fc_out columns as float32 locals (units >= H: zeros), lane 0 also fc_out's bias; the
// parameter plane is read once, before the prologue's vmcnt wait, never inside the loop.  The locals do NOT all stay in registers:
// 86 - 95 floats next to a kernel already at 403 - 503 of 512 registers put every instantiation at the budget, and the compiler
// spills 166 - 259 VGPRs to 408 - 720 B of private scratch per lane and reloads them inside the step loop (figures and the measured
// cost: profiles/NOTES.md AE).  At the loop top every lane computes its hidden units and its A
// partial scores in float64 (unit order l, l + 16, ...), the partials are summed over the row lane 0 .. 15 in order (fmac_bcast with
// weight 1: the same bits in every lane, the same order in every call), then the argmax / continuous row of POLICY = 1.
// POLICY = 3 (srlhip_rollout_mlp_policy_sampled; kuka_tree_mlp_sample.hip): POLICY = 2 up to the six scores, discrete actions only
// (JOINTS = false); the action is then drawn from their softmax with the env's own action stream (contract: include/srlhip.h), and
// the exit store leaves that stream's counter T further on.
// POLICY = 4 (srlhip_rollout_policy_sampled; kuka_tree_policy_sample.hip): POLICY = 1 up to the six broadcast scores, discrete actions
// only (JOINTS = false), then POLICY = 3's draw (row_softmax_draw) and its counter store.
// POLICY != 0, srlhip_rollout_policy_summary (contract: include/srlhip.h): words 11 .. 14 of the header are the call's four output pointers,
// all null in a plane call — tested at run time, so that the summary form adds no instantiation to kernels that compile for minutes
// and the argument block stays the one the POLICY = 0 kernels share.  The sums are spread over the env's 16-lane row, two float64
// accumulators per lane: lane d < 3 holds dimension d's obs_sum and obs_sqsum (every lane can form the observation: the env scalars
// are replicated over the row), lane 3 the return; the row-uniform length and the latched done flag sit in every lane.  Each sum
// takes its terms in ascending t and every product is rounded before it is added (contract(off): this unit lets products fuse).
template <int MODE, bool JOINTS, bool GIVEN, int NB, int RB = 0, int SPEC = 0, int PERSIST = 0, int POLICY = 0>
__global__ void __launch_bounds__(kGroupBlock)
kuka_tree_rollout_k(KukaParams p, KukaState s, RngState rs, EpisodeStats st, int T, const void *actions, const double *noise,
                    float *obs, float *rew, uint8_t *done_out, void *act_out, PersistArgs pa) {
    static_assert(!PERSIST || GIVEN, "persistent stepping takes the caller's actions");
    static_assert(!POLICY || (!GIVEN && !PERSIST && !SPEC && !RB), "the policy source has generic, launching instantiations only");
    constexpr bool kMlp = POLICY == 2 || POLICY == 3, kDraw = POLICY == 3 || POLICY == 4;      // the score function; the selection
    static_assert(!kDraw || !JOINTS, "only discrete actions are sampled");
    using namespace grp;
    __shared__ double scratch_all[kGroupEnvs][kTS];
    const int64_t n = p.n;
    // XCD-aware block -> env map (the grid is a multiple of 8 blocks, kuka_tree.hip): workgroup b runs on XCD b % 8 and every XCD has its
    // own L2, so with env = 4 b + ... the 8 wavefronts whose 16-byte pieces make up one 128-byte line of an output plane sat on 8
    // different L2s and every line went to HBM in pieces (WRITE_SIZE 1.95x the planes, rounds 3-5).  XCD x now owns the contiguous env
    // range [x, x + 1) * nb / 8 * 4: a line is assembled in ONE L2.  Placement is a speed matter only; results do not depend on it.
    const int bid = ((int)blockIdx.x & 7) * ((int)gridDim.x >> 3) + ((int)blockIdx.x >> 3);
    if constexpr (PERSIST) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t xcc = xcd_id();
        if (threadIdx.x == 0) persist_register(pa, xcc);          // every workgroup, the padding ones too
#endif
    }
    if (bid * kGroupEnvs >= p.n) return;             // a padding block of the rounded-up grid (whole wavefront): it must not shadow env n - 1
                                                     // from another wavefront (GroupMt regenerates the env's generator state in HBM in place)
    const int e_raw = bid * kGroupEnvs + (int)(threadIdx.x / GL);
    const bool valid = e_raw < p.n;
    const int e = valid ? e_raw : p.n - 1;           // tail groups shadow the last env (every lane stays active for the cross-lane ops)
    Cfg cfg_c = p.cfg;
    if constexpr (SPEC == 1) {
        cfg_c.is_discrete = 1; cfg_c.action_joints = 0; cfg_c.random_target = 0; cfg_c.force_down = 1; cfg_c.shape_reward = 0;
        cfg_c.action_repeat = 1; cfg_c.obs_mode = 0; cfg_c.auto_reset = 1; cfg_c.moving = 0; cfg_c.two = 0; cfg_c.rand_objects = 0;
        cfg_c.max_steps = kMaxSteps;
    }
    const Cfg &cfg = cfg_c;
    __shared__ double tab[tree::kLaneTableDoubles];
    double *scratch = scratch_all[threadIdx.x / GL];
    LaneId L;
    build_lane_table(L, s.ttable, tab);
#if defined(SRL_TREE_PROF) && defined(__HIP_DEVICE_COMPILE__)
    if (threadIdx.x == 0) { unsigned long long *pp = tree::tprof_buf(); for (int i = 0; i < tree::kProfSlots; i++) pp[i] = 0; pp[tree::kProfSlots] = __builtin_amdgcn_s_memtime(); }
#endif
    const bool lead = L.l == 0 && valid;
    using Rng = std::conditional_t<MODE == SRLHIP_RNG_PHILOX, GroupPhilox, std::conditional_t<MODE == SRLHIP_RNG_MT19937, GroupMt, typename KRng<MODE>::type>>;
    Rng rng0;
    if constexpr (MODE == SRLHIP_RNG_PHILOX) rng0.init(rs.key[e], rs.key[n + e], rs.ctr[e]);
    else if constexpr (MODE == SRLHIP_RNG_MT19937) rng0.load(rs.mt, e);
    else krng_load<MODE>(rng0, rs, e, p.n, noise ? noise + e : nullptr);
    Env v = {};
    GState g;
    tload(s, n, e, L, v, g, NB == 2);
    tree::RBody body = {};
    if constexpr (RB) tload_body(s, n, e, L.l, body);
    // (requested before the forward kinematics so that their round trip overlaps it: single-step launches are latency)
    // (Monitor's record of the last finished episode is written only when an episode finishes in this launch and is not read: on
    //  host-pointer handles those two planes are mapped host memory — srlhip_episode_records — and a read / an unconditional
    //  write-back would cross PCIe in every launch)
    double ep_ret = st.ep_return[e], last_ret = 0.0, last_reward = 0.0;
    int32_t ep_len = st.ep_length[e], last_len = 0, n_fin = st.n_finished[e];
    const int32_t n_fin0 = n_fin;
    GroupActions gact; gact.init(rs.key[e], rs.key[n + e], rs.act_ctr[e]);
    tree::tfk(tree::lane_view(tab), g);
    Philox &act = gact.p;
    const int od = cfg.obs_mode == 1 ? 14 : cfg.obs_mode == 2 ? 17 : 3;
    const int adim = cfg.is_discrete ? 1 : cfg.action_joints ? 7 : 3;
    double pol_w[3] = {0.0, 0.0, 0.0}, pol_mean[3] = {0.0, 0.0, 0.0}, pol_std[3] = {1.0, 1.0, 1.0}, pol_clip = 0.0;
    bool pol_freeze = false, pol_norm = false, pol_frozen = false;
    (void)pol_w; (void)pol_mean; (void)pol_std; (void)pol_clip; (void)pol_freeze; (void)pol_norm; (void)pol_frozen;
    constexpr int kMlpU = 8, kMlpA = JOINTS ? 7 : 6;          // hidden units per lane; score rows an instantiation can need
    float mlp_w1[kMlpU][3], mlp_b1[kMlpU], mlp_w2[kMlpA][kMlpU], mlp_b2[kMlpA];
    const int mlp_A = cfg.is_discrete ? 6 : adim;
    (void)mlp_w1; (void)mlp_b1; (void)mlp_w2; (void)mlp_b2; (void)mlp_A;
    if constexpr (kMlp) {
        const double *hdr = noise;
        const int A = cfg.is_discrete ? 6 : adim, H = (int)hdr[10];
        const float *w = static_cast<const float *>(actions) + (hdr[0] != 0.0 ? (int64_t)e * (3 * H + H + A * H + A) : 0);
        const float *w2 = w + 4 * H, *b2 = w2 + A * H;
#pragma unroll
        for (int u = 0; u < kMlpU; u++) {
            const int j = L.l + GL * u;
            const bool on = j < H;
            const int jc = on ? j : 0;                        // clamped: every lane loads (inside the env's parameter block) and selects
#pragma unroll                                                // afterwards — a load under a branch would be waited for one by one
            for (int d = 0; d < 3; d++) { const float x = w[jc * 3 + d]; mlp_w1[u][d] = on ? x : 0.f; }
            { const float x = w[3 * H + jc]; mlp_b1[u] = on ? x : 0.f; }
#pragma unroll
            for (int k = 0; k < kMlpA; k++) { const float x = w2[(k < A ? k : 0) * H + jc]; mlp_w2[k][u] = on && k < A ? x : 0.f; }
        }
#pragma unroll
        for (int k = 0; k < kMlpA; k++) { const float x = b2[k < A ? k : 0]; mlp_b2[k] = L.l == 0 && k < A ? x : 0.f; }
#pragma unroll
        for (int d = 0; d < 3; d++) { pol_mean[d] = hdr[4 + d]; pol_std[d] = hdr[7 + d]; }
        pol_freeze = hdr[1] != 0.0; pol_norm = hdr[2] != 0.0; pol_clip = hdr[3];
    } else if constexpr (POLICY) {
        const double *hdr = noise;
        const int A = cfg.is_discrete ? 6 : adim;
        const double *w = static_cast<const double *>(actions) + (hdr[0] != 0.0 ? (int64_t)e * 3 * A : 0);
        const int col = L.l < A ? L.l : 0;
#pragma unroll
        for (int d = 0; d < 3; d++) { pol_w[d] = L.l < A ? w[d * A + col] : 0.0; pol_mean[d] = hdr[4 + d]; pol_std[d] = hdr[7 + d]; }
        pol_freeze = hdr[1] != 0.0; pol_norm = hdr[2] != 0.0; pol_clip = hdr[3];
    }
    double *sum_ret = nullptr, *sum_obs = nullptr, *sum_sq = nullptr;
    int32_t *sum_len = nullptr;
    double sum_a = 0.0, sum_b = 0.0;                 // this lane's two accumulators (see above)
    int32_t sum_n = 0;
    bool sum_seen = false;
    (void)sum_ret; (void)sum_obs; (void)sum_sq; (void)sum_len; (void)sum_a; (void)sum_b; (void)sum_n; (void)sum_seen;
    if constexpr (POLICY) {
        const uint64_t *words = reinterpret_cast<const uint64_t *>(noise);
        sum_ret = reinterpret_cast<double *>(words[11]); sum_len = reinterpret_cast<int32_t *>(words[12]);
        sum_obs = reinterpret_cast<double *>(words[13]); sum_sq = reinterpret_cast<double *>(words[14]);
    }
    // Every load of the prologue retires HERE.  Otherwise the compiler's wait for them sits at their first use INSIDE the loop, as
    // `s_waitcnt vmcnt(0)` — and gfx9 counts stores on the same counter, so from the second step on that wait drains the previous
    // step's output stores: a full store round trip (~1.5 k cycles) in every step of the rollout.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // Per-lane RUNNING plane pointers in VGPRs, advanced by one [n]-row per step: with the base pointers left in the kernel arguments
    // the compiler, short of SGPRs, re-read them from the kernarg segment at every store site (s_load + s_waitcnt lgkmcnt(0): four
    // scalar-cache round trips per step) and rebuilt each address with 64-bit multiplies.
    float *obs_p = obs ? obs + (int64_t)e * od : nullptr, *rew_p = rew ? rew + e : nullptr;
    uint8_t *done_p = done_out ? done_out + e : nullptr;
    char *act_p = act_out ? static_cast<char *>(act_out) + (int64_t)e * adim * 4 : nullptr;
    const char *given_p = GIVEN ? static_cast<const char *>(actions) + (int64_t)e * adim * 4 : nullptr;
    const int64_t act_stride = n * adim * 4;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(obs_p), "+v"(rew_p), "+v"(done_p), "+v"(act_p), "+v"(given_p));
#endif
    uint32_t my_seq = pa.start_seq, persist_k = 0;      // persist_k: steps since this launch
    (void)my_seq; (void)persist_k;
    bool direct = false, park_now = false;
    (void)direct; (void)park_now;
    if constexpr (PERSIST) {
#if defined(__HIP_DEVICE_COMPILE__)
        // start barrier -> 1: outputs straight to the host's mapped planes, 2: the staging copy and the copier below, 3: park
        uint32_t verdict = 0;
        if (threadIdx.x == 0) {
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
        }
        verdict = __builtin_amdgcn_readfirstlane(verdict);
        direct = verdict == 1u;
        park_now = verdict == 3u;
        if (direct) {
            obs_p = reinterpret_cast<float *>(pa.host_out) + (int64_t)e * od;
            rew_p = reinterpret_cast<float *>(pa.host_out + pa.rew_dw) + e;
            done_p = reinterpret_cast<uint8_t *>(pa.host_out + pa.done_dw) + e;
        }
#endif
    }
    for (int t = 0; (PERSIST && !park_now) || (!PERSIST && t < T); t++) {
        tree::PreDyn pre;
        tree::PreStep pre2;
        // (the launching kernel of the default configuration with the caller's actions — the per-step path of HipVecEnv — takes the same
        //  split: its action is REQUESTED first, from mapped host memory on a single-step launch, and everything in front of the action
        //  runs under that PCIe round trip)
        constexpr bool kLaunchSplit = GIVEN && !PERSIST && SPEC == 1;
        int a = 0; float ca[7] = {0, 0, 0, 0, 0, 0, 0};
        if constexpr (kLaunchSplit) {
            a = *reinterpret_cast<const int32_t *>(given_p);
            given_p += act_stride;
            tree::tphysics_pre2<0>(v, g, tab, scratch, pre2);
        }
        if constexpr (PERSIST && SPEC == 1) {
            // everything of the step that depends on the state only — dynamics, collision detection, the rows up to their right-hand
            // sides and, on a contact step, the general path's whole setup (16 k cycles of the step that sets the batch's latency) —
            // runs BEFORE the wait for the host's action
            tree::tphysics_pre2<0>(v, g, tab, scratch, pre2);
        } else if constexpr (PERSIST) {
            // the action-independent half of the step's (first) physics step — joint axes, bias forces, the mass matrix and its inverse:
            // 8 k of a free step's 53 k cycles — runs BEFORE the wait for the host's action: off the step's latency
            tree::tphysics_pre(g, tab, pre);
        }
        if constexpr (PERSIST) {
#if defined(__HIP_DEVICE_COMPILE__)
            uint32_t token = 0;
            if (threadIdx.x == 0) {
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
                    for (;;) {
                        token = __hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (token != my_seq) break;
                        __builtin_amdgcn_s_sleep(8);
                    }
                }
            }
            token = __builtin_amdgcn_readfirstlane(token);
            if (token == kPersistPark) break;
            my_seq = token;
            persist_k += 1;
            SRL_PSTAMP(0);
            asm volatile("" ::: "memory");                       // the action reads below stay behind the token (they are system-scope loads)
#endif
        }
        if constexpr (kMlp) {
            const float ob[3] = {(float)(v.grip[0] - v.bpos[0]), (float)(v.grip[1] - v.bpos[1]), (float)(v.grip[2] - v.bpos[2])};
            double x[3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                float xf = ob[d];
                if (pol_norm) xf = (float)fmin(fmax(((double)ob[d] - pol_mean[d]) / pol_std[d], -pol_clip), pol_clip);
                x[d] = (double)xf;
            }
            double part[kMlpA];
#pragma unroll
            for (int k = 0; k < kMlpA; k++) part[k] = (double)mlp_b2[k];
#pragma unroll
            for (int u = 0; u < kMlpU; u++) {
                double hu = (double)mlp_b1[u];
#pragma unroll
                for (int d = 0; d < 3; d++) hu += (double)mlp_w1[u][d] * x[d];
                hu = hu > 0.0 ? hu : 0.0;
#pragma unroll
                for (int k = 0; k < kMlpA; k++) part[k] += (double)mlp_w2[k][u] * hu;
            }
            double sc[kMlpA];
#pragma unroll
            for (int k = 0; k < kMlpA; k++) sc[k] = k < mlp_A ? mlp_row_sum(part[k]) : 0.0;      // (uniform over the grid: rows the action form has)
            if constexpr (POLICY == 3) {
                a = row_softmax_draw(sc, L.l, act, t);
            } else if (cfg.is_discrete) {
                double best = sc[0];
#pragma unroll
                for (int k = 1; k < 6; k++) if (sc[k] > best) { best = sc[k]; a = k; }      // strict: the lowest index wins a tie
            } else {
#pragma unroll
                for (int j = 0; j < kMlpA; j++) ca[j] = j < adim ? (float)sc[j] : 0.f;
            }
            if (pol_frozen) {                          // as POLICY = 1
                a = -1;
#pragma unroll
                for (int j = 0; j < 7; j++) ca[j] = 0.f;
            }
            if (act_p && lead) {
                if (cfg.is_discrete) *reinterpret_cast<int32_t *>(act_p) = a;
                else for (int j = 0; j < adim; j++) reinterpret_cast<uint32_t *>(act_p)[j] = pol_frozen ? 0x7fc00000u : __builtin_bit_cast(uint32_t, ca[j]);
            }
            if (act_p) act_p += act_stride;
        } else if constexpr (POLICY) {
            // observe() for ground truth (the host refuses the other modes), from the row's replicated scalars
            const float ob[3] = {(float)(v.grip[0] - v.bpos[0]), (float)(v.grip[1] - v.bpos[1]), (float)(v.grip[2] - v.bpos[2])};
            double score = 0.0;
#pragma unroll
            for (int d = 0; d < 3; d++) {
                float x = ob[d];
                if (pol_norm) x = (float)fmin(fmax(((double)ob[d] - pol_mean[d]) / pol_std[d], -pol_clip), pol_clip);
                score = d == 0 ? (double)x * pol_w[0] : score + (double)x * pol_w[d];
            }
            const double sc[7] = {bcast<0>(score), bcast<1>(score), bcast<2>(score), bcast<3>(score), bcast<4>(score), bcast<5>(score), bcast<6>(score)};
            if constexpr (POLICY == 4) {
                a = row_softmax_draw(sc, L.l, act, t);
            } else if (cfg.is_discrete) {
                double best = sc[0];
#pragma unroll
                for (int k = 1; k < 6; k++) if (sc[k] > best) { best = sc[k]; a = k; }      // strict: the lowest lane wins a tie
            } else {
#pragma unroll
                for (int j = 0; j < 7; j++) ca[j] = j < adim ? (float)sc[j] : 0.f;
            }
            if (pol_frozen) {                          // the reference's `None`: -1, or the all-NaN row (written as bits: this file is built with -fno-honor-nans)
                a = -1;
#pragma unroll
                for (int j = 0; j < 7; j++) ca[j] = 0.f;
            }
            if (act_p && lead) {
                if (cfg.is_discrete) *reinterpret_cast<int32_t *>(act_p) = a;
                else for (int j = 0; j < adim; j++) reinterpret_cast<uint32_t *>(act_p)[j] = pol_frozen ? 0x7fc00000u : __builtin_bit_cast(uint32_t, ca[j]);
            }
            if (act_p) act_p += act_stride;
        } else if constexpr (GIVEN) {
            if constexpr (kLaunchSplit) {
            } else if constexpr (PERSIST) {           // the same mapped row every step: re-read, never cached in a register
                if (cfg.is_discrete) a = __hip_atomic_load(reinterpret_cast<const int32_t *>(given_p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else {
                    for (int j = 0; j < adim; j++) ca[j] = __hip_atomic_load(reinterpret_cast<const float *>(given_p) + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    continuous_none(a, ca);                // a NaN row is `None` (kuka_env.hpp)
                }
            } else {
                if (cfg.is_discrete) a = *reinterpret_cast<const int32_t *>(given_p);
                else {
                    for (int j = 0; j < adim; j++) ca[j] = reinterpret_cast<const float *>(given_p)[j];
                    continuous_none(a, ca);
                }
                given_p += act_stride;
            }
        } else {
            if (cfg.is_discrete) a = gact.next(5);
            else for (int j = 0; j < adim; j += 2) {
                uint32_t o[4]; act.block(o);
                ca[j] = (float)(-1.0 + 2.0 * Philox::to_double(o[0], o[1]));
                if (j + 1 < adim) ca[j + 1] = (float)(-1.0 + 2.0 * Philox::to_double(o[2], o[3]));
            }
            if (act_p && lead) {
                if (cfg.is_discrete) *reinterpret_cast<int32_t *>(act_p) = a;
                else for (int j = 0; j < adim; j++) reinterpret_cast<float *>(act_p)[j] = ca[j];
            }
            if (act_p) act_p += act_stride;
        }
        float ca_own = 0.f;
#pragma unroll
        for (int j = 0; j < ND; j++) ca_own = L.l == j ? ca[j] : ca_own;
#if defined(SRL_PERSIST_PROF) && defined(__HIP_DEVICE_COMPILE__)
        if constexpr (PERSIST) { __builtin_amdgcn_s_waitcnt(0x0F70); SRL_PSTAMP(1); }
#endif
#if defined(SRL_TREE_PROF) && defined(__HIP_DEVICE_COMPILE__)
        { using namespace tree; SRL_TSTAMP(20); }     // loop back-edge + the agent's action (sampled or loaded)
#endif
        bool done;
        double reward;
        if constexpr ((PERSIST || kLaunchSplit) && SPEC == 1) reward = tree::tenv_step<NB, RB, 0, 0, 2>(v, g, tab, cfg, scratch, rng0, a, ca, ca_own, &done, &body, nullptr, nullptr, &pre2);
        else if constexpr (PERSIST) reward = tree::tenv_step<NB, RB, 0, SPEC ? 0 : -1, 1>(v, g, tab, cfg, scratch, rng0, a, ca, ca_own, &done, &body, nullptr, &pre);
        else reward = tree::tenv_step<NB, RB, 0, SPEC ? 0 : -1>(v, g, tab, cfg, scratch, rng0, a, ca, ca_own, &done, &body);
        ep_ret += reward; ep_len += 1; last_reward = reward;
        const int info = cfg.info_bits ? (v.ikx & 1) << 1 : 0;      // srlhip_config.info_bits: the IK conditioning flag this step ran under (before the auto-reset clears it)
        if (done) {
            last_ret = ep_ret; last_len = ep_len; n_fin += 1; ep_ret = 0.0; ep_len = 0;
            if constexpr (POLICY) pol_frozen = pol_frozen || pol_freeze;      // from the NEXT step on
            if (cfg.auto_reset) {
                double *objs = valid ? s.objs + e : nullptr;
                tree::tenv_reset<JOINTS ? 1 : 0, NB, RB>(v, g, tab, cfg, scratch, rng0, s.tstarts, s.tsettled, objs, n, &body);
                // the start-state loads retire HERE, not at their first use in the next step (where vmcnt(0) would also wait for
                // the output stores of steps that did not reset)
                __builtin_amdgcn_s_waitcnt(0x0F70);
            }
        }
        if constexpr (PERSIST) {
#if defined(__HIP_DEVICE_COMPILE__)
            // direct: plain stores to the mapped planes; otherwise agent-scope (write-through) stores to the staging copy (step_signal.hpp
            // has the reasons).  Monitor's record of an episode that ended in this step goes to its mapped plane directly (rare:
            // system-scope stores).
            SRL_PSTAMP(2);
            if (lead) {
                float ob[17];
                observe(v, cfg, ob, 1);
                if (direct) {                                    // plain stores to the mapped planes: into this XCD's L2
                    for (int j = 0; j < od; j++) obs_p[j] = ob[j];
                    *rew_p = (float)reward;
                    *done_p = (uint8_t)((int)done | info);
                } else {
                    for (int j = 0; j < od; j++) __hip_atomic_store(obs_p + j, ob[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(rew_p, (float)reward, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(done_p, (uint8_t)((int)done | info), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (done) {
                    __hip_atomic_store(st.last_return + e, last_ret, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(st.last_length + e, last_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);         // "written through" = the store counter reaching 0
            asm volatile("" ::: "memory");
            SRL_PSTAMP(3);
            // the LAST wavefront of its eighth of the workgroups (a contiguous env range) to arrive — staged form: copies that range of
            // the three planes from the staging copy to the host's, dwords, coalesced, whole lines — reports
            const int per = (int)gridDim.x >> 3, grp8 = bid / per;
            const int real = contiguous_real(grp8, (p.n + kGroupEnvs - 1) / kGroupEnvs, per);
            uint32_t last = 0;
            if (threadIdx.x == 0) last = signal_arrive(eighth_counter(pa.count, grp8), real, persist_k);
            SRL_PSTAMP(4);
            if (__builtin_amdgcn_readfirstlane(last)) {
                const int lo = grp8 * per * kGroupEnvs, hi = min(lo + per * kGroupEnvs, p.n);
                const PersistSeg seg[3] = {{pa.stage + (int64_t)lo * od, pa.host_out + (int64_t)lo * od, (hi - lo) * od},
                                           {pa.stage + pa.rew_dw + lo, pa.host_out + pa.rew_dw + lo, hi - lo},
                                           {pa.stage + pa.done_dw + lo / 4, pa.host_out + pa.done_dw + lo / 4, (hi - lo + 3) / 4}};
                if (!direct) persist_copy(seg);
                SRL_PSTAMP(5);
                signal_writeback();
                SRL_PSTAMP(6);
                if (threadIdx.x == 0) persist_post(pa, grp8, my_seq);
            }
#endif
        } else {
            if constexpr (POLICY) {
                if (sum_ret && !sum_seen && L.l < 4) {   // a live row of this call: none before it reported done; lanes 4 .. 15 hold no sum
#pragma clang fp contract(off)
                    // the row's observation as observe() writes it (ground truth: the host refuses the other modes), after the auto-reset
                    const float own = L.l == 0 ? (float)(v.grip[0] - v.bpos[0]) : L.l == 1 ? (float)(v.grip[1] - v.bpos[1]) : (float)(v.grip[2] - v.bpos[2]);
                    const double x = L.l < 3 ? (double)own : done ? 0.0 : (double)(float)reward;      // lane 3: the reporting step's reward is not counted
                    const double xx = x * x;
                    sum_a = sum_a + x;
                    sum_b = sum_b + xx;
                    sum_n += 1;
                    sum_seen = done;                     // (done is uniform over the row: lanes 0 .. 3 latch together)
                }
            }
            if (lead) {
                if (obs_p) observe(v, cfg, obs_p, 1);
                if (rew_p) *rew_p = (float)reward;
                if (done_p) *done_p = (uint8_t)((int)done | info);
            }
            if (obs_p) obs_p += n * od;
            if (rew_p) rew_p += n;
            if (done_p) done_p += n;
            if constexpr (GIVEN) {
#if defined(__HIP_DEVICE_COMPILE__)
                // early completion signal of a single-step launch (step_signal.hpp; armed: pa.done set): the last wavefront of each eighth reports
                if (pa.done && t == T - 1) {
                    if (done && lead) {          // Monitor's record: the host reads it right after the step, before the exit stores below
                        __hip_atomic_store(st.last_return + e, last_ret, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        __hip_atomic_store(st.last_length + e, last_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    const int per = (int)gridDim.x >> 3, grp8 = bid / per;
                    const uint32_t xcc = xcd_id();
                    uint32_t *cnt = eighth_counter(pa.count, grp8);
                    if (threadIdx.x == 0) step_signal_tag(cnt, xcc);
                    __builtin_amdgcn_s_waitcnt(0x0F70);
                    asm volatile("" ::: "memory");
                    const int real = contiguous_real(grp8, (p.n + kGroupEnvs - 1) / kGroupEnvs, per);
                    uint32_t last = 0;
                    if (threadIdx.x == 0) last = signal_arrive(cnt, real, pa.start_seq);
                    if (__builtin_amdgcn_readfirstlane(last)) {
                        signal_writeback();
                        if (threadIdx.x == 0) step_signal_post(pa, cnt, grp8);
                    }
                }
#endif
            }
        }
#if defined(SRL_TREE_PROF) && defined(__HIP_DEVICE_COMPILE__)
        { using namespace tree; SRL_TSTAMP(11); }     // episode statistics, auto-reset, observation + output stores
#endif
    }
#if defined(SRL_TREE_PROF) && defined(__HIP_DEVICE_COMPILE__)
    if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == 511)) {
        const unsigned long long *pp = tree::tprof_buf();
        for (int i = 0; i < tree::kProfSlots; i++) printf("tprof block %d T %d phase %d cycles %llu\n", (int)blockIdx.x, T, i, pp[i]);
    }
    // every workgroup: how many of its first wavefront's steps carried generic / joint-limit / contact rows (the launch lasts as long as
    // the wavefront with the most of them)
    if (threadIdx.x == 0) { const unsigned long long *pp = tree::tprof_buf(); printf("tprof_counts block %d T %d generic %llu limit %llu contact %llu\n", (int)blockIdx.x, T, pp[17], pp[18], pp[19]); }
#endif
    int e_out = e;
    asm volatile("" : "+v"(e_out));       // exit-store addresses are recomputed instead of being kept live across the loop
    tstore(s, n, e_out, L, v, g, valid, NB == 2);
    if constexpr (RB) tstore_body(s, n, e_out, L.l, body, valid);
    if (lead) {
        if constexpr (MODE == SRLHIP_RNG_PHILOX) rs.ctr[e_out] = rng0.p.ctr;
        else if constexpr (MODE == SRLHIP_RNG_MT19937) rng0.store(rs.mt, e_out);
        else krng_store<MODE>(rng0, rs, e_out);
        if constexpr (!GIVEN && !POLICY) rs.act_ctr[e_out] = act.ctr;
        if constexpr (kDraw) rs.act_ctr[e_out] = act.ctr + (uint64_t)T;      // c0 + T, whatever happened in between
        st.ep_return[e_out] = ep_ret; st.ep_length[e_out] = ep_len;
        if (n_fin != n_fin0) { st.last_return[e_out] = last_ret; st.last_length[e_out] = last_len; }
        st.n_finished[e_out] = n_fin; st.last_reward[e_out] = last_reward;
    }
    if constexpr (POLICY) {
        if (sum_ret && valid) {
            if (L.l < 3 && sum_obs) { sum_obs[(int64_t)e_out * 3 + L.l] = sum_a; sum_sq[(int64_t)e_out * 3 + L.l] = sum_b; }
            if (L.l == 3) sum_ret[e_out] = sum_a;
            if (L.l == 0 && sum_len) sum_len[e_out] = sum_n;
        }
    }
}

// srlhip_reset: KukaButtonGymEnv.reset by lane groups
template <int MODE, bool JOINTS, int NB, int RB = 0>
__global__ void __launch_bounds__(kGroupBlock)
kuka_tree_reset_k(KukaParams p, KukaState s, RngState rs, EpisodeStats st, const uint8_t *mask, const double *host_rand, int rand_stride, float *obs) {
    using namespace grp;
    __shared__ double scratch_all[kGroupEnvs][kTS];
    const int64_t n = p.n;
    const int e_raw = blockIdx.x * kGroupEnvs + (int)(threadIdx.x / GL);
    const bool valid = e_raw < p.n && !(mask && !mask[e_raw < p.n ? e_raw : 0]);
    const int e = e_raw < p.n ? e_raw : p.n - 1;
    __shared__ double tab[tree::kLaneTableDoubles];
    LaneId L; build_lane_table(L, s.ttable, tab);
    const bool lead = L.l == 0 && valid;
    using Rng = std::conditional_t<MODE == SRLHIP_RNG_PHILOX, GroupPhilox, std::conditional_t<MODE == SRLHIP_RNG_MT19937, GroupMt, typename KRng<MODE>::type>>;
    // A masked-out env (and the shadow rows of a tail group) must not draw: GroupMt's twist() rewrites the env's 624 state words in
    // HBM in place while its index is only stored by the lead lane of a VALID env — a masked draw across a twist boundary would
    // leave the running env with a regenerated block and a stale index.  `valid` is uniform over the 16-lane row, and every
    // cross-lane operation of the reset is row-local (the rollout kernel already runs tenv_reset under row divergence).
    if (!valid) return;
    Rng rng0;
    if constexpr (MODE == SRLHIP_RNG_PHILOX) rng0.init(rs.key[e], rs.key[n + e], rs.ctr[e]);
    else if constexpr (MODE == SRLHIP_RNG_MT19937) rng0.load(rs.mt, e);
    else krng_load<MODE>(rng0, rs, e, p.n, host_rand ? host_rand + (int64_t)e * rand_stride : nullptr);
    Env v = {};
    v.ikx = s.i[I_IKX * n + e];              // the flagged-step count outlives the episode (tenv_reset clears the sticky bit only)
    GState g;
    double *objs = s.objs + e;
    tree::RBody body = {};
    tree::tenv_reset<JOINTS ? 1 : 0, NB, RB>(v, g, tab, p.cfg, scratch_all[threadIdx.x / GL], rng0, s.tstarts, s.tsettled, objs, n, &body);
    tstore(s, n, e, L, v, g, valid, NB == 2);
    if constexpr (RB) tstore_body(s, n, e, L.l, body, valid);
    if (lead) {
        if constexpr (MODE == SRLHIP_RNG_PHILOX) rs.ctr[e] = rng0.p.ctr;
        else if constexpr (MODE == SRLHIP_RNG_MT19937) rng0.store(rs.mt, e);
        else krng_store<MODE>(rng0, rs, e);
        st.ep_return[e] = 0.0; st.ep_length[e] = 0;
        if (obs) {
            const int od = p.cfg.obs_mode == 1 ? 14 : p.cfg.obs_mode == 2 ? 17 : 3;
            observe(v, p.cfg, obs + (int64_t)e * od, 1);
        }
    }
}

// ---- launches: the ONE place per kernel template where its template arguments meet a launch ---------------------------------------
// (a new instantiation is a new arm in the dispatch of the translation unit that is to hold it; templates, so that only a unit that
//  calls one instantiates its kernels)

// the (JOINTS, NB) pairs the kernels exist for: Cartesian two buttons (Kuka2ButtonGymEnv takes discrete actions only), joint-space one
// button (compiled out with JOINT_ARM = false), Cartesian one button.  f(joints, nb)
template <bool JOINT_ARM = true, class F>
bool dispatch_tree_arm(int joints, int nb, F &&f) {
    if (nb == 2 && !joints) { f(Const<0>{}, Const<2>{}); return true; }
    if constexpr (JOINT_ARM) if (nb == 1 && joints) { f(Const<1>{}, Const<1>{}); return true; }
    if (nb == 1 && !joints) { f(Const<0>{}, Const<1>{}); return true; }
    return false;
}

// what a rollout launch passes through to kuka_tree_rollout_k
struct TreeIo { int T; const void *actions; const double *noise; float *obs, *rew; uint8_t *done; void *act_out; };

// kuka_tree_rollout_k<MODE, JOINTS, GIVEN, NB, RB, SPEC, PERSIST, POLICY>: grid (a multiple of 8 blocks: the kernel maps blocks to envs
// XCD by XCD), the early completion signal, launch, error check.  arm_signal (kuka_tree_select.hpp): a single-step launch with the
// caller's actions on a handle whose host side armed the signal (api.hip) — the kernel reports the step's outputs per eighth of the grid
// before it ends.  pa: the resident kernel's control block (PERSIST = 1), nothing otherwise.
template <int RB = 0, int SPEC = 0, int PERSIST = 0, int POLICY = 0, int MODE, int JOINTS, int GIVEN, int NB>
int tree_rollout_launch(Handle *h, const KukaParams &p, Const<MODE>, Const<JOINTS>, Const<GIVEN>, Const<NB>, bool arm_signal, const TreeIo &io,
                        PersistArgs pa = PersistArgs{}) {
    const int real = (h->n + kGroupEnvs - 1) / kGroupEnvs;
    dim3 grid(contiguous_grid(real)), block(kGroupBlock);
    if (arm_signal) {
        pa = h->step_signal; h->step_signal_armed = true;
        h->signal_eighths = contiguous_eighths(real);
    }
    hipLaunchKernelGGL((kuka_tree_rollout_k<MODE, JOINTS != 0, GIVEN != 0, NB, RB, SPEC, PERSIST, POLICY>), grid, block, 0, h->stream, p, *h->kuka, h->rng,
                       h->stats, io.T, io.actions, io.noise, io.obs, io.rew, io.done, io.act_out, pa);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

// kuka_tree_reset_k<MODE, JOINTS, NB, RB>
template <int RB, int MODE, int JOINTS, int NB>
int tree_reset_launch(Handle *h, const KukaParams &p, Const<MODE>, Const<JOINTS>, Const<NB>, const uint8_t *d_mask, const double *d_host_rand, int stride, float *obs) {
    dim3 grid((h->n + kGroupEnvs - 1) / kGroupEnvs), block(kGroupBlock);
    hipLaunchKernelGGL((kuka_tree_reset_k<MODE, JOINTS != 0, NB, RB>), grid, block, 0, h->stream, p, *h->kuka, h->rng, h->stats, d_mask, d_host_rand, stride, obs);
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

// srlhip_rollout_policy (POLICY = 1, kuka_tree_policy.hip) / srlhip_rollout_mlp_policy (POLICY = 2, kuka_tree_mlp.hip) /
// srlhip_rollout_mlp_policy_sampled (POLICY = 3, kuka_tree_mlp_sample.hip) / srlhip_rollout_policy_sampled (POLICY = 4,
// kuka_tree_policy_sample.hip): the launch all four share — {PHILOX, MT19937} x {Cartesian
// one button, joint-space actions one button, Cartesian two buttons}, generic configuration (SPEC = 0), launching form; POLICY = 3 and 4
// sample discrete actions only and have no joint-space arm (four kernels instead of six).  Every batch size runs this
// one-wavefront-per-SIMD kernel (the two-wavefront variant of kuka_tree_occ.hip has no policy form).  Instantiating it instantiates the
// kernels: once per POLICY, each in its own translation unit.
// The guard restates what the entry points have refused by name before they come here (api.hip: rollout_policy): through the ABI it
// never fires, so where a caller's own refusal stands relative to it cannot be observed.
template <int POLICY>
int kuka_tree_policy_launch(Handle *h, const char *name, int T, const PolicyArgs &pol, double *d_hdr, float *obs, float *d_rew, uint8_t *d_done, void *d_act_out,
                            const SummaryOut *sum) {
    constexpr bool kSampled = POLICY == 3 || POLICY == 4;
    const srlhip_config &c = h->cfg;
    const auto refuse = [&] { return h->fail(SRLHIP_ENOTSUP, std::string(name) + ": no policy instantiation for this Kuka configuration"); };
    if (!h->kuka || !h->kuka->full || c.env_kind == SRLHIP_ENV_KUKA_RAND || c.obs_mode != SRLHIP_OBS_GROUND_TRUTH || !c.auto_reset ||
        (kSampled && !c.is_discrete) || !tree_device_rng(c))
        return refuse();
    const KukaParams p = params_of(h);
    int rc = kuka_policy_header(h, d_hdr, pol, sum);
    if (rc) return rc;
    const bool two = c.env_kind == SRLHIP_ENV_KUKA_2BUTTON;
    const TreeIo io = {T, pol.w, d_hdr, obs, d_rew, d_done, d_act_out};
    const bool hit = dispatch_rollout_device_rng(c.rng_mode, [&](auto mode) {
        return dispatch_tree_arm<!kSampled>(!two && tree_joint_actions(c), two ? 2 : 1, [&](auto joints, auto nb) {
            rc = tree_rollout_launch<0, 0, 0, POLICY>(h, p, mode, joints, Const<0>{}, nb, false, io);
        });
    });
    return hit ? rc : refuse();
}

}  // namespace
}  // namespace srl
