// api_rules_hostcheck.cpp — every rule of api_rules.hpp over its case space, as a stand-alone host program that includes nothing else of
// the library.  TESTS ONLY (make apiruleshostcheck; tests/test_api_rules_cpu.py compares every line with its own restatement of the rules).
//   api_rules_hostcheck TABLES      TABLES: srlhip_kuka_default_model's 138 doubles, then srlhip_kuka_tree_default_model's 510
// One line per case on stdout, "<section> <inputs> | <outputs>"; a verdict prints as "<code> <message>" ("0 -" = accepted).
//   default  kind | every field of fill_default_config's result, in declaration order
//   cfg      kind disc obs_mode joints random_target multi_view rng_mode auto_reset kuka_model info_bits action_repeat side num_envs
//            | obs_dim num_actions action_dim frame_bytes obs_bytes action_bytes(3) policy_outputs reset_rand_count | check_config
//   layout   kind disc joints obs_mode side multi_view io_device zero_copy_enabled n | ob ab in_noise in_total out_rew out_done out_total pixels zero_copy
//   bound    n | out_total zero_copy      ground-truth MobileRobotGymEnv: the largest n of a zero-copy step, and the next
//   rows     dim pattern | all_finite_f32 kuka_rows_ok              three rows of `dim`; the middle one carries the pattern
//   actions  kind joints pattern | continuous_actions_ok
//   discrete top value | copy_discrete_checked, the copy
//   model / tree  case | the table check       policy-*: the policy checks (see main)
//   jpeg     side multi_view n blob_cap | ch ns cap frames off_at ovf_at blob_at bytes(io_device 0) bytes(1)
//   episodes n | block bytes, byte offset of the lengths
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <vector>

#include "api_rules.hpp"

using namespace srl;

static void verdict(const Verdict &v) { printf("%d %s\n", v.code, v.code ? v.msg : "-"); }

static void configs() {
    srlhip_config c = {};
    c.struct_size = (int32_t)sizeof c;
    const int sides[4] = {7, 8, 1024, 1025};
    for (int kind = -1; kind <= 8; kind++) for (int disc = 0; disc < 2; disc++) for (int om = 0; om <= 4; om++) for (int joints = 0; joints < 2; joints++)
    for (int rt = 0; rt < 2; rt++) for (int mv = 0; mv < 2; mv++) for (int mode = -1; mode <= 3; mode++) for (int ar = 0; ar < 2; ar++)
    for (int km = 0; km <= 2; km++) for (int ib = 0; ib <= 2; ib++) for (int rep = 0; rep < 2; rep++) for (int side : sides) for (int n = 0; n < 2; n++) {
        c.env_kind = kind; c.is_discrete = disc; c.obs_mode = om; c.action_joints = joints; c.random_target = rt; c.multi_view = mv; c.rng_mode = mode;
        c.auto_reset = ar; c.kuka_model = km; c.info_bits = ib; c.action_repeat = rep; c.img_h = c.img_w = side; c.num_envs = n;
        printf("cfg %d %d %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %zu %zu %zu %zu %d | ", kind, disc, om, joints, rt, mv, mode, ar, km, ib, rep, side, n,
               obs_dim_of(c), num_actions_of(c), action_dim_of(c), frame_bytes(c), obs_bytes_per_env(c), action_bytes(c, 3), policy_outputs(c), reset_rand_count(c));
        verdict(check_config(c));
    }
    // the image sides are checked one by one, and the struct size first of all
    for (int k = 0; k < 4; k++) {
        fill_default_config(SRLHIP_ENV_MOBILE, &c);
        c.img_h = k == 0 ? 7 : k == 1 ? 1025 : 224; c.img_w = k == 2 ? 7 : k == 3 ? 1025 : 224;
        printf("cfg-side %d %d | ", c.img_h, c.img_w);
        verdict(check_config(c));
    }
    fill_default_config(SRLHIP_ENV_MOBILE, &c);
    c.struct_size = 4; c.num_envs = 0;
    printf("cfg-size 4 | ");
    verdict(check_config(c));
}

static void defaults() {
    for (int kind = 0; kind <= SRLHIP_ENV_LAST; kind++) {
        srlhip_config c;
        memset(&c, 0xff, sizeof c);
        fill_default_config(kind, &c);
        printf("default %d | %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %.17g\n", kind, c.struct_size, c.env_kind, c.num_envs, c.device_id,
               c.first_env_id, c.is_discrete, c.random_target, c.force_down, c.shape_reward, c.action_repeat, c.action_joints, c.obs_mode, c.img_h, c.img_w,
               c.multi_view, c.rng_mode, c.auto_reset, c.io_device, c.kuka_model, c.info_bits, (long long)c.seed0, c.max_distance);
    }
}

static void print_layout(const srlhip_config &c, int zc, size_t n) {
    const StepLayout L = step_layout(c, n, zc != 0);
    printf("layout %d %d %d %d %d %d %d %d %zu | %zu %zu %zu %zu %zu %zu %zu %d %d\n", c.env_kind, c.is_discrete, c.action_joints, c.obs_mode, c.img_h, c.multi_view,
           c.io_device, zc, n, L.ob, L.ab, L.in_noise, L.in_total, L.out_rew, L.out_done, L.out_total, (int)L.pixels, (int)L.zero_copy);
}
static void layouts() {
    const size_t ns[4] = {1, 3, 5, 4096};
    srlhip_config c;
    for (int kind = 0; kind <= SRLHIP_ENV_LAST; kind++) for (int disc = 0; disc < 2; disc++) for (int joints = 0; joints < 2; joints++) for (int om = 0; om <= 3; om++)
    for (int mv = 0; mv < 2; mv++) for (int io = 0; io < 2; io++) for (int zc = 0; zc < 2; zc++) for (size_t n : ns) {
        fill_default_config(kind, &c);
        c.is_discrete = disc; c.action_joints = joints; c.obs_mode = om; c.img_h = c.img_w = 8; c.multi_view = mv; c.io_device = io;
        print_layout(c, zc, n);
    }
    // the zero-copy bound on ground-truth MobileRobotGymEnv: out_total grows with n, so the largest n within the bound is found by bisection
    fill_default_config(SRLHIP_ENV_MOBILE, &c);
    size_t lo = 1, hi = (size_t)1 << 20;                          // lo fits, hi does not
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        (step_layout(c, mid, true).out_total <= kZeroCopyMaxBytes ? lo : hi) = mid;
    }
    for (size_t n : {lo, hi}) {
        const StepLayout L = step_layout(c, n, true);
        printf("bound %zu | %zu %d\n", n, L.out_total, (int)L.zero_copy);
    }
}

// three rows of `dim` floats, finite but for the middle row: 0 finite, 1 all NaN, 2 NaN first, 3 NaN last, 4 +inf first, 5 -inf last, 6 NaN and +inf
static std::vector<float> rows_of(int dim, int pattern) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> a(3 * (size_t)dim);
    for (size_t i = 0; i < a.size(); i++) a[i] = 0.25f * (float)i - 1.0f;
    float *r = a.data() + dim;
    if (pattern == 1) for (int j = 0; j < dim; j++) r[j] = nan;
    if (pattern == 2) r[0] = nan;
    if (pattern == 3) r[dim - 1] = nan;
    if (pattern == 4) r[0] = inf;
    if (pattern == 5) r[dim - 1] = -inf;
    if (pattern == 6) { for (int j = 0; j < dim; j++) r[j] = nan; r[dim - 1] = inf; }
    return a;
}
static void caller_data() {
    for (int dim : {2, 3, 7}) for (int pattern = 0; pattern <= 6; pattern++) {
        const std::vector<float> a = rows_of(dim, pattern);
        printf("rows %d %d | %d %d\n", dim, pattern, (int)all_finite_f32(a.data(), a.size()), (int)kuka_rows_ok(a.data(), 3, dim));
    }
    for (int kind : {SRLHIP_ENV_MOBILE, SRLHIP_ENV_MOBILE_LINE, SRLHIP_ENV_KUKA_BUTTON, SRLHIP_ENV_KUKA_2BUTTON}) for (int joints = 0; joints < 2; joints++)
    for (int pattern = 0; pattern <= 6; pattern++) {
        srlhip_config c;
        fill_default_config(kind, &c);
        c.is_discrete = 0; c.action_joints = joints;
        const std::vector<float> a = rows_of(action_dim_of(c), pattern);
        printf("actions %d %d %d | %d\n", kind, joints, pattern, (int)continuous_actions_ok(c, a.data(), 3));
    }
    const double dnan = std::numeric_limits<double>::quiet_NaN(), dinf = std::numeric_limits<double>::infinity();
    const double noise[4][3] = {{0.0, -1.5, 2.0}, {0.0, dnan, 2.0}, {dinf, 0.0, 0.0}, {0.0, 0.0, -dinf}};
    for (int k = 0; k < 4; k++) printf("noise %d | %d\n", k, (int)all_finite_f64(noise[k], 3));
    for (int32_t top : {2, 4, 6}) for (int32_t value : {-2, -1, top - 1, top}) {
        const int32_t src[3] = {0, value, top - 1};
        int32_t dst[3] = {99, 99, 99};
        const bool ok = copy_discrete_checked(src, dst, 3, top);
        printf("discrete %d %d | %d %d %d %d\n", top, value, (int)ok, dst[0], dst[1], dst[2]);
    }
}

static void models(const char *path) {
    static_assert(sizeof(srlhip_kuka_model) == 138 * 8 && sizeof(srlhip_kuka_tree_model) == 510 * 8, "the tables are arrays of doubles");
    srlhip_kuka_model m0;
    srlhip_kuka_tree_model t0;
    FILE *f = fopen(path, "rb");
    if (!f || fread(&m0, sizeof m0, 1, f) != 1 || fread(&t0, sizeof t0, 1, f) != 1) { fprintf(stderr, "cannot read the default tables\n"); exit(2); }
    fclose(f);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const auto lumped = [&](const char *name, auto &&edit) { srlhip_kuka_model m = m0; edit(m); printf("model %s | ", name); verdict(check_kuka_model(m)); };
    lumped("default", [](srlhip_kuka_model &) {});
    lumped("mass0-zero", [](srlhip_kuka_model &m) { m.mass[0] = 0.0; });
    lumped("mass6-negative", [](srlhip_kuka_model &m) { m.mass[6] = -1.0; });
    lumped("mass3-nan", [&](srlhip_kuka_model &m) { m.mass[3] = nan; });
    lumped("inertia-x", [](srlhip_kuka_model &m) { m.inertia[2][0] = 0.0; });
    lumped("inertia-y", [](srlhip_kuka_model &m) { m.inertia[2][1] = -1e-3; });
    lumped("inertia-z", [&](srlhip_kuka_model &m) { m.inertia[6][2] = nan; });
    lumped("limits-equal", [](srlhip_kuka_model &m) { m.joint_lower[4] = m.joint_upper[4]; });
    lumped("limits-swapped", [](srlhip_kuka_model &m) { const double u = m.joint_upper[0]; m.joint_upper[0] = m.joint_lower[0]; m.joint_lower[0] = u; });
    lumped("limits-nan", [&](srlhip_kuka_model &m) { m.joint_upper[1] = nan; });
    const auto tree = [&](const char *name, auto &&edit) { srlhip_kuka_tree_model m = t0; edit(m); printf("tree %s | ", name); verdict(check_kuka_tree_model(m)); };
    using T = srlhip_kuka_tree_model;
    tree("default", [](T &) {});
    tree("nd-11", [](T &m) { m.nd = 11; });
    tree("nd-13", [](T &m) { m.nd = 13; });
    tree("nsphere-negative", [](T &m) { m.nsphere = -1; });
    tree("nsphere-17", [](T &m) { m.nsphere = 17; });
    tree("nsphere-0", [](T &m) { m.nsphere = 0; });
    tree("rows-negative", [](T &m) { m.max_generic_rows = -1; });
    tree("rows-7", [](T &m) { m.max_generic_rows = 7; });
    tree("rows-6", [](T &m) { m.max_generic_rows = 6; });
    tree("ee-link-5", [](T &m) { m.ee_link = 5; });
    tree("grip-link-negative", [](T &m) { m.grip_link = -1; });
    tree("grip-link-12", [](T &m) { m.grip_link = 12; });
    tree("parent-self", [](T &m) { m.j[9].parent = 9; });
    tree("parent-below-root", [](T &m) { m.j[0].parent = -2; });
    tree("mass-zero", [](T &m) { m.j[11].mass = 0; });
    tree("mass-nan", [&](T &m) { m.j[0].mass = nan; });
    tree("inertia-xx", [](T &m) { m.j[5].inertia[0] = 0; });
    tree("inertia-yy", [](T &m) { m.j[5].inertia[3] = -1; });
    tree("inertia-zz", [&](T &m) { m.j[5].inertia[5] = nan; });
    tree("axis-long", [](T &m) { for (double &a : m.j[7].axis) a *= 1.01; });
    tree("axis-zero", [](T &m) { for (double &a : m.j[2].axis) a = 0; });
    tree("max-force-zero", [](T &m) { m.j[8].max_force = 0; });
    tree("kp-negative", [](T &m) { m.j[1].kp = -0.3; });
    tree("arm-not-serial", [](T &m) { m.j[3].parent = 1; });
    tree("gripper-reparented", [](T &m) { m.j[8].parent = 0; });
    tree("two-clauses-joint-first", [](T &m) { m.j[3].parent = 1; m.j[2].mass = 0; });
    tree("two-clauses-header-first", [](T &m) { m.nd = 11; m.j[2].mass = 0; });
    tree("detail-half", [](T &m) { m.solver_detail = 0.5; });
    tree("detail-negative", [](T &m) { m.solver_detail = -1; });
    tree("detail-8", [](T &m) { m.solver_detail = 8; });
    tree("detail-7", [](T &m) { m.solver_detail = 7; });
    tree("contact-erp-negative", [](T &m) { m.contact_erp = -0.1; });
    tree("contact-erp-nan", [&](T &m) { m.contact_erp = nan; });
    tree("limit-erp-high", [](T &m) { m.limit_erp = 1.1; });
    tree("slop-high", [](T &m) { m.linear_slop = 0.02; });
    tree("slop-negative", [](T &m) { m.linear_slop = -1e-6; });
    tree("slop-top", [](T &m) { m.linear_slop = 0.01; });
    tree("sphere-link-negative", [](T &m) { m.s[0].link = -1; });
    tree("sphere-link-12", [](T &m) { m.s[1].link = 12; });
    tree("sphere-radius-zero", [](T &m) { m.s[0].r = 0; });
    tree("sphere-unused-bad", [](T &m) { m.nsphere = 8; m.s[8].r = 0; });
    tree("two-clauses-solver-first", [](T &m) { m.s[0].r = 0; m.limit_erp = 2; });
}

static void policies() {
    const double w64[3] = {0.5, -1.0, 2.0}, mean[3] = {0, 0, 0}, std3[3] = {1, 1, 1};
    const float w32[3] = {0.5f, -1.0f, 2.0f};
    srlhip_linear_policy lin = {};
    lin.struct_size = (int32_t)sizeof lin; lin.weights = w64; lin.clip_obs = 10.0;
    srlhip_mlp_policy mlp = {};
    mlp.struct_size = (int32_t)sizeof mlp; mlp.hidden = 100; mlp.params = w32; mlp.clip_obs = 10.0;
    // 1. the ABI checks
    printf("policy-abi linear null | "); verdict(check_policy_abi((const srlhip_linear_policy *)nullptr));
    printf("policy-abi mlp null | "); verdict(check_policy_abi((const srlhip_mlp_policy *)nullptr));
    for (int32_t size : {(int32_t)sizeof lin, (int32_t)sizeof lin - 8, (int32_t)sizeof mlp, 0}) { srlhip_linear_policy p = lin; p.struct_size = size; printf("policy-abi linear %d | ", size); verdict(check_policy_abi(&p)); }
    for (int32_t size : {(int32_t)sizeof mlp, (int32_t)sizeof mlp + 8, (int32_t)sizeof lin, 0}) { srlhip_mlp_policy p = mlp; p.struct_size = size; printf("policy-abi mlp %d | ", size); verdict(check_policy_abi(&p)); }
    // 2. the shape checks; the linear policy has none
    for (int32_t hidden : {-1, 0, 1, 100, 128, 129}) for (int32_t reserved : {0, 1}) {
        srlhip_mlp_policy p = mlp; p.hidden = hidden; p.reserved = reserved;
        printf("policy-shape mlp %d %d | ", hidden, reserved); verdict(check_policy_shape(policy_view(p)));
    }
    printf("policy-shape linear | "); verdict(check_policy_shape(policy_view(lin)));
    // 3. the pointers: w given, normalize, mean given, std given
    for (int is_mlp = 0; is_mlp < 2; is_mlp++) for (int w = 0; w < 2; w++) for (int norm = 0; norm < 2; norm++) for (int m = 0; m < 2; m++) for (int s = 0; s < 2; s++) {
        srlhip_linear_policy a = lin; a.weights = w ? w64 : nullptr; a.normalize = norm; a.obs_mean = m ? mean : nullptr; a.obs_std = s ? std3 : nullptr;
        srlhip_mlp_policy b = mlp; b.params = w ? w32 : nullptr; b.normalize = norm; b.obs_mean = m ? mean : nullptr; b.obs_std = s ? std3 : nullptr;
        const PolicyView v = is_mlp ? policy_view(b) : policy_view(a);
        printf("policy-pointers %s %d %d %d %d | ", v.what, w, norm, m, s); verdict(check_policy_pointers(v));
    }
    // parameters per policy
    for (int kind = 0; kind <= SRLHIP_ENV_LAST; kind++) for (int disc = 0; disc < 2; disc++) for (int joints = 0; joints < 2; joints++) for (int32_t hidden : {0, 1, 100}) {
        srlhip_config c;
        fill_default_config(kind, &c);
        c.is_discrete = disc; c.action_joints = joints;
        srlhip_mlp_policy b = mlp; b.hidden = hidden;
        printf("policy-params %d %d %d %d | %zu\n", kind, disc, joints, hidden, policy_param_count(c, hidden ? policy_view(b) : policy_view(lin)));
    }
    // 4. what the fused rollouts refuse by name
    for (int mode = 0; mode < 2; mode++) for (int ar = 0; ar < 2; ar++) for (int om = 0; om <= 3; om++) for (int kind : {SRLHIP_ENV_MOBILE, SRLHIP_ENV_KUKA_BUTTON, SRLHIP_ENV_KUKA_RAND})
    for (int km = 0; km < 2; km++) for (int disc = 0; disc < 2; disc++) for (int sample = 0; sample < 2; sample++) {
        srlhip_config c;
        fill_default_config(kind, &c);
        c.rng_mode = mode; c.auto_reset = ar; c.obs_mode = om; c.kuka_model = km; c.is_discrete = disc;
        printf("policy-config %d %d %d %d %d %d %d | ", mode, ar, om, kind, km, disc, sample); verdict(check_rollout_policy_config(c, sample != 0));
    }
    // 5. the values: which of (parameter 1, mean 1, std 1) carries which bad value (0 none, 1 NaN, 2 +inf; std also 3 zero, 4 negative)
    const double bad64[5] = {1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), 0.0, -1.0};
    for (int is_mlp = 0; is_mlp < 2; is_mlp++) for (int norm = 0; norm < 2; norm++) for (int bw = 0; bw < 3; bw++) for (int bm = 0; bm < 3; bm++) for (int bs = 0; bs < 5; bs++) {
        double w[3] = {0.5, bad64[bw], 2.0}, m3[3] = {0.0, bm ? bad64[bm] : 0.0, 0.0}, s3[3] = {1.0, bad64[bs], 2.0};
        float wf[3] = {0.5f, (float)bad64[bw], 2.0f};
        srlhip_linear_policy a = lin; a.weights = w; a.normalize = norm; a.obs_mean = m3; a.obs_std = s3;
        srlhip_mlp_policy b = mlp; b.params = wf; b.normalize = norm; b.obs_mean = m3; b.obs_std = s3;
        const PolicyView v = is_mlp ? policy_view(b) : policy_view(a);
        printf("policy-values %s %d %d %d %d | ", v.what, norm, bw, bm, bs); verdict(check_policy_values(v, 3, 3));
    }
    // srlhip_policy_act's own checks
    for (int l = 0; l < 2; l++) for (int m = 0; m < 2; m++) { printf("act-which %d %d | ", l, m); verdict(check_policy_act_which(l != 0, m != 0)); }
    for (int32_t obs_dim : {0, 1, 1024, 1025}) for (int sample = 0; sample < 2; sample++) for (int is_mlp = 0; is_mlp < 2; is_mlp++) {
        printf("act-shape %d %d %d | ", obs_dim, sample, is_mlp); verdict(check_policy_act_shape(obs_dim, sample != 0, is_mlp != 0));
    }
    for (int obs = 0; obs < 2; obs++) for (int act = 0; act < 2; act++) for (int freeze = 0; freeze < 2; freeze++) for (int frozen = 0; frozen < 2; frozen++)
    for (int io = 0; io < 2; io++) for (int sample = 0; sample < 2; sample++) for (int disc = 0; disc < 2; disc++) {
        srlhip_config c;
        fill_default_config(SRLHIP_ENV_KUKA_BUTTON, &c);
        c.io_device = io; c.is_discrete = disc;
        srlhip_mlp_policy b = mlp; b.freeze_after_done = freeze;
        printf("act-planes %d %d %d %d %d %d %d | ", obs, act, freeze, frozen, io, sample, disc);
        verdict(check_policy_act_planes(c, policy_view(b), sample != 0, obs != 0, act != 0, frozen != 0));
    }
}

// srlhip_rollout_policy_summary's own argument checks (`api_rules_hostcheck summary`: a table of its own, after the ones above were pinned
// line by line); the config rules it shares with the plane calls are the policy-config rows above
static void summary() {
    double ret[1], sum[1], sq[1];
    int32_t len[1];
    printf("summary null | "); verdict(check_rollout_summary(nullptr));
    for (int32_t size : {(int32_t)sizeof(srlhip_rollout_summary), (int32_t)sizeof(srlhip_rollout_summary) - 8, 0}) for (int32_t reserved : {0, 1})
    for (int r = 0; r < 2; r++) for (int l = 0; l < 2; l++) for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) {
        const srlhip_rollout_summary o = {size, reserved, r ? ret : nullptr, l ? len : nullptr, a ? sum : nullptr, b ? sq : nullptr};
        printf("summary %d %d %d %d %d %d | ", size, reserved, r, l, a, b); verdict(check_rollout_summary(&o));
    }
    printf("summary-size | %zu\n", sizeof(srlhip_rollout_summary));
}

static void scratch() {
    for (int side : {8, 9, 224}) for (int mv = 0; mv < 2; mv++) for (size_t n : {(size_t)1, (size_t)5}) for (int64_t blob_cap : {(int64_t)0, (int64_t)1000, (int64_t)65536}) {
        srlhip_config c;
        fill_default_config(SRLHIP_ENV_KUKA_BUTTON, &c);
        c.img_h = side; c.img_w = side + 8; c.multi_view = mv;
        const JpegScratch s = jpeg_scratch(c, n, blob_cap);
        printf("jpeg %d %d %zu %lld | %d %zu %lld %zu %zu %zu %zu %zu %zu\n", side, mv, n, (long long)blob_cap, s.ch, s.ns, (long long)s.cap, s.frames, s.off_at, s.ovf_at,
               s.blob_at, s.bytes(false), s.bytes(true));
    }
    for (size_t n : {(size_t)1, (size_t)3, (size_t)5, (size_t)4096}) {
        std::vector<uint8_t> block(episode_block_bytes(n));
        printf("episodes %zu | %zu %td %td\n", n, block.size(), reinterpret_cast<uint8_t *>(episode_returns(block.data())) - block.data(),
               reinterpret_cast<uint8_t *>(episode_lengths(block.data(), n)) - block.data());
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: api_rules_hostcheck TABLES | summary\n"); return 2; }
    if (!strcmp(argv[1], "summary")) { summary(); return fflush(stdout) == 0 && !ferror(stdout) ? 0 : 2; }
    defaults();
    configs();
    layouts();
    caller_data();
    models(argv[1]);
    policies();
    scratch();
    return fflush(stdout) == 0 && !ferror(stdout) ? 0 : 2;
}
