// policy_act.hpp — the per-env arithmetic of srlhip_policy_act (contract: include/srlhip.h), host + gfx950 device code.
//
// One definition of every step that fixes a bit of the result — the policy's input, the two score functions with their summation
// ORDER, and the finishing step behind ANY score function (act_finish: freeze bookkeeping, score plane, selection, action row; act_draw:
// the env's action-stream block) — called by the kernels of policy_act.hip, cnn_policy.hip and pixel_policy.hip and by the stand-alone
// host programs policy_hostcheck.cpp, cnn_policy_hostcheck.cpp and pixel_policy_hostcheck.cpp, which tests/test_policy_act_cpu.py,
// test_cnn_policy_cpu.py and test_pixel_policy_cpu.py hold to their numpy restatements bit for bit.
// The same steps exist inside the fused rollout kernels (mobile.hip: policy_input, row_sum16, softmax_weights, softmax_pick; the Kuka
// tree kernels): those keep their own text — moving it would change their code objects — and tests/test_gpu_policy_act.py holds
// both copies to the one reference, closed loop.  Build every user with -ffp-contract=off: no product may fuse with its sum.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rng.hpp"

namespace srl {

constexpr int kActLanes = 16;        // the virtual lane row of the MLP's second layer
constexpr int kActMaxHidden = 128, kActMaxDim = 1024, kActMaxOut = 8;

// x_d: the float32 observation, or its frozen VecNormalize image — float64, clamped, rounded back to float32 (mobile.hip: policy_input)
SRL_HD float act_input(float o, bool normalize, double mean, double sd, double clip) {
#pragma clang fp contract(off)
    if (!normalize) return o;
    return (float)fmin(fmax(((double)o - mean) / sd, -clip), clip);
}

// linear policy: score_a = sum_d (double)x_d * W[d][a], d ascending; the sum STARTS with the d = 0 product (a zero keeps its IEEE sign)
SRL_HD double act_linear_step(bool first, double acc, float x, double w) {
#pragma clang fp contract(off)
    const double t = (double)x * w;
    return first ? t : acc + t;
}

// MLP, first layer: acc starts from (double)b1_j and takes (double)W1[j][d] * (double)x_d for d ascending; then the ReLU
SRL_HD double act_hidden_step(double acc, float w, float x) {
#pragma clang fp contract(off)
    const double t = (double)w * (double)x;
    return acc + t;
}
SRL_HD double act_relu(double v) { return v > 0.0 ? v : 0.0; }

// MLP, second layer: the partial score of virtual lane l for one output — the lane's units l, l + 16, ... in that order; fc_out's bias
// sits with lane 0, the other lanes start from +0.0.  w2_row = fc_out.weight[a], h = the H hidden activations.
SRL_HD double act_lane_partial(int l, int H, const float *w2_row, float b2a, const double *h) {
#pragma clang fp contract(off)
    double p = l == 0 ? (double)b2a : 0.0;
    for (int j = l; j < H; j += kActLanes) {
        const double t = (double)w2_row[j] * h[j];
        p = p + t;
    }
    return p;
}

// the 16 partials combined in row_sum16's pattern (mobile.hip): every lane adds its partner's value, partner l ^ 1, then l ^ 2, then
// 7 - l inside each half of eight, then 15 - l.  Every lane ends with the same bits; lane 0's are returned.
SRL_HD double act_row_sum16(const double *p) {
#pragma clang fp contract(off)
    double x[kActLanes], y[kActLanes];
    for (int l = 0; l < kActLanes; l++) x[l] = p[l];
    for (int l = 0; l < kActLanes; l++) y[l] = x[l] + x[l ^ 1];
    for (int l = 0; l < kActLanes; l++) x[l] = y[l] + y[l ^ 2];
    for (int l = 0; l < kActLanes; l++) y[l] = x[l] + x[(l & 8) | (7 - (l & 7))];
    for (int l = 0; l < kActLanes; l++) x[l] = y[l] + y[15 - l];
    return x[0];
}

// discrete: the strict arg-max, the lowest index wins a tie
SRL_HD int act_argmax(const double *score, int A) {
    int a = 0;
    double best = score[0];
    for (int k = 1; k < A; k++) if (score[k] > best) { best = score[k]; a = k; }
    return a;
}

// sampled: w_k = exp(score_k - max) (this build's exp: libm on the host, the device math library on the GPU) ...
SRL_HD void act_softmax_weights(const double *score, int A, double *w) {
#pragma clang fp contract(off)
    double m = score[0];
    for (int k = 1; k < A; k++) m = score[k] > m ? score[k] : m;
    for (int k = 0; k < A; k++) w[k] = exp(score[k] - m);
}
// ... and the inverse CDF, branch-free: how many of c_0 .. c_{A-2} z = u * c_{A-1} has reached
SRL_HD int act_softmax_pick(const double *w, int A, double u) {
#pragma clang fp contract(off)
    double c[kActMaxOut];
    c[0] = w[0];
    for (int k = 1; k < A; k++) c[k] = c[k - 1] + w[k];
    const double z = u * c[A - 1];
    int a = 0;
    for (int k = 0; k < A - 1; k++) a += z >= c[k] ? 1 : 0;
    return a;
}

// freeze_after_done's bookkeeping: the env's frozen byte after this call (bit 0 of done_prev alone counts: bit 1 is info_bits')
SRL_HD uint8_t act_frozen(uint8_t frozen, bool has_done_prev, uint8_t done_prev) {
    return (uint8_t)((frozen ? 1 : 0) | (has_done_prev ? (done_prev & 1) : 0));
}

// the action row of env-local index `row`: discrete -> int32 (frozen: -1); continuous -> A float32 (frozen: NaNs on a Kuka handle,
// zeros on a MobileRobot one).  `a` is the discrete choice (argmax or the draw).
SRL_HD void act_store(void *act, int64_t row, int A, bool discrete, bool none_nan, bool frozen, int a, const double *score) {
    if (discrete) {
        static_cast<int32_t *>(act)[row] = frozen ? -1 : a;
        return;
    }
    float *out = static_cast<float *>(act) + row * A;
    for (int k = 0; k < A; k++) out[k] = frozen ? (none_nan ? __builtin_nanf("") : 0.f) : (float)score[k];
}

// one block of env e's action stream (Philox stream 1; key: the [2][n] key plane, ctr: the [n] block counters): opened at the stored
// counter, one block taken, the counter stored back — it moves inside the kernel, so a graph replay draws afresh.  A sampled call draws
// for every env, frozen or not; a call that does not sample never comes here.
SRL_HD double act_draw(const uint32_t *key, int n, uint64_t *ctr, int64_t e) {
    Philox draw;
    draw.k0 = key[e]; draw.k1 = key[n + e]; draw.stream = 1; draw.ctr = ctr[e];
    const double u = draw.double01();
    ctr[e] = draw.ctr;
    return u;
}

// What the finishing step of an action call works on besides the scores.  Passed to kernels BY VALUE inside their argument blocks.
struct ActFinish {
    const uint8_t *done_prev;    // [n] or null
    uint8_t *frozen;             // [n]: read and written only with freeze
    void *act;                   // int32 [n] / float [n][A]
    int32_t A, freeze, discrete, sample, none_nan;
};

// The finishing step of every action call, one thread per env, in this order: the freeze bookkeeping; the scores into row e of the
// score plane (score_out null: none), for a frozen env too; the selection — sample: the softmax weights (also into w_out where the
// caller wants them) and the inverse CDF at u, the caller's act_draw (unused otherwise); else, discrete, the arg-max — and the action row.
template <class S>
SRL_HD void act_finish(const ActFinish &f, int64_t e, const double *score, S *score_out, double u, double *w_out = nullptr) {
    bool frozen = false;
    if (f.freeze) {
        const uint8_t b = act_frozen(f.frozen[e], f.done_prev != nullptr, f.done_prev ? f.done_prev[e] : (uint8_t)0);
        f.frozen[e] = b;
        frozen = b != 0;
    }
    if (score_out)
        for (int k = 0; k < f.A; k++) score_out[e * f.A + k] = (S)score[k];
    int choice = 0;
    if (f.sample) {
        double wl[kActMaxOut], *w = w_out ? w_out : wl;
        act_softmax_weights(score, f.A, w);
        choice = act_softmax_pick(w, f.A, u);
    } else if (f.discrete) choice = act_argmax(score, f.A);
    act_store(f.act, e, f.A, f.discrete != 0, f.none_nan != 0, frozen, choice, score);
}

}  // namespace srl
