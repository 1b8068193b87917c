// policy_act.hpp — the per-env arithmetic of srlhip_policy_act (contract: include/srlhip.h), host + gfx950 device code.
//
// One definition of every step that fixes a bit of the result — the policy's input, the two score functions with their summation
// ORDER, the action selection — called by the kernels of policy_act.hip and by the stand-alone host program policy_hostcheck.cpp
// (make policyhostcheck), which tests/test_policy_act_cpu.py holds to the numpy restatement tests/policy_act_ref.py bit for bit.
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

}  // namespace srl
