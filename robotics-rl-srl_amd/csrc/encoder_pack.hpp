// encoder_pack.hpp — the SRL encoder's host logic as plain C++17: no HIP types, no handle, no environment reads.  The frame-shape
// arithmetic, the packers that turn torch-layout weights (BatchNorms folded) into the MFMA B-operand images of encoder.hip and
// encoder_general.hip, the layout of the fused kernel's float parameter block and the choice among its instantiations — one definition
// each.  A stand-alone host program (encoder_pack_hostcheck.cpp, make encoderpackhostcheck) writes every image out, plain and under the
// address / undefined-behaviour sanitizers; tests/test_encoder_pack_hostcheck_cpu.py holds them to the library's C-ABI and to recorded
// digests.
// The reference transposes H and W before the network (models.py:185-188); all layers are symmetric in the two spatial dims, so the
// kernels work on the frame as rasterised and the packers swap the kernel axes: the tap at frame offset (ky, kx) is torch's
// w[o][c][kx][ky], and the FC's flatten order is swapped likewise.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

namespace srlenc {

// ---- frame shapes ----------------------------------------------------------------------------------------------------------------------
struct Geometry {
    int H, W, C;                 // frame rows, columns, channels (3 or 6)
    int Hc[3], Wc[3];            // convolution output of layer 1..3
    int Hp[3], Wp[3];            // after that layer's 3x3/2 max-pool
    bool ok;
};
// conv7x7/2 p3 + pool3/2 p1 -> conv3x3 p1 + pool3/2 -> conv3x3/2 p1 + pool3/2 (floor mode, like torch)
inline Geometry geometry(int img_h, int img_w, int n_channels) {
    Geometry g;
    g.H = img_h; g.W = img_w; g.C = n_channels;
    int h = img_h, w = img_w;
    const int k[3] = {7, 3, 3}, s[3] = {2, 1, 2}, pad[3] = {3, 1, 1}, ppad[3] = {1, 0, 0};
    g.ok = (n_channels == 3 || n_channels == 6) && img_h >= 8 && img_w >= 8 && img_h <= 1024 && img_w <= 1024;
    for (int l = 0; l < 3; l++) {
        g.Hc[l] = (h + 2 * pad[l] - k[l]) / s[l] + 1; g.Wc[l] = (w + 2 * pad[l] - k[l]) / s[l] + 1;
        g.Hp[l] = g.Hc[l] + 2 * ppad[l] >= 3 ? (g.Hc[l] + 2 * ppad[l] - 3) / 2 + 1 : 0;
        g.Wp[l] = g.Wc[l] + 2 * ppad[l] >= 3 ? (g.Wc[l] + 2 * ppad[l] - 3) / 2 + 1 : 0;
        if (g.Hp[l] < 1 || g.Wp[l] < 1) g.ok = false;
        h = g.Hp[l]; w = g.Wp[l];
    }
    return g;
}
// inputs of the fully connected layer: 64 channels x the last pooled map, 0 for a shape that is not covered
inline int feature_count(const Geometry &g) { return g.ok ? 64 * g.Hp[2] * g.Wp[2] : 0; }

// ---- constants of the packed images ----------------------------------------------------------------------------------------------------
constexpr float kMean[3] = {0.485f, 0.456f, 0.406f}, kStd[3] = {0.229f, 0.224f, 0.225f};      // preprocessImage's ImageNet statistics
constexpr float kWeightTop = 16384.f;        // split-f16 layers: largest |weight| after the layer's power-of-two pre-scale
constexpr int kScaleClamp = 40;              // ... whose exponent stays within +-40
// int8 layer 1 (3-channel frames): three balanced base-256 digits, most significant first, of per-channel 24-bit fixed-point weights; the
// validity-mask byte of an inside pixel is 127 (its tap carries weight / 127: same scale as the colour taps)
constexpr int kI8Steps = 7, kI8Digits = 3, kMaskI8 = 127, kWeightTopI8 = 127 * 65536 + 127 * 256 + 127, kScaleClampI8 = 60;
constexpr double kOffsetI8 = 128.0 / 255.0;  // the int8 colour taps multiply p - 128
constexpr size_t kStepBytes = 2048;          // one k-step (K = 16) of a split-f16 image: [64 lanes][8 hi | 8 lo] f16
constexpr int kSteps3x3 = 36;                // layers 2-3: K = 9 taps x 64 channels = 576
// layer 1, split f16: a staged pixel is cpix f16 — (c_0 .. c_{C-1}, mask[, 0]) —, K = 7 kernel rows x 8 pixel slots x cpix
constexpr int layer1_cpix(int C) { return C == 3 ? 4 : 8; }
constexpr int layer1_steps(int C) { return 7 * 8 * layer1_cpix(C) / 16; }                    // 14 | 28
constexpr size_t layer1_bytes(int C) { return 2 * layer1_steps(C) * kStepBytes; }
constexpr size_t kPack3x3Bytes = 2 * kSteps3x3 * kStepBytes;
constexpr size_t kPackI8Bytes = 2 * kI8Steps * kI8Digits * 64 * 16;                           // [n-half][kernel row][digit][lane][16 i8]
constexpr size_t kPackFusedBytes = layer1_bytes(3) + 2 * kPack3x3Bytes;                       // the fused kernel's b1 | b2 | b3

// The fused kernel's float parameter block: inv_scale[3] pad bias2[64] bias3[64] fcw[state_dim][64] fcb[state_dim] (float offsets; fcw
// rows are 16-byte aligned for float4 loads)
constexpr size_t kF32InvScale = 0, kF32Bias2 = 4, kF32Bias3 = kF32Bias2 + 64, kF32Fcw = kF32Bias3 + 64;
constexpr size_t f32_fcb(int state_dim) { return kF32Fcw + (size_t)state_dim * 64; }
constexpr size_t f32_count(int state_dim) { return f32_fcb(state_dim) + (size_t)state_dim; }

// ---- which instantiation of the fused kernel runs a handle -----------------------------------------------------------------------------
// encoder_fwd_k<PROF, MG, I8>: MG wave groups along M (2 = 4 waves per workgroup, one per SIMD; 4 = 8 waves), layer 1 on the int8 pipe
struct FusedVariant { int groups; bool l1_i8; };
constexpr FusedVariant kFusedVariants[3] = {{2, true}, {2, false}, {4, false}};
constexpr int fused_variant(int groups, bool l1_i8) { return groups == 2 && l1_i8 ? 0 : groups == 2 ? 1 : 2; }
// the two experiment knobs, as read by the caller (0 = unset): SRLHIP_ENCODER_WAVES = 4 | 8 waves per workgroup; SRLHIP_ENCODER_L1=f16
// keeps the split-f16 layer 1, which the two-waves-per-SIMD form always runs
constexpr int fused_groups(int waves) { return waves == 8 ? 4 : 2; }
constexpr bool fused_l1_i8(int groups, bool want_f16) { return groups == 2 && !want_f16; }

// ---- packers ---------------------------------------------------------------------------------------------------------------------------
inline void split_f16(float v, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}
// largest power of two that keeps wmax * scale <= top, its exponent clamped to +-clamp; 1 for an all-zero or non-finite layer
inline double pow2_scale(double top, double wmax, int clamp) {
    int e = 0;
    if (wmax > 0.0 && std::isfinite(wmax)) {
        frexp(top / wmax, &e);                     // top / wmax = f * 2^e, f in [0.5, 1)
        e = e - 1 > clamp ? clamp : (e - 1 < -clamp ? -clamp : e - 1);
    }
    return ldexp(1.0, e);
}
// split-f16 layers: the lo parts then sit well inside f16's normal range
inline float pick_scale(double wmax) { return (float)pow2_scale((double)kWeightTop, wmax, kScaleClamp); }

// The folded layer-1 tap of output o at frame offset (ky, kx) for staged channel c, conv1_w [64][C][7][7] (torch OIHW), conv1_b [64],
// C = 3 or 6.  c < C: the colour tap w / (255 std_c), which multiplies the pixel byte minus 255 * offset; c = C: the validity-mask tap
// (mask value inside the frame, 0 in the padding ring) [sum_c w_c (offset - mean_c) / std_c + the folded BN bias on the centre tap] /
// mask — zero padding stays exact in NORMALISED space; c > C: fill.  Split f16: offset 0, mask 1.  int8: offset 128 / 255, mask 127.
inline double layer1_weight(const float *w, const float *b, int C, int o, int ky, int kx, int c, double offset, double mask) {
    if (c < C) return (double)w[((o * C + c) * 7 + kx) * 7 + ky] / (255.0 * (double)kStd[c % 3]);
    if (c > C) return 0.0;
    double v = 0.0;
    for (int cc = 0; cc < C; cc++) v += (double)w[((o * C + cc) * 7 + kx) * 7 + ky] * (offset - (double)kMean[cc % 3]) / (double)kStd[cc % 3];
    if (ky == 3 && kx == 3) v += (double)b[o];
    return v / mask;
}
// split f16: k = (ky * 8 + kx) * cpix + c, pixel slot kx = 7 carries no tap
inline double tap_f16(const float *w, const float *b, int C, int o, int k) {
    const int cpix = layer1_cpix(C), ky = k / (8 * cpix), kx = (k / cpix) % 8, c = k % cpix;
    return kx < 7 ? layer1_weight(w, b, C, o, ky, kx, c, 0.0, 1.0) : 0.0;
}
// int8: k = ky * 32 + slot * 4 + c; ONE of the eight pixel slots of a kernel row carries no tap — slot 0 in the fused kernel (the
// fragment of output pixel j starts at input pixel 2 j - 4, 16-byte aligned quads), slot 7 in the layered kernels (the fragment starts
// at the window column of tap 0)
inline double tap_i8(const float *w, const float *b, int zero_slot, int o, int k) {
    const int ky = k / 32, slot = (k % 32) / 4, c = k % 4, kx = zero_slot == 0 ? slot - 1 : slot;
    return slot != zero_slot ? layer1_weight(w, b, 3, o, ky, kx, c, kOffsetI8, (double)kMaskI8) : 0.0;
}

// out: [n-half][k-step][lane][8 hi | 8 lo] f16, layer1_bytes(C) bytes; lane (h, n) of k-step s holds k = 16 s + 8 h .. + 7 of output
// channel 32 * half + n.  Returns the layer's pre-scale.
inline float pack_layer1_f16(const float *w, const float *b, int C, _Float16 *out) {
    const int ks = layer1_steps(C);
    double wmax = 0.0;
    for (int o = 0; o < 64; o++)
        for (int k = 0; k < 16 * ks; k++) wmax = fmax(wmax, fabs(tap_f16(w, b, C, o, k)));
    const float scale = pick_scale(wmax);
    for (int nh = 0; nh < 2; nh++)
        for (int s = 0; s < ks; s++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 8; e++) {
                    const int o = 32 * nh + (lane & 31), k = 16 * s + 8 * (lane >> 5) + e;
                    _Float16 *dst = out + ((size_t)(nh * ks + s) * 64 + lane) * 16;
                    split_f16((float)(tap_f16(w, b, C, o, k) * (double)scale), dst[e], dst[8 + e]);
                }
    return scale;
}
// out: [n-half][kernel row][digit][lane][16 i8], kPackI8Bytes bytes; inv256[o] = 256 / scale_o, scale_o = the largest power of two with
// max_k |w| scale_o <= kWeightTopI8: weight = (65536 d0 + 256 d1 + d2) / scale_o with balanced digits in [-128, 127].
inline void pack_layer1_i8(const float *w, const float *b, int zero_slot, int8_t *out, float *inv256) {
    for (int o = 0; o < 64; o++) {
        double wmax = 0.0;
        for (int k = 0; k < 32 * kI8Steps; k++) wmax = fmax(wmax, fabs(tap_i8(w, b, zero_slot, o, k)));
        const double scale = pow2_scale((double)kWeightTopI8, wmax, kScaleClampI8);
        inv256[o] = (float)(256.0 / scale);
        const int nh = o >> 5;
        for (int k = 0; k < 32 * kI8Steps; k++) {
            long long z = llround(tap_i8(w, b, zero_slot, o, k) * scale);
            if (z > kWeightTopI8) z = kWeightTopI8;
            if (z < -kWeightTopI8) z = -kWeightTopI8;
            int dg[kI8Digits];
            for (int d = kI8Digits - 1; d >= 0; d--) {          // least significant first
                long long r = ((z + 128) % 256 + 256) % 256 - 128;
                dg[d] = (int)r;
                z = (z - r) / 256;
            }
            const int s = k / 32, hh = (k % 32) / 16, el = k % 16, lane = hh * 32 + (o & 31);
            for (int d = 0; d < kI8Digits; d++)
                out[((size_t)((nh * kI8Steps + s) * kI8Digits + d) * 64 + lane) * 16 + el] = (int8_t)dg[d];
        }
    }
}
// conv_w [64][64][3][3] (torch OIHW, BatchNorm folded): k = (ky * 3 + kx) * 64 + c; out as pack_layer1_f16's, kPack3x3Bytes bytes
inline float pack_layer3x3(const float *w, _Float16 *out) {
    double wmax = 0.0;
    for (int i = 0; i < 64 * 64 * 9; i++) wmax = fmax(wmax, fabs((double)w[i]));
    const float scale = pick_scale(wmax);
    for (int nh = 0; nh < 2; nh++)
        for (int s = 0; s < kSteps3x3; s++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 8; e++) {
                    const int o = 32 * nh + (lane & 31), k = 16 * s + 8 * (lane >> 5) + e;
                    const int tap = k / 64, c = k % 64, ky = tap / 3, kx = tap % 3;
                    _Float16 *dst = out + ((size_t)(nh * kSteps3x3 + s) * 64 + lane) * 16;
                    split_f16(w[((o * 64 + c) * 3 + kx) * 3 + ky] * scale, dst[e], dst[8 + e]);
                }
    return scale;
}
// the fused kernel's image (kPackFusedBytes bytes at out): layer 1 for 3 channels, then layers 2 and 3; scales3 = their pre-scales
inline void pack_fused(const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv3_w, char *out, float *scales3) {
    scales3[0] = pack_layer1_f16(conv1_w, conv1_b, 3, reinterpret_cast<_Float16 *>(out));
    scales3[1] = pack_layer3x3(conv2_w, reinterpret_cast<_Float16 *>(out + layer1_bytes(3)));
    scales3[2] = pack_layer3x3(conv3_w, reinterpret_cast<_Float16 *>(out + layer1_bytes(3) + kPack3x3Bytes));
}
// The layered path's FC matrix: its features are [frame row p][frame column q][channel]; torch flattens the transposed map as
// (channel, q, p).  fc_w, out: [state_dim][64 * Hp * Wp]
inline void reorder_fc(const float *fc_w, int state_dim, int Hp, int Wp, float *out) {
    const size_t F = (size_t)64 * Hp * Wp;
    for (int s = 0; s < state_dim; s++)
        for (int p = 0; p < Hp; p++)
            for (int q = 0; q < Wp; q++)
                for (int c = 0; c < 64; c++) out[(size_t)s * F + (p * Wp + q) * 64 + c] = fc_w[(size_t)s * F + (size_t)c * Wp * Hp + q * Hp + p];
}

}  // namespace srlenc
