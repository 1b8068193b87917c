// cnn_policy_hostcheck.cpp — srlhip_cnn_policy_act's per-env arithmetic (cnn_policy.hpp, the text the kernel of cnn_policy.hip calls) and
// its rules (api_rules.hpp) as a stand-alone host program.  TESTS ONLY (make cnnpolicyhostcheck; tests/test_cnn_policy_cpu.py).
//   cnn_policy_hostcheck <case file> <result file>
//     case    int32 [12]  N C H W A per_env freeze discrete sample none_nan has_done_prev 0
//             uint8       frames [N][H][W][C]
//             float32     params [(N)][P], per env with per_env
//             uint8       done_prev [N], frozen [N]
//             float64     u [N]: the uniform draw of every env (sample)
//     result  float32 score [N][A], float64 w [N][A] (the softmax weights; zeros without sample), int32 [N] | float32 [N][A] the action
//             rows, uint8 frozen [N]
//   cnn_policy_hostcheck shapes      one line per frame shape: the conv and pooled planes, F and P
//   cnn_policy_hostcheck refusals    one line per argument case: the code and the message of the checks
// The workgroup's threads are walked one after the other: thread u of group g takes the cells u, u + TG, ..., its partial sums are
// combined by cnn_tree_sum over the TG threads — the kernel's butterfly, in thread order.
#include <stdlib.h>
#include <string.h>

#include "cnn_policy.hpp"
#include "hostcheck_io.hpp"
#include "policy_act.hpp"

using namespace srl;

template <int K, int PAD, int CO, int CG, class In>
static void layer(const In &in, int Cin, int hc, int wc, const float *w, const float *gamma, const float *beta, std::vector<float> &pooled) {
    constexpr int G = CO / CG, TG = kCnnBlock / G;
    const int hcell = (hc + 1) / 2, wcell = (wc + 1) / 2, hp = hc / 2, wp = wc / 2;
    std::vector<float> wt((size_t)CO * Cin * K * K);
    for (int i = 0; i < CO * Cin * K * K; i++) wt[cnn_weight_slot(i, Cin, K * K, CO)] = w[i];
    pooled.assign((size_t)CO * hp * wp, 0.f);
    std::vector<double> S((size_t)CO * TG, 0.0), Q((size_t)CO * TG, 0.0);      // [channel][thread of its group]
    for (int g = 0; g < G; g++)
        for (int u = 0; u < TG; u++) {
            double s[CG], q[CG];
            for (int k = 0; k < CG; k++) s[k] = q[k] = 0.0;
            for (int cell = u; cell < hcell * wcell; cell += TG) {
                float acc[CG][4];
                cnn_cell<K, PAD, CG>(in, Cin, CO, g * CG, wt.data(), cell / wcell, cell % wcell, acc);
                cnn_cell_finish<CG>(acc, cell / wcell, cell % wcell, hc, wc, g * CG, gamma, s, q, pooled.data());
            }
            for (int k = 0; k < CG; k++) { S[(size_t)(g * CG + k) * TG + u] = s[k]; Q[(size_t)(g * CG + k) * TG + u] = q[k]; }
        }
    for (int c = 0; c < CO; c++) {
        double mean, gs;
        cnn_channel_stats(cnn_tree_sum(&S[(size_t)c * TG], TG), cnn_tree_sum(&Q[(size_t)c * TG], TG), hc * wc, gamma[c], &mean, &gs);
        for (int i = 0; i < hp * wp; i++) pooled[(size_t)c * hp * wp + i] = cnn_normalise(pooled[(size_t)c * hp * wp + i], mean, gs, beta[c]);
    }
}

static void forward(const CnnShape &s, const CnnParamLayout &L, const float *P, const uint8_t *img, int A, float *score) {
    std::vector<float> p1, p2, p3;
    const int H = s.H, W = s.W, C = s.C;
    const auto frame = [=](int ci, int r, int c) { return (r >= 0 && r < H && c >= 0 && c < W) ? cnn_input(img[((size_t)r * W + c) * C + ci]) : 0.f; };
    layer<5, 2, kCnnCh1, kCnnCg1>(frame, C, s.hc[0], s.wc[0], P + L.w1, P + L.g1, P + L.b1, p1);
    const float *q1 = p1.data();
    const int h1 = s.hp[0], w1 = s.wp[0];
    const auto plane1 = [=](int ci, int r, int c) { return (r >= 0 && r < h1 && c >= 0 && c < w1) ? q1[(ci * h1 + r) * w1 + c] : 0.f; };
    layer<3, 1, kCnnCh2, kCnnCg2>(plane1, kCnnCh1, s.hc[1], s.wc[1], P + L.w2, P + L.g2, P + L.b2, p2);
    const float *q2 = p2.data();
    const int h2 = s.hp[1], w2 = s.wp[1];
    const auto plane2 = [=](int ci, int r, int c) { return (r >= 0 && r < h2 && c >= 0 && c < w2) ? q2[(ci * h2 + r) * w2 + c] : 0.f; };
    layer<3, 1, kCnnCh3, kCnnCg3>(plane2, kCnnCh2, s.hc[2], s.wc[2], P + L.w3, P + L.g3, P + L.b3, p3);
    for (int a = 0; a < A; a++) score[a] = cnn_fc(P + L.fcw + (size_t)a * s.F, P[L.fcb + a], p3.data(), s.F);
}

static int print_shapes() {
    for (int H = kCnnMinSide - 3; H <= kCnnMaxSide + 2; H++)
        for (int form = 0; form < 2; form++) {
            const int W = form ? kCnnMinSide + kCnnMaxSide - (H < kCnnMinSide ? kCnnMinSide : H > kCnnMaxSide ? kCnnMaxSide : H) : H, C = form ? 6 : 3, A = form ? 3 : 6;
            const CnnShape s = cnn_shape(C, H, W);
            printf("shape %d %d %d %d ok %d planes", C, H, W, A, cnn_side_ok(H) && cnn_side_ok(W) ? 1 : 0);
            for (int l = 0; l < 3; l++) printf(" %d %d %d %d", s.hc[l], s.wc[l], s.hp[l], s.wp[l]);
            printf(" F %d P %zu\n", s.F, cnn_param_count(C, H, W, A));
        }
    return 0;
}

static int print_refusals() {
    srlhip_cnn_policy pol;
    float dummy = 0.f;
    const auto fresh = [&]() { memset(&pol, 0, sizeof pol); pol.struct_size = (int32_t)sizeof pol; pol.params = &dummy; };
    verdict("null policy", check_cnn_policy_abi(nullptr));
    fresh(); pol.struct_size -= 4; verdict("struct_size", check_cnn_policy_abi(&pol));
    fresh(); pol.reserved = 1; verdict("reserved", check_cnn_policy_abi(&pol));
    fresh(); pol.params = nullptr; verdict("null params", check_cnn_policy_abi(&pol));
    fresh(); verdict("policy", check_cnn_policy_abi(&pol));
    srlhip_config c;
    const auto base = [&]() { fill_default_config(SRLHIP_ENV_KUKA_BUTTON, &c); c.io_device = 1; c.obs_mode = SRLHIP_OBS_RAW_PIXELS; c.img_h = c.img_w = 64; };
    base(); verdict("planes", check_cnn_policy_act(c, true, true, true, true, true));
    base(); verdict("null images", check_cnn_policy_act(c, false, false, false, true, false));
    base(); verdict("null act_out", check_cnn_policy_act(c, false, false, true, false, false));
    base(); verdict("freeze without frozen", check_cnn_policy_act(c, true, false, true, true, false));
    base(); c.io_device = 0; verdict("host-pointer handle", check_cnn_policy_act(c, false, false, true, true, false));
    base(); c.obs_mode = SRLHIP_OBS_GROUND_TRUTH; verdict("ground_truth", check_cnn_policy_act(c, false, false, true, true, false));
    base(); c.img_h = 42; verdict("img_h 42", check_cnn_policy_act(c, false, false, true, true, false));
    base(); c.img_h = 43; c.img_w = 224; verdict("43 x 224", check_cnn_policy_act(c, false, false, true, true, false));
    base(); c.img_w = 225; verdict("img_w 225", check_cnn_policy_act(c, false, false, true, true, false));
    base(); c.is_discrete = 0; verdict("sample continuous", check_cnn_policy_act(c, false, true, true, true, false));
    base(); c.is_discrete = 0; verdict("continuous", check_cnn_policy_act(c, false, false, true, true, false));
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "shapes")) return print_shapes();
    if (argc == 2 && !strcmp(argv[1], "refusals")) return print_refusals();
    if (argc != 3) { fprintf(stderr, "usage: cnn_policy_hostcheck <case> <result> | shapes | refusals\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd;
    std::vector<uint8_t> frames, done_prev, frozen;
    std::vector<float> params;
    std::vector<double> u;
    if (!rd(f, hd, 12)) { fprintf(stderr, "short header\n"); return 2; }
    const int N = hd[0], C = hd[1], H = hd[2], W = hd[3], A = hd[4];
    const bool per_env = hd[5], freeze = hd[6], discrete = hd[7], sample = hd[8], none_nan = hd[9], has_done = hd[10];
    if (N < 1 || (C != 3 && C != 6) || !cnn_side_ok(H) || !cnn_side_ok(W) || A < 1 || A > kActMaxOut) { fprintf(stderr, "bad shape\n"); return 2; }
    const CnnShape s = cnn_shape(C, H, W);
    const CnnParamLayout L = cnn_param_layout(C, H, W, A);
    const size_t fb = (size_t)H * W * C;
    bool ok = rd(f, frames, (size_t)N * fb) && rd(f, params, (per_env ? (size_t)N : 1) * L.total) && rd(f, done_prev, N) && rd(f, frozen, N) && rd(f, u, N);
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }

    std::vector<float> score((size_t)N * A);
    std::vector<double> wout((size_t)N * A, 0.0);
    std::vector<int32_t> act_i(discrete ? N : 0);
    std::vector<float> act_f(discrete ? 0 : (size_t)N * A);
    const ActFinish fin{has_done ? done_prev.data() : nullptr, frozen.data(), discrete ? static_cast<void *>(act_i.data()) : static_cast<void *>(act_f.data()),
                        A, freeze, discrete, sample, none_nan};
    for (int e = 0; e < N; e++) {
        float sf[kActMaxOut];
        forward(s, L, params.data() + (per_env ? (size_t)e * L.total : 0), frames.data() + (size_t)e * fb, A, sf);
        double sd[kActMaxOut];
        for (int k = 0; k < A; k++) sd[k] = (double)sf[k];
        act_finish(fin, e, sd, score.data(), u[e], &wout[(size_t)e * A]);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = wr(f, score) && wr(f, wout) && wr(f, act_i) && wr(f, act_f) && wr(f, frozen);
    return fclose(f) == 0 && ok ? 0 : 2;
}
