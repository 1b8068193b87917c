// policy_hostcheck.cpp — srlhip_policy_act's per-env arithmetic (policy_act.hpp, the text the kernels of policy_act.hip call) as a
// stand-alone host program: `policy_hostcheck <case file> <result file>`.  TESTS ONLY (make policyhostcheck; tests/test_policy_act_cpu.py
// writes the case, reads the result and compares it with tests/policy_act_ref.py bit for bit).
//   case    int32 [12]  N D H A per_env normalize freeze discrete sample none_nan has_done_prev 0     (H = 0: the linear policy)
//           float64     clip
//           float32     obs [N][D]
//           float64 [(N)][D][A] (linear) | float32 [(N)][P] (MLP): the parameters, per env with per_env
//           float64     mean [D], std [D]
//           uint8       done_prev [N], frozen [N]
//           float64     u [N]: the uniform draw of every env (sample)
//   result  float64 score [N][A], float64 w [N][A] (the softmax weights; zeros without sample), int32 [N] | float32 [N][A] the action rows,
//           uint8 frozen [N]
#include <stdlib.h>

#include "hostcheck_io.hpp"
#include "policy_act.hpp"

using namespace srl;

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: policy_hostcheck <case> <result>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd;
    std::vector<double> clipv, wd, mean, sd, u;
    std::vector<float> obs, wf;
    std::vector<uint8_t> done_prev, frozen;
    if (!rd(f, hd, 12) || !rd(f, clipv, 1)) { fprintf(stderr, "short header\n"); return 2; }
    const int N = hd[0], D = hd[1], H = hd[2], A = hd[3];
    const bool per_env = hd[4], normalize = hd[5], freeze = hd[6], discrete = hd[7], sample = hd[8], none_nan = hd[9], has_done = hd[10];
    if (N < 1 || D < 1 || D > kActMaxDim || H < 0 || H > kActMaxHidden || A < 1 || A > kActMaxOut) { fprintf(stderr, "bad shape\n"); return 2; }
    const size_t P = H ? (size_t)H * D + H + (size_t)A * H + A : (size_t)D * A, blocks = per_env ? N : 1;
    bool ok = rd(f, obs, (size_t)N * D) && (H ? rd(f, wf, blocks * P) : rd(f, wd, blocks * P)) && rd(f, mean, D) && rd(f, sd, D) &&
              rd(f, done_prev, N) && rd(f, frozen, N) && rd(f, u, N);
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    const double clip = clipv[0];

    std::vector<double> score((size_t)N * A), wout((size_t)N * A, 0.0);
    std::vector<int32_t> act_i(discrete ? N : 0);
    std::vector<float> act_f(discrete ? 0 : (size_t)N * A);
    std::vector<float> x(D);
    std::vector<double> h(H ? H : 1);
    const ActFinish fin{has_done ? done_prev.data() : nullptr, frozen.data(), discrete ? static_cast<void *>(act_i.data()) : static_cast<void *>(act_f.data()),
                        A, freeze, discrete, sample, none_nan};
    for (int e = 0; e < N; e++) {
        for (int d = 0; d < D; d++) x[d] = act_input(obs[(size_t)e * D + d], normalize, normalize ? mean[d] : 0.0, normalize ? sd[d] : 1.0, clip);
        double s[kActMaxOut];
        if (!H) {
            const double *W = wd.data() + (per_env ? (size_t)e * P : 0);
            for (int a = 0; a < A; a++) {
                double acc = 0.0;
                for (int d = 0; d < D; d++) acc = act_linear_step(d == 0, acc, x[d], W[(size_t)d * A + a]);
                s[a] = acc;
            }
        } else {
            const float *w = wf.data() + (per_env ? (size_t)e * P : 0);
            const float *b1 = w + (size_t)H * D, *w2 = b1 + H, *b2 = w2 + (size_t)A * H;
            for (int j = 0; j < H; j++) {
                double acc = (double)b1[j];
                for (int d = 0; d < D; d++) acc = act_hidden_step(acc, w[(size_t)j * D + d], x[d]);
                h[j] = act_relu(acc);
            }
            for (int a = 0; a < A; a++) {
                double part[kActLanes];
                for (int l = 0; l < kActLanes; l++) part[l] = act_lane_partial(l, H, w2 + (size_t)a * H, b2[a], h.data());
                s[a] = act_row_sum16(part);
            }
        }
        act_finish(fin, e, s, score.data(), u[e], &wout[(size_t)e * A]);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = wr(f, score) && wr(f, wout) && wr(f, act_i) && wr(f, act_f) && wr(f, frozen);
    return fclose(f) == 0 && ok ? 0 : 2;
}
