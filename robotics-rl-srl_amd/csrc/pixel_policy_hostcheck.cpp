// pixel_policy_hostcheck.cpp — srlhip_pixel_policy_act's per-env arithmetic (pixel_policy.hpp, the text the kernel of pixel_policy.hip
// calls) and its rules (api_rules.hpp) as a stand-alone host program.  TESTS ONLY (make pixelpolicyhostcheck; tests/test_pixel_policy_cpu.py).
//   pixel_policy_hostcheck <case file> <result file>
//     case    int32 [12]  N C H W A paired freeze discrete none_nan has_done_prev 0 0
//             float64     noise
//             uint8       frames [N][H][W][C]
//             float64     M [D][A], then with paired delta [N / 2][D][A]
//             uint8       done_prev [N], frozen [N]
//     result  float64 score [N][A], int32 [N] | float32 [N][A] the action rows, uint8 frozen [N]
//   pixel_policy_hostcheck shapes      one line per frame shape: D, the chunks, and for which populations a launch is split over them
//   pixel_policy_hostcheck refusals    one line per argument case: the code and the message of the checks
// The virtual lanes of a chunk are walked one after the other, their partials combined by pix_tree_sum — the kernel's levels in LDS.
#include <stdlib.h>
#include <string.h>

#include "hostcheck_io.hpp"
#include "pixel_policy.hpp"
#include "policy_act.hpp"

using namespace srl;

// one env's scores: sign +1 / -1 the env's side of its direction, 0 unpaired (delta is not read)
static void forward(const uint8_t *x, const double *M, const double *delta, double noise, int sign, int64_t D, int A, double *score) {
    std::vector<double> part(kPixLanes);
    for (int a = 0; a < A; a++) {
        double s = 0.0;
        for (int c = 0; c < pix_chunks(D); c++) {
            for (int v = 0; v < kPixLanes; v++) {
                double acc = 0.0;
                for (int j = 0; j < kPixSteps; j++) {
                    const int64_t d = (int64_t)c * kPixChunk + v + (int64_t)j * kPixLanes;
                    if (d >= D) break;
                    double w = M[d * A + a];
                    if (sign) {
                        double wp, wm;
                        pix_weights(w, delta[d * A + a], noise, &wp, &wm);
                        w = sign > 0 ? wp : wm;
                    }
                    acc = pix_step(acc, x[d], w);
                }
                part[v] = acc;
            }
            s = pix_chunk_join(c == 0, s, pix_tree_sum(part.data(), 1, 0));
        }
        score[a] = s;
    }
}

static int print_shapes() {
    const int sides[] = {7, 8, 9, 11, 16, 26, 27, 45, 51, 64, 224, 1024, 1025};
    for (int H : sides)
        for (int form = 0; form < 2; form++) {
            const int W = form ? sides[(H * 7) % 13] : H, C = form ? 6 : 3;
            srlhip_config c;
            fill_default_config(SRLHIP_ENV_MOBILE, &c);
            c.img_h = H; c.img_w = W; c.multi_view = form;
            const int64_t D = (int64_t)frame_bytes(c);
            const int nc = pix_chunks(D);
            printf("shape %d %d %d ok %d D %lld chunks %d split", C, H, W, check_config(c).code == 0 ? 1 : 0, (long long)D, nc);
            for (int items : {1, 10, 255, 256, 2048}) printf(" %d", pix_split(items, nc) ? 1 : 0);
            printf("\n");
        }
    return 0;
}

static int print_refusals() {
    srlhip_pixel_policy pol;
    double dummy = 0.0;
    const auto fresh = [&]() { memset(&pol, 0, sizeof pol); pol.struct_size = (int32_t)sizeof pol; pol.weights = &dummy; };
    verdict("null policy", check_pixel_policy_abi(nullptr));
    fresh(); pol.struct_size -= 4; verdict("struct_size", check_pixel_policy_abi(&pol));
    fresh(); pol.reserved = 1; verdict("reserved", check_pixel_policy_abi(&pol));
    fresh(); pol.weights = nullptr; verdict("null weights", check_pixel_policy_abi(&pol));
    fresh(); pol.paired = 1; verdict("paired without delta", check_pixel_policy_abi(&pol));
    fresh(); pol.delta = &dummy; verdict("delta without paired", check_pixel_policy_abi(&pol));
    fresh(); verdict("policy", check_pixel_policy_abi(&pol));
    fresh(); pol.paired = 1; pol.delta = &dummy; verdict("paired policy", check_pixel_policy_abi(&pol));
    srlhip_config c;
    const auto base = [&]() { fill_default_config(SRLHIP_ENV_KUKA_BUTTON, &c); c.io_device = 1; c.obs_mode = SRLHIP_OBS_RAW_PIXELS; c.img_h = c.img_w = 8; c.num_envs = 4; };
    base(); verdict("planes", check_pixel_policy_act(c, true, true, true, true, true));
    base(); verdict("null images", check_pixel_policy_act(c, false, false, false, true, false));
    base(); verdict("null act_out", check_pixel_policy_act(c, false, false, true, false, false));
    base(); c.num_envs = 5; verdict("paired odd num_envs", check_pixel_policy_act(c, true, false, true, true, false));
    base(); c.num_envs = 5; verdict("unpaired odd num_envs", check_pixel_policy_act(c, false, false, true, true, false));
    base(); verdict("freeze without frozen", check_pixel_policy_act(c, false, true, true, true, false));
    base(); c.io_device = 0; verdict("host-pointer handle", check_pixel_policy_act(c, false, false, true, true, false));
    base(); c.obs_mode = SRLHIP_OBS_GROUND_TRUTH; verdict("ground_truth", check_pixel_policy_act(c, false, false, true, true, false));
    base(); c.img_h = 1024; c.img_w = 1024; c.multi_view = 1; verdict("1024 x 1024 x 6", check_pixel_policy_act(c, true, false, true, true, false));
    base(); c.is_discrete = 0; verdict("continuous", check_pixel_policy_act(c, false, false, true, true, false));
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "shapes")) return print_shapes();
    if (argc == 2 && !strcmp(argv[1], "refusals")) return print_refusals();
    if (argc != 3) { fprintf(stderr, "usage: pixel_policy_hostcheck <case> <result> | shapes | refusals\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd;
    std::vector<uint8_t> frames, done_prev, frozen;
    std::vector<double> nu, M, delta;
    if (!rd(f, hd, 12)) { fprintf(stderr, "short header\n"); return 2; }
    const int N = hd[0], C = hd[1], H = hd[2], W = hd[3], A = hd[4];
    const bool paired = hd[5], freeze = hd[6], discrete = hd[7], none_nan = hd[8], has_done = hd[9];
    if (N < 1 || (C != 3 && C != 6) || H < 8 || W < 8 || H > 1024 || W > 1024 || A < 1 || A > kPixMaxOut || (paired && N % 2)) { fprintf(stderr, "bad shape\n"); return 2; }
    const int64_t D = (int64_t)H * W * C;
    bool ok = rd(f, nu, 1) && rd(f, frames, (size_t)N * D) && rd(f, M, (size_t)D * A) && rd(f, delta, paired ? (size_t)(N / 2) * D * A : 0) &&
              rd(f, done_prev, N) && rd(f, frozen, N);
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }

    std::vector<double> score((size_t)N * A);
    std::vector<int32_t> act_i(discrete ? N : 0);
    std::vector<float> act_f(discrete ? 0 : (size_t)N * A);
    const ActFinish fin{has_done ? done_prev.data() : nullptr, frozen.data(), discrete ? static_cast<void *>(act_i.data()) : static_cast<void *>(act_f.data()),
                        A, freeze, discrete, 0, none_nan};
    for (int e = 0; e < N; e++) {
        double sd[kPixMaxOut];
        forward(frames.data() + (size_t)e * D, M.data(), paired ? delta.data() + (size_t)(e / 2) * D * A : nullptr, nu[0], paired ? (e % 2 ? -1 : 1) : 0, D, A, sd);
        act_finish(fin, e, sd, score.data(), 0.0);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = wr(f, score) && wr(f, act_i) && wr(f, act_f) && wr(f, frozen);
    return fclose(f) == 0 && ok ? 0 : 2;
}
