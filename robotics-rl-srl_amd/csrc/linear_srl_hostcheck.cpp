// linear_srl_hostcheck.cpp — srlhip_linear_srl_*'s arithmetic and rules (linear_srl.hpp, the text the kernels of linear_srl.hip call) as a
// stand-alone host program.  TESTS ONLY (make linearsrlhostcheck; tests/test_linear_srl_cpu.py).
//   linear_srl_hostcheck <case file> <result file>
//     case    int64 [5]   F S n C steps
//             float64     scale [C], offset [C], adam [4] (lr beta1 beta2 eps), bc [steps][2] (bc1 bc2 of every step)
//             float64     V [F][S], c [S], m [F][S], v [F][S], G [n][S]
//             uint8       frames [n][F]
//     result  float64     states [n][S] (forward, before any step), grad [F][S] (of the last step), V, m, v [F][S] after `steps` steps
//   linear_srl_hostcheck check       every buffer a heap block of its exact size (under the sanitizers a load that leaves the frames aborts):
//                                    ragged chunks, F no multiple of the lane count, n = 1, S = 1 and S = 64; prints "check ok"
//   linear_srl_hostcheck rules       one line per case of the shape, batch, table and Adam rules; then the launches' shape for a few (F, S, n)
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "hostcheck_io.hpp"
#include "linear_srl.hpp"

using namespace srl;

static void line(const char *what, long long a, long long b, long long c, const Verdict &v) {
    printf("%s %lld %lld %lld: %d %s\n", what, a, b, c, v.code, v.msg ? v.msg : "accepted");
}

static int print_rules() {
    for (int64_t F : {(int64_t)0, (int64_t)1, (int64_t)150528})
        for (int32_t S : {0, 1, 64, 65})
            for (int32_t C : {0, 1, 8, 9}) line("shape", (long long)F, S, C, check_lin_shape(F, S, C));
    for (int32_t n : {-1, 0, 1, 1024, 1025}) line("batch", n, 0, 0, check_lin_batch(n));
    const double ok[2] = {1.0, 2.0}, bad[2] = {1.0, INFINITY};
    line("tables", 0, 0, 0, check_lin_tables(ok, ok, 2));
    line("tables", 1, 0, 0, check_lin_tables(nullptr, ok, 2));
    line("tables", 2, 0, 0, check_lin_tables(ok, bad, 2));
    const LinAdam good{1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001};
    line("adam", 0, 0, 0, check_lin_adam(good));
    LinAdam a = good; a.lr = NAN; line("adam", 1, 0, 0, check_lin_adam(a));
    a = good; a.beta1 = 1.0; line("adam", 2, 0, 0, check_lin_adam(a));
    a = good; a.beta2 = -0.1; line("adam", 3, 0, 0, check_lin_adam(a));
    a = good; a.eps = -1.0; line("adam", 4, 0, 0, check_lin_adam(a));
    a = good; a.bc1 = 0.0; line("adam", 5, 0, 0, check_lin_adam(a));
    a = good; a.bc2 = 1.5; line("adam", 6, 0, 0, check_lin_adam(a));
    for (int64_t F : {(int64_t)1, (int64_t)193, (int64_t)513, (int64_t)12288, (int64_t)150528})
        for (int32_t S : {1, 5, 12, 32, 40, 64})
            for (int32_t n : {1, 257, 1024})
                printf("launch F %lld S %d n %d: chunks %lld SP %d tiles %lld workspace %zu group %d groups %d blocks %lld\n", (long long)F, S, n,
                       (long long)lin_chunks(F), lin_padded_dim(S), (long long)lin_tiles(n, lin_padded_dim(S)), lin_workspace_bytes(F, S, n),
                       lin_step_group(S), lin_step_groups(S), (long long)lin_step_blocks(F));
    return 0;
}

// exact-size heap blocks, one forward and two steps per shape
static int run_check() {
    struct Shape { int64_t F; int32_t S, n, C; };
    const Shape shapes[] = {{1, 1, 1, 3}, {511, 5, 2, 3}, {512, 64, 1, 6}, {513, 1, 3, 3}, {64 * 3 + 1, 64, 2, 3}, {1025, 7, 1, 8}, {130, 33, 257, 6}};
    uint64_t lcg = 12345;
    const auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 33); };
    for (const Shape &sh : shapes) {
        const size_t FS = (size_t)(sh.F * sh.S), nS = (size_t)sh.n * sh.S, nF = (size_t)(sh.n * sh.F);
        std::unique_ptr<uint8_t[]> frames(new uint8_t[nF]);
        std::unique_ptr<double[]> V(new double[FS]), m(new double[FS]), v(new double[FS]), grad(new double[FS]), c(new double[sh.S]), G(new double[nS]),
            states(new double[nS]), scale(new double[sh.C]), offset(new double[sh.C]);
        for (size_t k = 0; k < nF; k++) frames[k] = (uint8_t)next();
        for (size_t k = 0; k < FS; k++) { V[k] = (next() % 2001 - 1000.0) * 1e-4; m[k] = 0.0; v[k] = 0.0; }
        for (int32_t k = 0; k < sh.S; k++) c[k] = k * 0.25;
        for (size_t k = 0; k < nS; k++) G[k] = (next() % 2001 - 1000.0) * 1e-3;
        for (int32_t k = 0; k < sh.C; k++) { scale[k] = 1.0 / (255.0 * (0.2 + 0.01 * k)); offset[k] = (0.4 + 0.01 * k) / (0.2 + 0.01 * k); }
        if (check_lin_shape(sh.F, sh.S, sh.C).code || check_lin_batch(sh.n).code || check_lin_tables(scale.get(), offset.get(), sh.C).code) return 1;
        const LinNorm t = lin_norm(scale.get(), offset.get(), sh.C);
        lin_forward_host(frames.get(), sh.n, sh.F, sh.S, t, V.get(), c.get(), states.get());
        double b1 = 1.0, b2 = 1.0;
        for (int step = 0; step < 2; step++) {
            b1 *= 0.9; b2 *= 0.999;
            const LinAdam adam{1e-3, 0.9, 0.999, 1e-8, 1.0 - b1, 1.0 - b2};
            if (check_lin_adam(adam).code) return 1;
            lin_step_host(frames.get(), sh.n, sh.F, sh.S, t, G.get(), V.get(), m.get(), v.get(), adam, step ? grad.get() : nullptr);
        }
        // the first feature's gradient of column 0, restated here
        double g = 0.0;
        for (int32_t i = 0; i < sh.n; i++) g = fma(fma(scale[0], (double)frames[(size_t)i * sh.F], -offset[0]), G[(size_t)i * sh.S], g);
        if (g != grad[0] || !(states[0] == states[0]) || !(V[FS - 1] == V[FS - 1])) { fprintf(stderr, "check failed at F %lld\n", (long long)sh.F); return 1; }
    }
    printf("check ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "rules")) return print_rules();
    if (argc == 2 && !strcmp(argv[1], "check")) return run_check();
    if (argc != 3) { fprintf(stderr, "usage: linear_srl_hostcheck <case> <result> | check | rules\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int64_t> hd;
    std::vector<double> scale, offset, ad, bc, V, c, m, v, G;
    std::vector<uint8_t> frames;
    if (!rd(f, hd, 5)) { fprintf(stderr, "short header\n"); fclose(f); return 2; }
    const int64_t F = hd[0], S = hd[1], n = hd[2], C = hd[3], steps = hd[4];
    if (F > (int64_t)1 << 28 || S > kLinMaxDim || C > kLinMaxChannels || check_lin_shape(F, (int32_t)S, (int32_t)C).code || n > kLinMaxFrames ||
        check_lin_batch((int32_t)n).code || steps < 0 || steps > 64) {
        fprintf(stderr, "bad shape\n"); fclose(f); return 2;
    }
    const size_t FS = (size_t)(F * S);
    const bool ok = rd(f, scale, (size_t)C) && rd(f, offset, (size_t)C) && rd(f, ad, 4) && rd(f, bc, (size_t)(2 * steps)) && rd(f, V, FS) && rd(f, c, (size_t)S) && rd(f, m, FS) &&
                    rd(f, v, FS) && rd(f, G, (size_t)(n * S)) && rd(f, frames, (size_t)(n * F));
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    if (check_lin_tables(scale.data(), offset.data(), (int32_t)C).code) { fprintf(stderr, "bad tables\n"); return 2; }
    const LinNorm t = lin_norm(scale.data(), offset.data(), (int32_t)C);
    std::vector<double> states((size_t)(n * S)), grad(FS, 0.0);
    lin_forward_host(frames.data(), (int32_t)n, F, (int32_t)S, t, V.data(), c.data(), states.data());
    for (int64_t step = 0; step < steps; step++) {
        const LinAdam adam{ad[0], ad[1], ad[2], ad[3], bc[2 * step], bc[2 * step + 1]};
        if (check_lin_adam(adam).code) { fprintf(stderr, "bad adam\n"); return 2; }
        lin_step_host(frames.data(), (int32_t)n, F, (int32_t)S, t, G.data(), V.data(), m.data(), v.data(), adam, grad.data());
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool wrote = wr(f, states) && wr(f, grad) && wr(f, V) && wr(f, m) && wr(f, v);
    return fclose(f) == 0 && wrote ? 0 : 2;
}
