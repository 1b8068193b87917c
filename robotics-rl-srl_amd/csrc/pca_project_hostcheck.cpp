// pca_project_hostcheck.cpp — srlhip_pca_*'s arithmetic and rules (pca_project.hpp, the text the kernel of pca_project.hip calls) as a
// stand-alone host program.  TESTS ONLY (make pcahostcheck; tests/test_pca_cpu.py).
//   pca_project_hostcheck <case file> <result file>
//     case    int64 [4]   F S n states_f32
//             float64     w [F][S], b [S]
//             uint8       frames [n][F]
//     result  float64 [n][S] | float32 [n][S] the states
//   pca_project_hostcheck rules      one line per case of the shape and argument rules: the code and the message; then the launch's shape
//                                    (chunks, padded S, frames of a tile, tiles, tiles of one launch) for a few (F, S, n)
#include <stdlib.h>
#include <string.h>

#include "hostcheck_io.hpp"
#include "pca_project.hpp"

using namespace srl;

static void verdict(const char *what, long long a, long long b, const Verdict &v) { printf("%s %lld %lld: %d %s\n", what, a, b, v.code, v.msg ? v.msg : "accepted"); }

static int print_rules() {
    const int64_t Fs[] = {0, 1, 12288, 301056};
    const int32_t Ss[] = {0, 1, 64, 65};
    for (int64_t F : Fs)
        for (int32_t S : Ss) verdict("shape", (long long)F, S, check_pca_shape(F, S));
    verdict("forward n images", -1, 1, check_pca_forward(-1, true, true, 0));
    verdict("forward n images", 0, 0, check_pca_forward(0, false, false, 0));
    verdict("forward n images", 3, 0, check_pca_forward(3, false, true, 0));
    verdict("forward n states", 3, 0, check_pca_forward(3, true, false, 1));
    verdict("forward n f32", 3, 2, check_pca_forward(3, true, true, 2));
    verdict("forward n f32", 3, 1, check_pca_forward(3, true, true, 1));
    for (int64_t F : {(int64_t)1, (int64_t)192, (int64_t)512, (int64_t)513, (int64_t)720, (int64_t)12288, (int64_t)150528})
        for (int32_t S : {1, 5, 9, 32, 33, 64})
            for (int64_t n : {(int64_t)1, (int64_t)130, (int64_t)4096, (int64_t)600000}) {
                const int SP = pca_padded_dim(S);
                const int64_t nc = pca_chunks(F), tiles = pca_tiles(n, SP);
                printf("launch F %lld S %d n %lld: chunks %lld SP %d tile %d tiles %lld slab %lld\n", (long long)F, S, (long long)n, (long long)nc, SP,
                       SP == 8 ? pca_tile_frames(8) : SP == 16 ? pca_tile_frames(16) : SP == 32 ? pca_tile_frames(32) : pca_tile_frames(64), (long long)tiles,
                       (long long)pca_slab_tiles(tiles, nc, SP));
            }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "rules")) return print_rules();
    if (argc != 3) { fprintf(stderr, "usage: pca_project_hostcheck <case> <result> | rules\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int64_t> hd;
    std::vector<double> w, b;
    std::vector<uint8_t> frames;
    if (!rd(f, hd, 4)) { fprintf(stderr, "short header\n"); fclose(f); return 2; }
    const int64_t F = hd[0], S = hd[1], n = hd[2];
    const bool f32 = hd[3] != 0;
    if (check_pca_shape(F, (int32_t)S).code || S > kPcaMaxDim || n < 0 || n > (1 << 20) || F > (int64_t)1 << 28) { fprintf(stderr, "bad shape\n"); fclose(f); return 2; }
    const bool ok = rd(f, w, (size_t)(F * S)) && rd(f, b, (size_t)S) && rd(f, frames, (size_t)(n * F));
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    std::vector<uint8_t> out((size_t)(n * S) * (f32 ? sizeof(float) : sizeof(double)));
    pca_project_host(F, (int32_t)S, w.data(), b.data(), frames.data(), (int32_t)n, out.data(), f32);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool wrote = wr(f, out);
    return fclose(f) == 0 && wrote ? 0 : 2;
}
