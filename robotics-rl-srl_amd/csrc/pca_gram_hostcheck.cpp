// pca_gram_hostcheck.cpp — srlhip_pca_gram's arithmetic, rules and index math (pca_gram.hpp, the text the kernels of pca_gram.hip call) as
// a stand-alone host program.  TESTS ONLY (make pcagramhostcheck; tests/test_pca_gram_cpu.py).
//   pca_gram_hostcheck <case file> <result file>
//     case    int64 [2]   N F
//             uint8       frames [N][F]
//     result  int64 [N][N] gram, int64 [N] rowsum          (the host twin)
//   pca_gram_hostcheck check       proves, and prints one line per item ("ok ..." / "FAIL ..."; exit status 1 on any FAIL):
//     shift     x y = s t + 128 (x + y) - 16384 for all 65536 byte pairs through gram_signed_word; a masked byte is a signed 0
//     chunk     the extreme sums of kGramChunk features fit an int32, of one feature more may not
//     supported pca_gram_supported at the edges of N and, by 128-bit arithmetic, of F
//     tiles     gram_tile_of meets every pair ti <= tj exactly once
//     cover     for a table of (N, F, split) — every shape of tests/test_gpu_pca_gram.py among them — the loads of each tile operand over
//               all slices, steps and lanes take every real byte of its rows exactly once and never leave [0, N F)
//     twin      pca_gram_host against a triple loop, and the kernel's signed route (chunks, slices, unshift) against the twin
#include <stdlib.h>
#include <string.h>

#include "hostcheck_io.hpp"
#include "pca_gram.hpp"

using namespace srl;

static int g_fail = 0;
static void item(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0) {
    printf("%s %s %lld %lld %lld\n", ok ? "ok" : "FAIL", what, a, b, c);
    if (!ok) g_fail = 1;
}

static void check_shift() {
    bool ok = true;
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) {
            const int s = (int8_t)gram_signed_word((uint32_t)x, 1), t = (int8_t)gram_signed_word((uint32_t)y, 1);
            ok = ok && s == x - 128 && t == y - 128 && (int64_t)x * y == gram_unshift((int64_t)s * t, x, y, 1);
        }
    item(ok, "shift identity over all byte pairs");
    ok = true;
    for (int valid = -3; valid <= 6; valid++) {
        const uint32_t w = gram_signed_word(0x00ff7f80u, valid);
        for (int q = 0; q < 4; q++) {
            const int got = (int8_t)(w >> (8 * q)), want = q < valid ? (int)((0x00ff7f80u >> (8 * q)) & 0xffu) - 128 : 0;
            ok = ok && got == want;
        }
    }
    item(ok, "padding is a signed 0 after the xor");
}

static void check_chunk() {
    // s, t in [-128, 127]: the extreme products are (-128)(-128) = 16384 and (-128)(127) = -16256
    const int64_t top = kGramChunk * 16384, bottom = kGramChunk * -16256;
    item(top == gram_chunk_bound(kGramChunk) && top <= INT32_MAX && bottom >= INT32_MIN, "a chunk's extreme sums fit an int32", top, bottom);
    item((kGramChunk * 2) * 16384 > INT32_MAX, "two chunks' do not", (kGramChunk * 2) * 16384);
    item(kGramChunkSteps * kGramStep == kGramChunk, "a chunk is whole steps", kGramChunkSteps);
}

static void check_supported() {
    bool ok = !pca_gram_supported(0, 1) && pca_gram_supported(1, 1) && pca_gram_supported(kGramMaxFrames, 1) && !pca_gram_supported(kGramMaxFrames + 1, 1) &&
              !pca_gram_supported(1, 0) && !pca_gram_supported(-1, 5) && pca_gram_supported(8192, 150528) && pca_gram_supported(33, 150528);
    item(ok, "supported at the edges of N");
    ok = true;
    for (int64_t N : {(int64_t)1, (int64_t)2, (int64_t)33, (int64_t)4096, (int64_t)8192}) {
        const int64_t most = (((int64_t)1 << 62) - 1) / (N * N * 65025);
        for (int64_t F : {most - 1, most, most + 1, most + 2}) {
            const unsigned __int128 v = (unsigned __int128)2 * (unsigned __int128)(N * N) * (unsigned __int128)F * 65025u;
            ok = ok && pca_gram_supported(N, F) == (v < ((unsigned __int128)1 << 63));
        }
    }
    item(ok, "supported at the edge of F by 128-bit arithmetic");
    ok = check_pca_gram(0, 4, 0, true, true, true).code == SRLHIP_ENOTSUP && check_pca_gram(8193, 4, 0, true, true, true).code == SRLHIP_ENOTSUP &&
         check_pca_gram(4, 0, 0, true, true, true).code == SRLHIP_ENOTSUP && check_pca_gram(4, 4, -1, true, true, true).code == SRLHIP_EINVAL &&
         check_pca_gram(4, 4, 0, false, true, true).code == SRLHIP_EINVAL && check_pca_gram(4, 4, 0, true, false, true).code == SRLHIP_EINVAL &&
         check_pca_gram(4, 4, 0, true, true, false).code == SRLHIP_EINVAL && check_pca_gram(4, 4, 7, true, true, true).code == 0;
    item(ok, "refusals by code");
}

static void check_tiles() {
    bool ok = true;
    for (int64_t N : {(int64_t)1, (int64_t)32, (int64_t)33, (int64_t)200, (int64_t)8192}) {
        const int64_t side = gram_tiles_side(N), upper = gram_tiles_upper(N);
        std::vector<uint8_t> seen((size_t)(side * side), 0);
        for (int64_t t = 0; t < upper; t++) {
            int ti, tj;
            gram_tile_of(t, side, &ti, &tj);
            ok = ok && ti >= 0 && ti <= tj && tj < side;
            if (ok) seen[(size_t)(ti * side + tj)]++;
        }
        for (int64_t i = 0; i < side && ok; i++)
            for (int64_t j = 0; j < side; j++) ok = ok && seen[(size_t)(i * side + j)] == (j >= i ? 1 : 0);
    }
    item(ok, "every tile of the upper triangle exactly once");
}

// the loads of tile operand `tb` (frames tb 32 .. tb 32 + 31) over every slice, step and lane, as the kernel makes them
static bool cover(int64_t N, int64_t F, int64_t split) {
    const int64_t per = gram_slice_steps(F, split > 0 ? split : gram_auto_split(N, F)), nslices = gram_slices(F, per);
    std::vector<uint8_t> hits((size_t)(N * F), 0);
    bool ok = per >= 1 && nslices >= 1 && (split <= 0 || nslices <= split);
    int64_t expect0 = 0;
    for (int64_t tb = 0; tb < gram_tiles_side(N) && ok; tb++)
        for (int64_t s = 0; s < nslices && ok; s++) {
            int64_t step0, step1;
            gram_slice_range(F, per, s, &step0, &step1);
            ok = ok && step0 < step1 && step0 == (s == 0 ? 0 : expect0);      // the slices are contiguous and none is empty
            expect0 = step1;
            if (s == nslices - 1) ok = ok && step1 == gram_steps(F);
            // the kernel's own walk: chunks of the slice, trips of kGramUnroll steps that may reach past the chunk's end
            for (int64_t c0 = step0; c0 < step1 && ok; c0 += kGramChunkSteps) {
                const int64_t c1 = c0 + kGramChunkSteps < step1 ? c0 + kGramChunkSteps : step1;
                for (int64_t step = c0; step < c1 && ok; step += kGramUnroll)
                    for (int u = 0; u < kGramUnroll && ok; u++)
                        for (int lane = 0; lane < 64; lane++) {
                            int64_t begin;
                            int count;
                            gram_load_range(N, F, tb * kGramTile + (lane & 31), step + u, c1, lane >> 5, &begin, &count);
                            if (count == 0) continue;
                            if (count < 0 || count > kGramPiece || begin < 0 || begin + count > N * F) { ok = false; break; }
                            if (gram_vec16(F, 0) && (count != kGramPiece || begin % kGramPiece != 0)) { ok = false; break; }
                            for (int q = 0; q < count; q++) hits[(size_t)(begin + q)]++;
                        }
            }
        }
    for (size_t k = 0; k < hits.size() && ok; k++) ok = hits[k] == 1;
    return ok;
}

static void check_cover() {
    for (int64_t N : {(int64_t)1, (int64_t)2, (int64_t)31, (int64_t)32, (int64_t)33, (int64_t)65, (int64_t)200})
        for (int64_t F : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)12288, (int64_t)65536 + 17})
            for (int64_t split : {(int64_t)0, (int64_t)1, (int64_t)7}) item(cover(N, F, split), "cover N F split", N, F, split);
    for (int64_t split : {(int64_t)0, (int64_t)1, (int64_t)7}) item(cover(33, 150528, split), "cover N F split", 33, 150528, split);
    for (int64_t split : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)5000}) item(cover(256, 12288, split), "cover N F split", 256, 12288, split);
    item(cover(3, 100, 1000), "cover N F split", 3, 100, 1000);
}

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 24; }

static bool twin_case(int64_t N, int64_t F, int content, int64_t split) {
    std::vector<uint8_t> x((size_t)(N * F));
    uint32_t seed = (uint32_t)(N * 7919 + F * 31 + content);
    for (int64_t i = 0; i < N; i++)
        for (int64_t f = 0; f < F; f++)
            x[(size_t)(i * F + f)] = content == 0 ? (uint8_t)lcg(seed) : content == 1 ? 0 : content == 2 ? 255 : (i % 2 ? 255 : 0);
    std::vector<int64_t> gram((size_t)(N * N), -1), rowsum((size_t)N, -1);
    pca_gram_host(x.data(), N, F, gram.data(), rowsum.data());
    bool ok = true;
    for (int64_t i = 0; i < N; i++) {
        int64_t r = 0;
        for (int64_t f = 0; f < F; f++) r += x[(size_t)(i * F + f)];
        ok = ok && rowsum[(size_t)i] == r;
        for (int64_t j = 0; j < N; j++) {
            int64_t acc = 0;
            for (int64_t f = 0; f < F; f++) acc += (int64_t)x[(size_t)(i * F + f)] * x[(size_t)(j * F + f)];
            ok = ok && gram[(size_t)(i * N + j)] == acc;
            ok = ok && pca_gram_signed_route(x.data(), N, F, i, j, split, rowsum.data()) == acc;
        }
    }
    return ok;
}

static void check_twin() {
    for (int content = 0; content < 4; content++) {
        bool ok = true;
        for (int64_t F : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)33, (int64_t)1000})
            for (int64_t split : {(int64_t)1, (int64_t)3, (int64_t)7}) ok = ok && twin_case(5, F, content, split);
        ok = ok && twin_case(2, kGramChunk + 17, content, 1) && twin_case(2, 150528, content, 1) && twin_case(2, 150528, content, 2);
        item(ok, "host twin = triple loop = signed route, content", content);
    }
}

static int run_check() {
    check_shift();
    check_chunk();
    check_supported();
    check_tiles();
    check_cover();
    check_twin();
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "check")) return run_check();
    if (argc != 3) { fprintf(stderr, "usage: pca_gram_hostcheck <case> <result> | check\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int64_t> hd;
    std::vector<uint8_t> frames;
    if (!rd(f, hd, 2)) { fprintf(stderr, "short header\n"); fclose(f); return 2; }
    const int64_t N = hd[0], F = hd[1];
    if (!pca_gram_supported(N, F) || N * F > (int64_t)1 << 28) { fprintf(stderr, "bad shape\n"); fclose(f); return 2; }
    const bool ok = rd(f, frames, (size_t)(N * F));
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    std::vector<int64_t> out((size_t)(N * N + N));
    pca_gram_host(frames.data(), N, F, out.data(), out.data() + N * N);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool wrote = wr(f, out);
    return fclose(f) == 0 && wrote ? 0 : 2;
}
