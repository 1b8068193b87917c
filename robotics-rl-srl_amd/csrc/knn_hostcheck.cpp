// knn_hostcheck.cpp — srlhip_knn's arithmetic, order, rules and index math (knn.hpp, the text the kernels of knn.hip call) as a
// stand-alone host program.  TESTS ONLY (make knnhostcheck; tests/test_knn_cpu.py).
//   knn_hostcheck <case file> <result file>
//     case    int64 [6]   N S k Q G f32        (Q = 0: no query list, every row is a query; G = 0: no ground truth)
//             float64 or float32 states [N][S], int32 queries [Q], float64 ground truth [N][G]
//     result  int32 idx [Q'][k], float64 dist [Q'][k], float64 err [Q'] (with a ground truth)      (the host twin; Q' = Q or N)
//   knn_hostcheck check       proves, and prints one line per item ("ok ..." / "FAIL ..."; exit status 1 on any FAIL):
//     list      KnnList<8> and <32> against a full sort of random (d, j) pairs with many equal d, NaN and +inf among them
//     slices    for a table of (N, Q, split) the slices are whole tiles, contiguous, none empty, and cover 0 .. N - 1 once; the merge of
//               the slices' lists equals the list of the whole range
//     rules     check_knn and knn_workspace_bytes at the edges of every bound
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "hostcheck_io.hpp"
#include "knn.hpp"

using namespace srl;

static int g_fail = 0;
static void item(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0) {
    printf("%s %s %lld %lld %lld\n", ok ? "ok" : "FAIL", what, a, b, c);
    if (!ok) g_fail = 1;
}

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

struct Pair { double d; int32_t j; };
static bool pair_before(const Pair &a, const Pair &b) { return knn_before(a.d, a.j, b.d, b.j); }

static std::vector<Pair> random_pairs(int count, uint32_t seed) {
    std::vector<Pair> p((size_t)count);
    for (int n = 0; n < count; n++) {
        const uint32_t r = lcg(seed) % 16;
        p[(size_t)n] = {r == 0 ? NAN : r == 1 ? INFINITY : (double)(lcg(seed) % 7), n};
    }
    for (int n = count - 1; n > 0; n--) std::swap(p[(size_t)n], p[(size_t)(lcg(seed) % (uint32_t)(n + 1))]);
    return p;
}

template <int KMAX> static bool list_case(int count, uint32_t seed) {
    const std::vector<Pair> p = random_pairs(count, seed);
    KnnList<KMAX> l;
    l.clear();
    for (const Pair &c : p) l.offer(c.d, c.j);
    std::vector<Pair> want;
    for (const Pair &c : p)
        if (c.d < INFINITY) want.push_back(c);              // neither NaN nor +inf enters
    std::sort(want.begin(), want.end(), pair_before);
    bool ok = true;
    for (int n = 0; n < KMAX; n++) {
        if ((size_t)n < want.size()) ok = ok && l.j[n] == want[(size_t)n].j && knn_bits(l.d[n]) == knn_bits(want[(size_t)n].d);
        else ok = ok && l.j[n] == -1 && l.d[n] == INFINITY;
    }
    return ok;
}

static void check_list() {
    bool ok = true;
    for (int count : {0, 1, 5, 8, 9, 31, 32, 33, 200})
        for (uint32_t seed = 1; seed <= 5; seed++) ok = ok && list_case<8>(count, seed) && list_case<32>(count, seed);
    item(ok, "a list is the head of the full sort, NaN and +inf stay out");
}

static bool slices_case(int64_t N, int64_t Q, int32_t split) {
    const int64_t per = knn_slice_len_for(N, Q, split), nslices = knn_slices(N, per);
    bool ok = per >= 1 && per % kKnnTile == 0 && nslices >= 1 && (split <= 0 || nslices <= split) && (nslices - 1) * per < N && nslices * per >= N;
    // merge of the slices' lists = the list of the whole range
    const std::vector<Pair> p = random_pairs((int)N, (uint32_t)(N * 31 + split));
    KnnList<8> whole, merged;
    whole.clear(); merged.clear();
    for (int64_t j = 0; j < N; j++) whole.offer(p[(size_t)j].d, (int32_t)j);
    for (int64_t c = 0; c < nslices; c++) {
        KnnList<8> part;
        part.clear();
        for (int64_t j = c * per; j < std::min((c + 1) * per, N); j++) part.offer(p[(size_t)j].d, (int32_t)j);
        for (int n = 0; n < 5; n++)                          // k = 5 of the 8 slots travel
            if (part.j[n] >= 0) merged.offer(part.d[n], part.j[n]);
    }
    for (int n = 0; n < 5; n++) ok = ok && whole.j[n] == merged.j[n] && knn_bits(whole.d[n]) == knn_bits(merged.d[n]);
    return ok;
}

static void check_slices() {
    for (int64_t N : {(int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)130, (int64_t)1000, (int64_t)4096, (int64_t)65536})
        for (int64_t Q : {(int64_t)1, (int64_t)300, (int64_t)4096})
            for (int32_t split : {0, 1, 7, 5000}) item(slices_case(N, Q, split), "slices N Q split", N, Q, split);
    item(knn_auto_split(4096, 4096) == 4 && knn_auto_split(65536, 4096) == 32 && knn_auto_split(1000, 300) == 1 && knn_auto_split(1 << 20, 1) == 64,
         "automatic split");
}

static void check_rules() {
    bool ok = knn_supported(2, 1, 1, 1, 0) && knn_supported(1 << 20, 64, 32, 1 << 20, 32) && !knn_supported(1, 1, 1, 1, 0) &&
              !knn_supported((1 << 20) + 1, 1, 1, 1, 0) && !knn_supported(100, 65, 1, 1, 0) && !knn_supported(100, 0, 1, 1, 0) &&
              !knn_supported(100, 8, 33, 1, 0) && !knn_supported(100, 8, 0, 1, 0) && !knn_supported(5, 8, 5, 1, 0) && knn_supported(5, 8, 4, 1, 0) &&
              !knn_supported(100, 8, 5, 0, 0) && !knn_supported(100, 8, 5, (1 << 20) + 1, 0) && !knn_supported(100, 8, 5, 1, 33) &&
              !knn_supported(100, 8, 5, 1, -1);
    item(ok, "supported at the edges of every bound");
    ok = check_knn(100, 8, 5, 10, 0, 0, true, true, true, false, false).code == 0 && check_knn(100, 8, 5, 10, 3, 7, true, true, true, true, true).code == 0 &&
         check_knn(100, 8, 5, 10, 0, -1, true, true, true, false, false).code == SRLHIP_EINVAL &&
         check_knn(100, 8, 5, 10, 0, 0, false, true, true, false, false).code == SRLHIP_EINVAL &&
         check_knn(100, 8, 5, 10, 0, 0, true, false, true, false, false).code == SRLHIP_EINVAL &&
         check_knn(100, 8, 5, 10, 0, 0, true, true, false, false, false).code == SRLHIP_EINVAL &&
         check_knn(100, 8, 5, 10, 3, 0, true, true, true, true, false).code == SRLHIP_EINVAL &&
         check_knn(100, 8, 5, 10, 3, 0, true, true, true, false, true).code == SRLHIP_EINVAL &&
         check_knn(100, 8, 5, 10, 33, 0, true, true, true, true, true).code == SRLHIP_ENOTSUP &&
         check_knn(100, 8, 5, 10, 0, 0, true, true, true, true, true).code == SRLHIP_ENOTSUP &&
         check_knn(100, 65, 5, 10, 0, 0, true, true, true, false, false).code == SRLHIP_ENOTSUP;
    item(ok, "refusals by code");
    ok = knn_workspace_bytes(1, 1, 1, 1, 0) == 0 && knn_workspace_bytes(100, 8, 5, 10, -1) == 0 && knn_workspace_bytes(100, 8, 5, 10, 1) == 5 * 10 * 12 &&
         knn_workspace_bytes(130, 8, 5, 10, 7) == 3 * 5 * 10 * 12 && knn_workspace_bytes(4096, 8, 5, 4096, 0) == (size_t)4 * 5 * 4096 * 12;
    item(ok, "workspace bytes");
}

static int run_check() {
    check_list();
    check_slices();
    check_rules();
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "check")) return run_check();
    if (argc != 3) { fprintf(stderr, "usage: knn_hostcheck <case> <result> | check\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int64_t> hd;
    if (!rd(f, hd, 6)) { fprintf(stderr, "short header\n"); fclose(f); return 2; }
    const int64_t N = hd[0], S = hd[1], k = hd[2], Q = hd[3], G = hd[4], f32 = hd[5];
    const int64_t rows = Q ? Q : N;
    if (!knn_supported(N, S, k, rows, G) || N * S > (int64_t)1 << 24 || (f32 != 0 && f32 != 1)) { fprintf(stderr, "bad shape\n"); fclose(f); return 2; }
    std::vector<double> x64, gt;
    std::vector<float> x32;
    std::vector<int32_t> queries;
    bool ok = f32 ? rd(f, x32, (size_t)(N * S)) : rd(f, x64, (size_t)(N * S));
    ok = ok && rd(f, queries, (size_t)Q) && rd(f, gt, (size_t)(N * G));
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }
    std::vector<int32_t> idx((size_t)(rows * k));
    std::vector<double> dist((size_t)(rows * k)), err((size_t)(G ? rows : 0));
    if (!knn_host(f32 ? (const void *)x32.data() : (const void *)x64.data(), (int32_t)f32, N, S, Q ? queries.data() : nullptr, rows, (int32_t)k,
                  G ? gt.data() : nullptr, (int32_t)G, idx.data(), dist.data(), G ? err.data() : nullptr)) {
        fprintf(stderr, "a query index is outside 0..n-1\n");
        return 2;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool wrote = wr(f, idx) && wr(f, dist) && wr(f, err);
    return fclose(f) == 0 && wrote ? 0 : 2;
}
