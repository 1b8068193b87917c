// encoder_pack_hostcheck.cpp — the SRL encoder's host logic (encoder_pack.hpp, the text encoder.hip and encoder_general.hip include) as a
// stand-alone host program: `encoder_pack_hostcheck <case file> <result file>`.  TESTS ONLY (make encoderpackhostcheck;
// tests/test_encoder_pack_hostcheck_cpu.py writes the case, reads the result and compares it with the library and with recorded digests).
//   case    int32 [4]   C state_dim H W
//           float32     conv1_w [64][C][7][7], conv1_b [64], conv2_w [64][64][3][3], conv3_w [64][64][3][3]
//           float32     fc_w [state_dim][F], F = the frame shape's feature count (absent for a shape that is not covered)
//   result  int32 [17]  geometry: H W C Hc[3] Wc[3] Hp[3] Wp[3] ok F
//           int32 [6][5] the fused kernel's launch choice for SRLHIP_ENCODER_WAVES in (unset, 4, 8) x SRLHIP_ENCODER_L1=f16 (no, yes):
//                       groups, l1_i8, index into the variant table, and that entry's (MG, I8)
//           the first-layer pack for C: layer1_bytes(C) bytes, float32 scale
//           C = 3 only: the fused pack, kPackFusedBytes bytes, float32 scales [3]; the int8 pack for zero_slot 0, kPackI8Bytes bytes,
//                       float32 inv256 [64]; the same for zero_slot 7
//           float32     the reordered FC matrix [state_dim][F] (covered shapes)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "encoder_pack.hpp"

using namespace srlenc;

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T> static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: encoder_pack_hostcheck <case> <result>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd;
    if (!rd(f, hd, 4)) { fprintf(stderr, "short header\n"); return 2; }
    const int C = hd[0], state_dim = hd[1];
    if ((C != 3 && C != 6) || state_dim < 1 || state_dim > 4096) { fprintf(stderr, "bad shape\n"); return 2; }
    const Geometry g = geometry(hd[2], hd[3], C);
    const size_t F = (size_t)feature_count(g);
    std::vector<float> w1, b1, w2, w3, fc;
    const bool ok = rd(f, w1, (size_t)64 * C * 49) && rd(f, b1, 64) && rd(f, w2, 64 * 64 * 9) && rd(f, w3, 64 * 64 * 9) && rd(f, fc, state_dim * F);
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 2; }

    std::vector<int32_t> geo = {g.H, g.W, g.C, g.Hc[0], g.Hc[1], g.Hc[2], g.Wc[0], g.Wc[1], g.Wc[2], g.Hp[0], g.Hp[1], g.Hp[2],
                                g.Wp[0], g.Wp[1], g.Wp[2], g.ok ? 1 : 0, (int32_t)F};
    std::vector<int32_t> choice;
    for (int waves : {0, 4, 8})
        for (int want_f16 : {0, 1}) {
            const int groups = fused_groups(waves), i8 = fused_l1_i8(groups, want_f16 != 0) ? 1 : 0, v = fused_variant(groups, i8 != 0);
            for (int x : {groups, i8, v, kFusedVariants[v].groups, kFusedVariants[v].l1_i8 ? 1 : 0}) choice.push_back(x);
        }
    // every image in a buffer of exactly its size: a packer that writes past its image is the sanitizer build's to catch
    std::vector<_Float16> first(layer1_bytes(C) / 2);
    std::vector<float> first_scale = {pack_layer1_f16(w1.data(), b1.data(), C, first.data())};
    std::vector<char> fused;
    std::vector<float> fused_scales, inv0, inv7;
    std::vector<int8_t> dig0, dig7;
    if (C == 3) {
        fused.resize(kPackFusedBytes); fused_scales.resize(3);
        pack_fused(w1.data(), b1.data(), w2.data(), w3.data(), fused.data(), fused_scales.data());
        dig0.resize(kPackI8Bytes); inv0.resize(64); dig7.resize(kPackI8Bytes); inv7.resize(64);
        pack_layer1_i8(w1.data(), b1.data(), 0, dig0.data(), inv0.data());
        pack_layer1_i8(w1.data(), b1.data(), 7, dig7.data(), inv7.data());
    }
    std::vector<float> fc_out(fc.size());
    if (F) reorder_fc(fc.data(), state_dim, g.Hp[2], g.Wp[2], fc_out.data());

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool wrote = wr(f, geo) && wr(f, choice) && wr(f, first) && wr(f, first_scale) && wr(f, fused) && wr(f, fused_scales) && wr(f, dig0) &&
                       wr(f, inv0) && wr(f, dig7) && wr(f, inv7) && wr(f, fc_out);
    return fclose(f) == 0 && wrote ? 0 : 2;
}
