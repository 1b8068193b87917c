// jpeg_hostcheck.cpp — csrc/jpeg.hpp (the JPEG encoder's per-MCU source, the text the kernels of jpeg.hip run) compiled for the host
// alone.  TESTS ONLY: `make jpeghostcheck`; tests/test_jpeg_cpu.py holds it to tests/jpeg_ref.py byte for byte.
#include <initializer_list>

#include "jpeg.hpp"

extern "C" {

// one stream; returns 0 (written), 1 (cap too small: only *len is set), -1 (bad arguments)
int hostcheck_jpeg_encode(const uint8_t *image, int img_h, int img_w, int pix_stride, int quality, uint8_t *out, size_t cap, size_t *len) {
    if (!image || !len || img_h < srljpeg::kMinSide || img_h > srljpeg::kMaxSide || img_w < srljpeg::kMinSide || img_w > srljpeg::kMaxSide ||
        quality < 1 || quality > 100 || pix_stride < 3)
        return -1;
    return srljpeg::encode_stream_host(image, img_h, img_w, pix_stride, quality, out, cap, len);
}

// the 8x8 transform and the quantiser's reciprocal on their own: block[64] in place; q[64] = quantised values of component `comp`, zigzag order
void hostcheck_jpeg_block(int16_t *block, int comp, int quality, int32_t *q) {
    srljpeg::Tables t;
    srljpeg::build_tables(quality, &t);
    const srljpeg::Block b{block, 1};
    srljpeg::fdct(b);
    for (int i = 0; i < 64; i++) {
        const int c = b[t.zigzag[i]];
        const uint32_t x = (uint32_t)(c < 0 ? -c : c) + t.half[comp][i];
        const int v = (int)(uint32_t)(((uint64_t)x * t.recip[comp][i]) >> 32);
        q[i] = c < 0 ? -v : v;
    }
}

}
