// jpeg_decode_hostcheck.cpp — csrc/jpeg_decode.hpp (the JPEG decoder's source, the text the kernels of jpeg_decode.hip run) as a
// stand-alone host program.  TESTS ONLY: `make jpegdecodehostcheck` builds it plain and under the address / undefined-behaviour
// sanitizers; tests/test_jpeg_decode_cpu.py runs both.
//
//   jpeg_decode_hostcheck damage [seed] [mutations]
// encodes seeded frames with csrc/jpeg.hpp, damages the streams (cut inside an MCU, a marker removed, two markers swapped, single bytes
// overwritten, `mutations` seeded random edits of 1..8 bytes anywhere, header included) and decodes every one.  Each stream lives in a
// heap block of exactly its own size and the frame in one of exactly its size, so that the sanitizer sees any access outside them; a
// decode must return status 0..3, write zeros unless the status is 0, and give the same bytes when run twice.  Prints one line per
// status count; exit status 0 when every case held.
//   jpeg_decode_hostcheck decode <in.jpg> <out.rgb>
// one file through the decoder: prints "status S h H w W", writes the H x W x 3 frame.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_decode.hpp"

namespace {

uint64_t rng_state = 1;
uint32_t rnd() {                                    // splitmix64, high word
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}

std::vector<uint8_t> make_frame(int kind, int h, int w) {
    std::vector<uint8_t> f((size_t)h * w * 3);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                uint8_t v;
                if (kind == 0) v = (uint8_t)(rnd() & 255);                                   // noise
                else if (kind == 1) v = (uint8_t)((40 * c + 200 * y / h + 55 * x / w) & 255);  // gradient
                else v = ((x + y) & 1) ? 255 : 0;                                            // checkerboard
                f[((size_t)y * w + x) * 3 + c] = v;
            }
    return f;
}

std::vector<uint8_t> encode(const std::vector<uint8_t> &frame, int h, int w, int quality) {
    std::vector<uint8_t> out(2048 + 12 * (size_t)h * w);
    size_t len = 0;
    if (srljpeg::encode_stream_host(frame.data(), h, w, 3, quality, out.data(), out.size(), &len)) abort();
    out.resize(len);
    return out;
}

int counts[4], failures, cases;

// status, or -1 when a property did not hold
int run_case(const std::vector<uint8_t> &stream, int h, int w) {
    uint8_t *in = (uint8_t *)malloc(stream.size() ? stream.size() : 1);
    if (!stream.empty()) memcpy(in, stream.data(), stream.size());
    const size_t n = (size_t)h * w * 3;
    uint8_t *a = (uint8_t *)malloc(n), *b = (uint8_t *)malloc(n);
    memset(a, 0xA5, n);
    memset(b, 0x5A, n);
    std::vector<uint8_t> scratch(srljpegdec::host_scratch_bytes(h, w) + 8);
    uint8_t *sc = scratch.data() + (8 - (uintptr_t)scratch.data() % 8) % 8;
    const int st = srljpegdec::decode_stream_host(in, stream.size(), h, w, a, 3, sc);
    const int st2 = srljpegdec::decode_stream_host(in, stream.size(), h, w, b, 3, sc);
    bool ok = st >= 0 && st <= 3 && st == st2 && memcmp(a, b, n) == 0 && (stream.empty() || memcmp(in, stream.data(), stream.size()) == 0);
    if (st != 0)
        for (size_t i = 0; i < n; i++) ok = ok && a[i] == 0;
    free(in);
    free(a);
    free(b);
    cases++;
    if (!ok) { failures++; return -1; }
    counts[st]++;
    return st;
}

std::vector<size_t> markers(const std::vector<uint8_t> &s) {
    std::vector<size_t> at;
    for (size_t i = srljpegdec::kHeaderBytes; i + 1 < s.size(); i++)
        if (s[i] == 0xFF && s[i + 1] != 0) at.push_back(i);
    return at;
}

int damage(uint64_t seed, int mutations) {
    rng_state = seed;
    const int shapes[3][2] = {{16, 16}, {24, 40}, {64, 64}};
    std::vector<std::vector<uint8_t>> streams;
    std::vector<int> hs, ws;
    for (int k = 0; k < 9; k++) {
        const int h = shapes[k % 3][0], w = shapes[k % 3][1];
        streams.push_back(encode(make_frame(k / 3, h, w), h, w, k % 2 ? 95 : 50));
        hs.push_back(h);
        ws.push_back(w);
    }
    for (size_t k = 0; k < streams.size(); k++) {
        const std::vector<uint8_t> &s = streams[k];
        const int h = hs[k], w = ws[k];
        if (run_case(s, h, w) != 0) { printf("intact stream %zu did not decode\n", k); failures++; }
        const std::vector<size_t> at = markers(s);
        // cut: inside the header, inside the first MCU, inside the last one, the EOI's second byte
        for (size_t cut : {(size_t)0, (size_t)100, (size_t)srljpegdec::kHeaderBytes + 1, s.size() - 3, s.size() - 1})
            if (run_case(std::vector<uint8_t>(s.begin(), s.begin() + cut), h, w) == 0) { printf("cut stream %zu decoded\n", k); failures++; }
        if (at.size() >= 3) {
            std::vector<uint8_t> d = s;
            d.erase(d.begin() + at[0], d.begin() + at[0] + 2);                           // a marker removed
            if (run_case(d, h, w) == 0) { printf("stream %zu without a marker decoded\n", k); failures++; }
            d = s;
            d[at[0] + 1] = s[at[1] + 1];                                                  // two markers swapped
            d[at[1] + 1] = s[at[0] + 1];
            if (run_case(d, h, w) == 0) { printf("stream %zu with swapped markers decoded\n", k); failures++; }
        }
        for (size_t pos = srljpegdec::kHeaderBytes; pos < s.size(); pos += 1 + s.size() / 64)
            for (int v : {0x00, 0xFF, 0x55}) {
                std::vector<uint8_t> d = s;
                d[pos] = (uint8_t)v;
                run_case(d, h, w);
            }
    }
    for (int i = 0; i < mutations; i++) {
        const size_t k = rnd() % streams.size();
        std::vector<uint8_t> d = streams[k];
        const int edits = 1 + (int)(rnd() % 8);
        const bool data_only = rnd() % 4 != 0;                                            // three in four leave the header alone
        for (int e = 0; e < edits; e++) {
            const size_t lo = data_only ? srljpegdec::kHeaderBytes : 0;
            d[lo + rnd() % (d.size() - lo)] = (uint8_t)(rnd() % 3 == 0 ? 0xFF : rnd());
        }
        if (rnd() % 8 == 0) d.resize(rnd() % d.size());
        run_case(d, hs[k], ws[k]);
    }
    printf("cases %d\n", cases);
    for (int s = 0; s < 4; s++) printf("status %d: %d\n", s, counts[s]);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

int decode_file(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 2;
    std::vector<uint8_t> s;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) s.insert(s.end(), buf, buf + n);
    fclose(f);
    int h = 0, w = 0;
    const int st = srljpegdec::probe_header(s.data(), s.size(), &h, &w);
    if (st != srljpegdec::ST_OK) { printf("status %d h 0 w 0\n", st); return 0; }
    std::vector<uint8_t> out((size_t)h * w * 3);
    std::vector<uint64_t> scratch(srljpegdec::host_scratch_bytes(h, w) / 8 + 1);
    printf("status %d h %d w %d\n", srljpegdec::decode_stream_host(s.data(), s.size(), h, w, out.data(), 3, (uint8_t *)scratch.data()), h, w);
    f = fopen(out_path, "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "damage")) return damage(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1, argc > 3 ? atoi(argv[3]) : 400);
    if (argc == 4 && !strcmp(argv[1], "decode")) return decode_file(argv[2], argv[3]);
    fprintf(stderr, "usage: jpeg_decode_hostcheck damage [seed] [mutations] | decode <in.jpg> <out.rgb>\n");
    return 2;
}
