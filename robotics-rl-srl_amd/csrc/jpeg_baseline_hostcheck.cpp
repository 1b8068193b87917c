// jpeg_baseline_hostcheck.cpp — csrc/jpeg_baseline.hpp (the baseline JPEG decoder's source, the text the kernels of jpeg_baseline.hip
// run) as a stand-alone host program.  TESTS ONLY: `make jpegbaselinehostcheck` builds it plain and under the address /
// undefined-behaviour sanitizers; tests/test_jpeg_baseline_cpu.py runs both.
//
//   jpeg_baseline_hostcheck batch <in.bin> <out.bin>
// in.bin holds records of three little-endian int32 (h, w, len) and len bytes of stream.  Every stream is decoded for sides h x w from a
// heap block of exactly its own size, at every one of the 16 alignments the bit source's aligned fetch can meet, into a frame of exactly
// h w 3 bytes, so that the sanitizer sees any access outside them; a decode must return status 0..3, write zeros unless the status is 0,
// leave the stream as it was and give the same bytes at every alignment.  Prints "status S" per record, then "failures N"; writes the
// frames to out.bin back to back; exit status 0 when every case held.
//   jpeg_baseline_hostcheck decode <in.jpg> <out.rgb>
// one file through the decoder: prints "status S h H w W sampling M", writes the H x W x 3 frame.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_baseline.hpp"

namespace {

bool read_file(const char *path, std::vector<uint8_t> *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

// status, or -1 when a property did not hold; the frame of alignment 0 is appended to frames
int run_case(const uint8_t *stream, size_t len, int h, int w, std::vector<uint8_t> *frames) {
    const size_t n = (size_t)h * w * 3;
    std::vector<uint64_t> scratch(srljpegbase::host_scratch_bytes_baseline(h, w) / 8 + 1);
    std::vector<uint8_t> first;
    int first_status = -1;
    bool ok = true;
    for (int shift = 0; shift < 16 && ok; shift++) {
        // a block of shift + len bytes: malloc's blocks are 16-byte aligned, so the stream begins `shift` bytes behind an aligned
        // address and ends with the block
        uint8_t *block = (uint8_t *)malloc(shift + len ? shift + len : 1), *in = block + shift;
        if (len) memcpy(in, stream, len);
        uint8_t *frame = (uint8_t *)malloc(n);
        memset(frame, 0xA5, n);
        const int st = srljpegbase::decode_stream_baseline_host(in, len, h, w, frame, 3, (uint8_t *)scratch.data());
        ok = st >= 0 && st <= 3 && (!len || memcmp(in, stream, len) == 0);
        if (st != 0)
            for (size_t i = 0; i < n; i++) ok = ok && frame[i] == 0;
        if (shift == 0) {
            first.assign(frame, frame + n);
            first_status = st;
        } else {
            ok = ok && st == first_status && memcmp(frame, first.data(), n) == 0;
        }
        free(frame);
        free(block);
    }
    if (!ok) return -1;
    frames->insert(frames->end(), first.begin(), first.end());
    return first_status;
}

int batch(const char *in_path, const char *out_path) {
    std::vector<uint8_t> file, frames;
    if (!read_file(in_path, &file)) return 2;
    int failures = 0;
    for (size_t at = 0; at < file.size();) {
        int32_t head[3];
        if (at + sizeof(head) > file.size()) return 2;
        memcpy(head, file.data() + at, sizeof(head));
        at += sizeof(head);
        if (head[0] < 8 || head[0] > 1024 || head[1] < 8 || head[1] > 1024 || head[2] < 0 || at + (size_t)head[2] > file.size()) return 2;
        const int st = run_case(file.data() + at, (size_t)head[2], head[0], head[1], &frames);
        at += (size_t)head[2];
        if (st < 0) {
            failures++;
            frames.resize(frames.size() + (size_t)head[0] * head[1] * 3);
        }
        printf("status %d\n", st);
    }
    printf("failures %d\n", failures);
    FILE *f = fopen(out_path, "wb");
    if (!f || (frames.size() && fwrite(frames.data(), 1, frames.size(), f) != frames.size())) return 2;
    fclose(f);
    return failures ? 1 : 0;
}

int decode_file(const char *in_path, const char *out_path) {
    std::vector<uint8_t> s;
    if (!read_file(in_path, &s)) return 2;
    int h = 0, w = 0, mode = 0;
    const int st = srljpegbase::probe_baseline(s.data(), s.size(), &h, &w, &mode);
    if (st != srljpegbase::ST_OK) { printf("status %d h 0 w 0 sampling 0\n", st); return 0; }
    std::vector<uint8_t> out((size_t)h * w * 3);
    std::vector<uint64_t> scratch(srljpegbase::host_scratch_bytes_baseline(h, w) / 8 + 1);
    printf("status %d h %d w %d sampling %d\n", srljpegbase::decode_stream_baseline_host(s.data(), s.size(), h, w, out.data(), 3, (uint8_t *)scratch.data()), h, w, mode);
    FILE *f = fopen(out_path, "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "batch")) return batch(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "decode")) return decode_file(argv[2], argv[3]);
    fprintf(stderr, "usage: jpeg_baseline_hostcheck batch <in.bin> <out.bin> | decode <in.jpg> <out.rgb>\n");
    return 2;
}
