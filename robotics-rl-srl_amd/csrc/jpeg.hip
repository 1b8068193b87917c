// jpeg.hip — baseline JPEG encoding of device-resident frames (include/srlhip.h: srlhip_jpeg_encode).  The per-MCU arithmetic is
// jpeg.hpp's, shared with the host; this file is the parallel frame around it.
//
// Restart interval = 1 MCU: every 16x16 MCU is byte-aligned and coded from DC predictor 0, so MCUs are independent.  One workgroup
// per stream, one lane per MCU (lanes stride over the MCUs of larger frames); a lane's two 8x8 working blocks live in LDS with the
// lanes interleaved (element k of lane l at [k][l]: conflict-free).  The call has no handle and no scratch memory, and a stream's
// place in the blob depends on the sizes of all streams before it, so it runs in three launches:
//   1. jpeg_encode_k<B, false>  every lane COUNTS its MCUs' bytes, a workgroup scan sums them: the stream's size (0 + overflow flag
//                               when it exceeds cap_per_stream) -> offsets[s + 1]
//   2. jpeg_scan_k              one workgroup turns the sizes into offsets
//   3. jpeg_encode_k<B, true>   counts again (the scan over MCUs gives every MCU its place inside the stream), then every lane
//                               encodes its MCUs once more and stores the bytes at their final address
// Every store of pass 3 is checked against the end of the stream's own range [offsets[s], offsets[s + 1]).
#include <string.h>

#include <initializer_list>
#include <vector>

#include "internal.hpp"
#include "jpeg.hpp"

using namespace srljpeg;

namespace {

struct JpegArgs {
    const uint8_t *images;
    uint8_t *blob;
    int64_t *offsets;
    int32_t *overflow;
    int64_t cap;
    int32_t h, w, views, n_streams;
};
constexpr int kHeaderWords = (kHeaderBytes + 3) / 4;
struct JpegConst {           // the same for every stream of a call: built on the host, passed by value
    Tables t;
    uint32_t header[kHeaderWords];
};
static_assert(sizeof(Tables) % 4 == 0 && sizeof(JpegArgs) + sizeof(JpegConst) <= 4096, "kernel arguments are limited to 4 KB");

// inclusive scan of part[0 .. B) in place
template <int B>
__device__ void block_scan(uint32_t *part, int tid) {
    for (int d = 1; d < B; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
}

template <int B, bool WRITE>
__global__ __launch_bounds__(B) void jpeg_encode_k(JpegArgs a, JpegConst c) {
    __shared__ Tables t;
    __shared__ int16_t blk[2][64 * B];
    __shared__ uint32_t part[B];
    extern __shared__ uint32_t off[];            // [n_mcus]: byte count of every MCU (trailer included), then its offset behind the header
    const int tid = threadIdx.x, s = blockIdx.x;
    int64_t start = 0, stop = 0;
    if (WRITE) {
        start = a.offsets[s]; stop = a.offsets[s + 1];
        if (stop <= start) return;               // (the whole workgroup) a stream that did not fit
    }
    for (int i = tid; i < (int)(sizeof(Tables) / 4); i += B) reinterpret_cast<uint32_t *>(&t)[i] = reinterpret_cast<const uint32_t *>(&c.t)[i];
    __syncthreads();
    const int frame = s / a.views, view = s % a.views, stride = 3 * a.views;
    const Image im{a.images + (size_t)frame * a.h * a.w * stride + 3 * view, a.h, a.w, stride};
    const int mw = (a.w + 15) / 16, nm = mw * ((a.h + 15) / 16);
    const Block b0{&blk[0][tid], B}, b1{&blk[1][tid], B};
    for (int m = tid; m < nm; m += B) off[m] = encode_mcu<false>(im, m / mw, m % mw, t, b0, b1, nullptr, nullptr) + 2u;
    __syncthreads();
    // lane `tid` owns the MCUs [lo, hi): its sum, a scan over the lanes, then the exclusive offsets back into off[]
    const int per = (nm + B - 1) / B, lo = tid * per < nm ? tid * per : nm, hi = lo + per < nm ? lo + per : nm;
    uint32_t mine = 0;
    for (int m = lo; m < hi; m++) mine += off[m];
    part[tid] = mine;
    __syncthreads();
    block_scan<B>(part, tid);
    const uint32_t total = (uint32_t)kHeaderBytes + part[B - 1];
    if (!WRITE) {
        if (tid == 0) {
            const bool fits = (int64_t)total <= a.cap;
            a.offsets[s + 1] = fits ? (int64_t)total : 0;
            a.overflow[s] = fits ? 0 : 1;
            if (s == 0) a.offsets[0] = 0;
        }
        return;
    }
    uint32_t at = part[tid] - mine;
    for (int m = lo; m < hi; m++) { const uint32_t n = off[m]; off[m] = at; at += n; }
    __syncthreads();
    uint8_t *out = a.blob + start;
    const uint8_t *end = a.blob + stop;
    const int64_t room = stop - start;
    for (int i = tid; i < kHeaderBytes; i += B)
        if (i < room) out[i] = (uint8_t)(c.header[i >> 2] >> (8 * (i & 3)));
    for (int m = tid; m < nm; m += B) {
        uint8_t *p = out + kHeaderBytes + off[m];
        const uint32_t n = encode_mcu<true>(im, m / mw, m % mw, t, b0, b1, p, end);
        if (p + n + 1 < end) { p[n] = 0xFF; p[n + 1] = mcu_trailer(m, nm); }
    }
}

// offsets[1 .. n] hold sizes: make them running sums (offsets[0] is 0)
__global__ __launch_bounds__(256) void jpeg_scan_k(int64_t *offsets, int n) {
    __shared__ int64_t part[256];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        part[tid] = i < n ? offsets[1 + i] : 0;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t v = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        if (i < n) offsets[1 + i] = carry + part[tid];
        carry += part[255];
        __syncthreads();
    }
}

template <int B>
hipError_t launch(const JpegArgs &a, const JpegConst &c, int n_mcus, hipStream_t stream) {
    const size_t dyn = (size_t)n_mcus * sizeof(uint32_t);
    hipLaunchKernelGGL((jpeg_encode_k<B, false>), dim3(a.n_streams), dim3(B), dyn, stream, a, c);
    hipLaunchKernelGGL(jpeg_scan_k, dim3(1), dim3(256), 0, stream, a.offsets, a.n_streams);
    hipLaunchKernelGGL((jpeg_encode_k<B, true>), dim3(a.n_streams), dim3(B), dyn, stream, a, c);
    return hipGetLastError();
}

bool shape_ok(int h, int w, int quality) {
    return h >= kMinSide && h <= kMaxSide && w >= kMinSide && w <= kMaxSide && quality >= 1 && quality <= 100;
}

}  // namespace

int srl::jpeg_encode_launch(const uint8_t *images_dev, int n, int img_h, int img_w, int n_channels, int quality, uint8_t *blob_dev,
                            int64_t cap_per_stream, int64_t *offsets_dev, int32_t *overflow_dev, hipStream_t stream) {
    if (!shape_ok(img_h, img_w, quality) || (n_channels != 3 && n_channels != 6) || n < 0 || n > (1 << 29) || cap_per_stream < 0) return SRLHIP_EINVAL;
    if (!offsets_dev || (n > 0 && (!images_dev || !blob_dev || !overflow_dev))) return SRLHIP_EINVAL;
    JpegArgs a{images_dev, blob_dev, offsets_dev, overflow_dev, cap_per_stream, img_h, img_w, n_channels / 3, n * (n_channels / 3)};
    if (n == 0) return hipMemsetAsync(offsets_dev, 0, sizeof(int64_t), stream) == hipSuccess ? SRLHIP_OK : SRLHIP_EHIP;
    JpegConst c;
    build_tables(quality, &c.t);
    uint8_t header[kHeaderWords * 4] = {0};
    write_header(header, img_h, img_w, quality);
    memcpy(c.header, header, sizeof(header));
    const int n_mcus = ((img_w + 15) / 16) * ((img_h + 15) / 16);
    const hipError_t e = n_mcus <= 64 ? launch<64>(a, c, n_mcus, stream) : launch<128>(a, c, n_mcus, stream);
    return e == hipSuccess ? SRLHIP_OK : SRLHIP_EHIP;
}

extern "C" {

int srlhip_jpeg_encode(int32_t device_id, const uint8_t *images_dev, int32_t n, int32_t img_h, int32_t img_w, int32_t n_channels,
                       int32_t quality, uint8_t *blob_dev, int64_t cap_per_stream, int64_t *offsets_dev, int32_t *overflow_dev,
                       void *hip_stream) {
    if (!shape_ok(img_h, img_w, quality) || (n_channels != 3 && n_channels != 6)) return SRLHIP_EINVAL;      // (before any HIP call)
    if (hipSetDevice(device_id) != hipSuccess) return SRLHIP_EHIP;
    return srl::jpeg_encode_launch(images_dev, n, img_h, img_w, n_channels, quality, blob_dev, cap_per_stream, offsets_dev, overflow_dev,
                                   static_cast<hipStream_t>(hip_stream));
}

size_t srlhip_jpeg_header_bytes(void) { return (size_t)kHeaderBytes; }

int srlhip_jpeg_encode_host(const uint8_t *image, int32_t img_h, int32_t img_w, int32_t pix_stride, int32_t quality, uint8_t *out,
                            size_t cap, size_t *len) {
    if (!image || !len || (!out && cap) || !shape_ok(img_h, img_w, quality) || pix_stride < 3) return SRLHIP_EINVAL;
    return encode_stream_host(image, img_h, img_w, pix_stride, quality, out, cap, len) ? SRLHIP_ENOMEM : SRLHIP_OK;
}

}  // extern "C"
