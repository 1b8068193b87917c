// jpeg_decode.hip — decoding of the library's own JPEG streams where they lie on the device (include/srlhip.h: srlhip_jpeg_decode).
// The per-MCU arithmetic is jpeg_decode.hpp's, shared with the host; this file is the parallel frame around it.
//
// The encoder's restart interval is one MCU, so every 16x16 MCU starts byte-aligned behind a marker from DC predictor 0 and decodes
// on its own.  Five launches:
//   0. jpeg_dec_zero_k          the coefficient area of the workspace to zero (entropy decoding stores non-zero coefficients only); a
//                               kernel and not hipMemsetAsync, whose captured form did not replay correctly (profiles/NOTES.md AZ)
//   1. jpeg_dec_scan_k          one workgroup per stream: compares the header, lanes count the markers of their chunk of the data, a
//                               workgroup scan numbers them, every marker is checked against the one its number demands and its
//                               offset written to ends[] -> status[s]
//   2. jpeg_dec_entropy_k       one lane per MCU (the bits of an MCU are sequential), Huffman tables in LDS -> dequantised int16
//                               coefficients; a malformed MCU raises its stream's status to 3
//   3. jpeg_dec_idct_k          eight lanes per 8x8 block: a column each, then a row each -> the Y / Cb / Cr planes
//   4. jpeg_dec_pixels_k        one lane per pixel: chroma upsampling (it reaches across MCU borders: hence the planes), colour, crop;
//                               zeros where the stream's status is not 0
// Reads of the blob stay inside the stream's own [offsets[s], offsets[s + 1]) and, in launch 2, inside the MCU's byte range; the
// workspace is written at ends[n_streams * n_mcus], coef[.. * 384], planes[.. * 384] only, the frames inside [0, frames * H * W * C).
#include <string.h>

#include "internal.hpp"
#include "jpeg_decode.hpp"

using namespace srljpegdec;

namespace {

constexpr int kB = 256;
constexpr int kHeaderWords = (kHeaderBytes + 3) / 4;

struct DecArgs {
    const uint8_t *blob;
    const int64_t *offsets;
    uint8_t *images;
    int32_t *status;
    int32_t *ends;           // [n_streams][nm]: offset (inside the stream) of the marker behind every MCU
    int16_t *coef;           // [n_streams][nm][6][64]
    uint8_t *planes;         // [n_streams]{Y [256 nm], Cb [64 nm], Cr [64 nm]}
    int32_t h, w, views, n_streams, mw, nm;
};
struct DecHeader { uint32_t word[kHeaderWords]; };           // the header every stream of the call must carry, passed by value
static_assert(sizeof(DecArgs) + sizeof(DecHeader) <= 4096, "kernel arguments are limited to 4 KB");
static_assert(sizeof(DecTables) % 4 == 0, "copied to LDS by words");

__constant__ DecTables d_tables = make_dec_tables();

__global__ __launch_bounds__(kB) void jpeg_dec_zero_k(uint4 *p, size_t count) {
    for (size_t i = (size_t)blockIdx.x * kB + threadIdx.x; i < count; i += (size_t)gridDim.x * kB) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kB) void jpeg_dec_scan_k(DecArgs a, DecHeader hd) {
    __shared__ uint32_t part[kB];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int64_t start = a.offsets[s], len = a.offsets[s + 1] - start;
    const uint8_t *p = a.blob + start;
    int st = len <= 0 ? ST_EMPTY : len < kHeaderBytes ? ST_HEADER : ST_OK;          // (the same in every lane, like all of st below)
    if (st == ST_OK) {
        int bad = 0;
        for (int i = tid; i < kHeaderBytes; i += kB)
            if (header_byte_is_compared(i) && p[i] != (uint8_t)(hd.word[i >> 2] >> (8 * (i & 3)))) bad = 1;
        if (__syncthreads_or(bad)) st = ST_HEADER;
    }
    if (st == ST_OK && len >= kMaxStreamBytes) st = ST_DATA;
    if (st != ST_OK) {
        if (tid == 0) a.status[s] = st;
        return;
    }
    // lane `tid` owns the data bytes [lo, hi)
    const int64_t dlen = len - kHeaderBytes, chunk = (dlen + kB - 1) / kB;
    const int64_t lo = kHeaderBytes + (tid * chunk < dlen ? tid * chunk : dlen), hi = lo + chunk < len ? lo + chunk : len;
    uint32_t mine = 0;
    for (int64_t i = lo; i < hi; i++) mine += marker_at(p, i, len) ? 1u : 0u;
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kB; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int bad = part[kB - 1] != (uint32_t)a.nm;
    if (!bad) {
        int64_t k = part[tid] - mine;                        // the number of this lane's first marker: below nm, as the total is nm
        int32_t *ends = a.ends + (size_t)s * a.nm;
        for (int64_t i = lo; i < hi; i++)
            if (marker_at(p, i, len)) {
                if (marker_ok(p, i, len, k, a.nm)) ends[k] = (int32_t)i;
                else bad = 1;
                k++;
            }
    }
    if (__syncthreads_or(bad)) st = ST_DATA;
    if (tid == 0) a.status[s] = st;
}

__global__ __launch_bounds__(kB) void jpeg_dec_entropy_k(DecArgs a) {
    __shared__ DecTables t;
    const int tid = threadIdx.x;
    for (int i = tid; i < (int)(sizeof(DecTables) / 4); i += kB) reinterpret_cast<uint32_t *>(&t)[i] = reinterpret_cast<const uint32_t *>(&d_tables)[i];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * kB + tid;
    if (g >= (int64_t)a.n_streams * a.nm) return;
    const int s = (int)(g / a.nm), m = (int)(g % a.nm);
    if (a.status[s] != ST_OK) return;
    const uint8_t *p = a.blob + a.offsets[s];
    const uint32_t start = m ? (uint32_t)a.ends[g - 1] + 2u : (uint32_t)kHeaderBytes, end = (uint32_t)a.ends[g];
    if (!decode_mcu(p, start, end, p + kDqtAt[0], p + kDqtAt[1], t, a.coef + (size_t)g * 384)) atomicMax(&a.status[s], (int32_t)ST_DATA);
}

// workgroup = 32 blocks x 8 lanes; lane j of a block loads coefficient row j (16 bytes), transforms column j, then row j
__global__ __launch_bounds__(kB) void jpeg_dec_idct_k(DecArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t cf[32][72];
    __shared__ int32_t ws[32][72];                             // [row][column] with rows 9 words apart
    const int tid = threadIdx.x, b = tid >> 3, j = tid & 7;
    const int64_t gb = (int64_t)blockIdx.x * 32 + b;
    const int s = (int)(gb / (6 * (int64_t)a.nm));
    const bool live = gb < (int64_t)a.n_streams * a.nm * 6 && a.status[s] == ST_OK;
    if (live) *reinterpret_cast<uint4 *>(&cf[b][8 * j]) = *reinterpret_cast<const uint4 *>(a.coef + (size_t)gb * 64 + 8 * j);
    __syncthreads();
    if (live) {
        int32_t in[8];
        for (int r = 0; r < 8; r++) in[r] = cf[b][8 * r + j];
        idct8<kPass1Shift>(in, 1, &ws[b][j], 9);
    }
    __syncthreads();
    if (live) {
        int32_t o[8];
        idct8<kPass2Shift>(&ws[b][9 * j], 1, o, 1);
        const int m = (int)((gb / 6) % a.nm), blk = (int)(gb % 6);
        int plane, offset, stride;
        block_place(blk, m / a.mw, m % a.mw, a.mw, &plane, &offset, &stride);
        uint8_t *dst = a.planes + (size_t)s * a.nm * 384 + (plane == 0 ? 0 : plane == 1 ? 256 : 320) * (size_t)a.nm + offset + j * stride;
        uint2 v;
        v.x = sample_of(o[0]) | sample_of(o[1]) << 8 | sample_of(o[2]) << 16 | (uint32_t)sample_of(o[3]) << 24;
        v.y = sample_of(o[4]) | sample_of(o[5]) << 8 | sample_of(o[6]) << 16 | (uint32_t)sample_of(o[7]) << 24;
        *reinterpret_cast<uint2 *>(dst) = v;
    }
}

__global__ __launch_bounds__(kB) void jpeg_dec_pixels_k(DecArgs a) {
    const int64_t hw = (int64_t)a.h * a.w, id = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (id >= hw * a.n_streams) return;
    const int s = (int)(id / hw);
    const int64_t r = id % hw;
    uint8_t *out = a.images + (((int64_t)(s / a.views) * hw + r) * a.views + s % a.views) * 3;
    uint8_t rgb[3] = {0, 0, 0};
    if (a.status[s] == ST_OK) {
        const uint8_t *pl = a.planes + (size_t)s * a.nm * 384;
        const Planes p{pl, pl + 256 * (size_t)a.nm, pl + 320 * (size_t)a.nm, 16 * a.mw, 8 * a.mw, (a.h + 1) / 2, (a.w + 1) / 2};
        pixel_rgb(p, (int)(r / a.w), (int)(r % a.w), rgb);
    }
    out[0] = rgb[0];
    out[1] = rgb[1];
    out[2] = rgb[2];
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// the sizes the call may take, and T = n_streams * n_mcus
bool shape_ok(int n_streams, int h, int w, int64_t *total_mcus) {
    if (!sides_ok(h, w) || n_streams < 0) return false;
    *total_mcus = (int64_t)n_streams * ((h + 15) / 16) * ((w + 15) / 16);
    return *total_mcus * 6 < ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

size_t srlhip_jpeg_decode_workspace_bytes(int32_t n_streams, int32_t img_h, int32_t img_w) {
    int64_t T;
    if (!shape_ok(n_streams, img_h, img_w, &T)) return 0;
    return align256(4 * (size_t)T) + (768 + 384) * (size_t)T;
}

int srlhip_jpeg_decode(int32_t device_id, const uint8_t *blob_dev, const int64_t *offsets_dev, int32_t n_streams, int32_t img_h,
                       int32_t img_w, int32_t n_channels, uint8_t *images_dev, int32_t *status_dev, void *workspace_dev, void *hip_stream) {
    int64_t T;
    if (!shape_ok(n_streams, img_h, img_w, &T) || (n_channels != 3 && n_channels != 6) || n_streams % (n_channels / 3)) return SRLHIP_EINVAL;
    if (!offsets_dev || (n_streams > 0 && (!blob_dev || !images_dev || !status_dev || !workspace_dev))) return SRLHIP_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 16) return SRLHIP_EINVAL;
    if (n_streams == 0) return SRLHIP_OK;
    if (hipSetDevice(device_id) != hipSuccess) return SRLHIP_EHIP;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    DecArgs a;
    a.blob = blob_dev; a.offsets = offsets_dev; a.images = images_dev; a.status = status_dev;
    a.ends = reinterpret_cast<int32_t *>(ws);
    a.coef = reinterpret_cast<int16_t *>(ws + align256(4 * (size_t)T));
    a.planes = ws + align256(4 * (size_t)T) + 768 * (size_t)T;
    a.h = img_h; a.w = img_w; a.views = n_channels / 3; a.n_streams = n_streams;
    a.mw = (img_w + 15) / 16; a.nm = a.mw * ((img_h + 15) / 16);
    DecHeader hd;
    uint8_t header[kHeaderWords * 4] = {0};
    expected_header(img_h, img_w, header);
    memcpy(hd.word, header, sizeof(header));
    const size_t coef_words = 768 * (size_t)T / 16;
    const size_t zero_blocks = (coef_words + kB - 1) / kB;
    hipLaunchKernelGGL(jpeg_dec_zero_k, dim3((unsigned)(zero_blocks < 4096 ? zero_blocks : 4096)), dim3(kB), 0, stream, reinterpret_cast<uint4 *>(a.coef), coef_words);
    const int64_t pixels = (int64_t)n_streams * img_h * img_w;
    hipLaunchKernelGGL(jpeg_dec_scan_k, dim3(n_streams), dim3(kB), 0, stream, a, hd);
    hipLaunchKernelGGL(jpeg_dec_entropy_k, dim3((unsigned)((T + kB - 1) / kB)), dim3(kB), 0, stream, a);
    hipLaunchKernelGGL(jpeg_dec_idct_k, dim3((unsigned)((6 * T + 31) / 32)), dim3(kB), 0, stream, a);
    hipLaunchKernelGGL(jpeg_dec_pixels_k, dim3((unsigned)((pixels + kB - 1) / kB)), dim3(kB), 0, stream, a);
    return hipGetLastError() == hipSuccess ? SRLHIP_OK : SRLHIP_EHIP;
}

int srlhip_jpeg_probe(const uint8_t *stream, size_t len, int32_t *img_h, int32_t *img_w) {
    if (!stream && len) return SRLHIP_EINVAL;
    int h = 0, w = 0;
    if (probe_header(stream, len, &h, &w) != ST_OK) return SRLHIP_ENOTSUP;
    if (img_h) *img_h = h;
    if (img_w) *img_w = w;
    return SRLHIP_OK;
}

int srlhip_jpeg_decode_host(const uint8_t *stream, size_t len, uint8_t *out, int32_t pix_stride, size_t out_cap, int32_t *status) {
    if ((!stream && len) || !out || pix_stride < 3) return SRLHIP_EINVAL;
    int h = 0, w = 0;
    const int st = probe_header(stream, len, &h, &w);
    if (st != ST_OK) {
        if (status) *status = st;
        return SRLHIP_ENOTSUP;
    }
    if (out_cap < ((size_t)h * w - 1) * (size_t)pix_stride + 3) return SRLHIP_ENOMEM;
    std::vector<uint64_t> scratch((host_scratch_bytes(h, w) + 7) / 8);
    const int r = decode_stream_host(stream, len, h, w, out, pix_stride, reinterpret_cast<uint8_t *>(scratch.data()));
    if (status) *status = r;
    return SRLHIP_OK;
}

}  // extern "C"
