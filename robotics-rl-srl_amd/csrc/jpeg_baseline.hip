// jpeg_baseline.hip — decoding of baseline JPEG streams as libjpeg writes them by default, where they lie on the device
// (include/srlhip.h: srlhip_jpeg_decode_baseline).  The per-stream work is jpeg_baseline.hpp's (and, behind the coefficients,
// jpeg_decode.hpp's), shared with the host; this file is the parallel frame around it.
//
// Such a stream is ONE interleaved scan: DC predictors and the bit position run across MCUs, so its entropy decode is sequential from
// SOS to the last MCU (restart markers, where a stream has them, are honoured but not used to split it).  Five launches:
//   0. jpeg_base_zero_k         the coefficient area of the workspace to zero (entropy decoding stores non-zero coefficients only); a
//                               kernel and not hipMemsetAsync, whose captured form did not replay correctly (profiles/NOTES.md AZ)
//   1. jpeg_base_parse_k        one lane per stream walks the marker segments -> the stream's descriptor in the workspace, status[s]
//   2. jpeg_base_entropy_k      one lane per stream, Huffman tables in LDS, the stream's bytes fetched in aligned 16-byte pieces into
//                               registers, its three quantisation tables in LDS (dynamic, 192 bytes per active lane) -> dequantised
//                               int16 coefficients; malformed data sets the stream's status to 3.  Only the
//                               first `lanes` lanes of a wavefront take a stream (kEntropyLanes below, measured)
//   3. jpeg_base_idct_k         eight lanes per 8x8 block: a column each, then a row each -> the Y / Cb / Cr planes of the stream's mode
//   4. jpeg_base_pixels_k       one lane per pixel: 4:2:0 upsampling or the 4:4:4 direct path, colour, crop; zeros where the stream's
//                               status is not 0
// Reads of the blob stay inside the stream's own [offsets[s], offsets[s + 1]); the workspace is written at desc[n_streams],
// coef[n_streams * cap * 64], planes[n_streams * cap * 64] only (cap = blocks_cap(H, W)), the frames inside [0, frames * H * W * C).
#include <string.h>

#include "internal.hpp"
#include "jpeg_baseline.hpp"

using namespace srljpegbase;

namespace {

constexpr int kB = 256;
// Active lanes per wavefront in the entropy launch.  4096 streams are 64 wavefronts at 64 lanes, 1024 at 4: fewer lanes trade lockstep
// divergence (every lane waits for the longest symbol path among its neighbours) for coverage of the chip's 1024 SIMDs.  Measured at
// 4096 streams of 64x64 / 224x224 (profiles/NOTES.md BB): 64 lanes 6.24 / 46.8 ms, 16 lanes 6.42 / 45.9 ms, 4 lanes 5.01 / 34.3 ms for the
// whole call.  SRLHIP_JPEG_BASELINE_LANES (64, 16 or 4; include/srlhip.h) overrides it per call: the measurement and
// tests/test_gpu_jpeg_baseline.py use that.
constexpr int kEntropyLanes = 4;

struct BaseArgs {
    const uint8_t *blob;
    const int64_t *offsets;
    uint8_t *images;
    int32_t *status;
    Desc *desc;              // [n_streams]
    int16_t *coef;           // [n_streams][cap][64]
    uint8_t *planes;         // [n_streams][cap * 64]: Y, Cb, Cr of the stream's mode
    int32_t h, w, views, n_streams, cap, lanes;
};
static_assert(sizeof(DecTables) % 4 == 0, "copied to LDS by words");

__constant__ DecTables d_base_tables = make_dec_tables();
__constant__ K3Bits d_k3_bits = make_k3_bits();

__global__ __launch_bounds__(kB) void jpeg_base_zero_k(uint4 *p, size_t count) {
    for (size_t i = (size_t)blockIdx.x * kB + threadIdx.x; i < count; i += (size_t)gridDim.x * kB) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kB) void jpeg_base_parse_k(BaseArgs a) {
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= a.n_streams) return;
    const int64_t start = a.offsets[s], len = a.offsets[s + 1] - start;
    int h = 0, w = 0;
    int st = parse_baseline(a.blob + start, len, d_k3_bits, d_base_tables, &a.desc[s], &h, &w);
    if (st == ST_OK && (h != a.h || w != a.w)) st = ST_HEADER;
    if (st == ST_OK && len >= kMaxStreamBytes) st = ST_DATA;
    a.status[s] = st;
}

__global__ __launch_bounds__(kB) void jpeg_base_entropy_k(BaseArgs a) {
    __shared__ DecTables t;
    extern __shared__ __attribute__((aligned(16))) uint8_t q_lds[];      // [kB / 64 * a.lanes][3][64]
    const int tid = threadIdx.x;
    for (int i = tid; i < (int)(sizeof(DecTables) / 4); i += kB) reinterpret_cast<uint32_t *>(&t)[i] = reinterpret_cast<const uint32_t *>(&d_base_tables)[i];
    __syncthreads();
    const int lane = tid & 63, wave = blockIdx.x * (kB / 64) + (tid >> 6);
    if (lane >= a.lanes) return;
    const int64_t s = (int64_t)wave * a.lanes + lane;
    if (s >= a.n_streams || a.status[s] != ST_OK) return;
    const int64_t start = a.offsets[s];
    const Desc &d = a.desc[s];
    const Geo g = geo_of(a.h, a.w, (int)d.sampling);
    uint8_t *q3 = q_lds + 192 * ((tid >> 6) * a.lanes + lane);
    for (int c = 0; c < 3; c++) {                                       // (a table is 64 bytes at a 16-byte aligned place of the descriptor)
        const uint4 *src = reinterpret_cast<const uint4 *>(d.q[sel_tq(d.sel, c)]);
        for (int i = 0; i < 4; i++) reinterpret_cast<uint4 *>(q3 + 64 * c)[i] = src[i];
    }
    const int st = decode_scan(a.blob + start, (uint32_t)(a.offsets[s + 1] - start), d, q3, g, t, a.coef + (size_t)s * a.cap * 64);
    if (st != ST_OK) a.status[s] = st;
}

// workgroup = 32 blocks x 8 lanes; lane j of a block loads coefficient row j (16 bytes), transforms column j, then row j
__global__ __launch_bounds__(kB) void jpeg_base_idct_k(BaseArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t cf[32][72];
    __shared__ int32_t ws[32][72];                             // [row][column] with rows 9 words apart
    const int tid = threadIdx.x, b = tid >> 3, j = tid & 7;
    const int64_t gb = (int64_t)blockIdx.x * 32 + b;
    const int s = (int)(gb / a.cap), sb = (int)(gb % a.cap);
    bool live = s < a.n_streams && a.status[s] == ST_OK;
    Geo g = geo_of(a.h, a.w, 1);
    int sampling = 1;
    if (live) {
        sampling = (int)a.desc[s].sampling;
        g = geo_of(a.h, a.w, sampling);
        live = sb < g.nblocks;
    }
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
        int offset, stride;
        block_place_scan(g, sampling, sb, &offset, &stride);
        uint8_t *dst = a.planes + (size_t)s * a.cap * 64 + offset + j * stride;
        uint2 v;
        v.x = sample_of(o[0]) | sample_of(o[1]) << 8 | sample_of(o[2]) << 16 | (uint32_t)sample_of(o[3]) << 24;
        v.y = sample_of(o[4]) | sample_of(o[5]) << 8 | sample_of(o[6]) << 16 | (uint32_t)sample_of(o[7]) << 24;
        *reinterpret_cast<uint2 *>(dst) = v;
    }
}

__global__ __launch_bounds__(kB) void jpeg_base_pixels_k(BaseArgs a) {
    const int64_t hw = (int64_t)a.h * a.w, id = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (id >= hw * a.n_streams) return;
    const int s = (int)(id / hw);
    const int64_t r = id % hw;
    uint8_t *out = a.images + (((int64_t)(s / a.views) * hw + r) * a.views + s % a.views) * 3;
    uint8_t rgb[3] = {0, 0, 0};
    if (a.status[s] == ST_OK) {
        const int sampling = (int)a.desc[s].sampling;
        pixel_rgb_scan(a.planes + (size_t)s * a.cap * 64, geo_of(a.h, a.w, sampling), sampling, a.h, a.w, (int)(r / a.w), (int)(r % a.w), rgb);
    }
    out[0] = rgb[0];
    out[1] = rgb[1];
    out[2] = rgb[2];
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// the sizes the call may take, and B = n_streams * blocks_cap
bool shape_ok(int n_streams, int h, int w, int64_t *total_blocks) {
    if (!sides_ok(h, w) || n_streams < 0) return false;
    *total_blocks = (int64_t)n_streams * blocks_cap(h, w);
    return *total_blocks < ((int64_t)1 << 31);
}

int entropy_lanes() {
    const char *e = getenv("SRLHIP_JPEG_BASELINE_LANES");
    const int v = e ? atoi(e) : 0;
    return v == 64 || v == 16 || v == 4 ? v : kEntropyLanes;
}

}  // namespace

extern "C" {

size_t srlhip_jpeg_decode_baseline_workspace_bytes(int32_t n_streams, int32_t img_h, int32_t img_w) {
    int64_t B;
    if (!shape_ok(n_streams, img_h, img_w, &B)) return 0;
    return align256(sizeof(Desc) * (size_t)n_streams) + (128 + 64) * (size_t)B;
}

int srlhip_jpeg_decode_baseline(int32_t device_id, const uint8_t *blob_dev, const int64_t *offsets_dev, int32_t n_streams, int32_t img_h,
                                int32_t img_w, int32_t n_channels, uint8_t *images_dev, int32_t *status_dev, void *workspace_dev,
                                void *hip_stream) {
    int64_t B;
    if (!shape_ok(n_streams, img_h, img_w, &B) || (n_channels != 3 && n_channels != 6) || n_streams % (n_channels / 3)) return SRLHIP_EINVAL;
    if (!offsets_dev || (n_streams > 0 && (!blob_dev || !images_dev || !status_dev || !workspace_dev))) return SRLHIP_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 16) return SRLHIP_EINVAL;
    if (n_streams == 0) return SRLHIP_OK;
    if (hipSetDevice(device_id) != hipSuccess) return SRLHIP_EHIP;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    BaseArgs a;
    a.blob = blob_dev; a.offsets = offsets_dev; a.images = images_dev; a.status = status_dev;
    a.desc = reinterpret_cast<Desc *>(ws);
    a.coef = reinterpret_cast<int16_t *>(ws + align256(sizeof(Desc) * (size_t)n_streams));
    a.planes = ws + align256(sizeof(Desc) * (size_t)n_streams) + 128 * (size_t)B;
    a.h = img_h; a.w = img_w; a.views = n_channels / 3; a.n_streams = n_streams;
    a.cap = blocks_cap(img_h, img_w);
    a.lanes = entropy_lanes();
    const size_t coef_words = 128 * (size_t)B / 16;
    const size_t zero_blocks = (coef_words + kB - 1) / kB;
    const int64_t pixels = (int64_t)n_streams * img_h * img_w, per_group = (int64_t)a.lanes * (kB / 64);
    hipLaunchKernelGGL(jpeg_base_zero_k, dim3((unsigned)(zero_blocks < 4096 ? zero_blocks : 4096)), dim3(kB), 0, stream, reinterpret_cast<uint4 *>(a.coef), coef_words);
    hipLaunchKernelGGL(jpeg_base_parse_k, dim3((unsigned)((n_streams + kB - 1) / kB)), dim3(kB), 0, stream, a);
    hipLaunchKernelGGL(jpeg_base_entropy_k, dim3((unsigned)((n_streams + per_group - 1) / per_group)), dim3(kB), (size_t)(192 * per_group), stream, a);
    hipLaunchKernelGGL(jpeg_base_idct_k, dim3((unsigned)((B + 31) / 32)), dim3(kB), 0, stream, a);
    hipLaunchKernelGGL(jpeg_base_pixels_k, dim3((unsigned)((pixels + kB - 1) / kB)), dim3(kB), 0, stream, a);
    return hipGetLastError() == hipSuccess ? SRLHIP_OK : SRLHIP_EHIP;
}

int srlhip_jpeg_probe_baseline(const uint8_t *stream, size_t len, int32_t *img_h, int32_t *img_w, int32_t *sampling) {
    if (!stream && len) return SRLHIP_EINVAL;
    int h = 0, w = 0, mode = 0;
    if (probe_baseline(stream, len, &h, &w, &mode) != ST_OK) return SRLHIP_ENOTSUP;
    if (img_h) *img_h = h;
    if (img_w) *img_w = w;
    if (sampling) *sampling = mode;
    return SRLHIP_OK;
}

int srlhip_jpeg_decode_baseline_host(const uint8_t *stream, size_t len, uint8_t *out, int32_t pix_stride, size_t out_cap, int32_t *status) {
    if ((!stream && len) || !out || pix_stride < 3) return SRLHIP_EINVAL;
    int h = 0, w = 0, mode = 0;
    const int st = probe_baseline(stream, len, &h, &w, &mode);
    if (st != ST_OK) {
        if (status) *status = st;
        return SRLHIP_ENOTSUP;
    }
    if (out_cap < ((size_t)h * w - 1) * (size_t)pix_stride + 3) return SRLHIP_ENOMEM;
    std::vector<uint64_t> scratch((host_scratch_bytes_baseline(h, w) + 7) / 8);
    const int r = decode_stream_baseline_host(stream, len, h, w, out, pix_stride, reinterpret_cast<uint8_t *>(scratch.data()));
    if (status) *status = r;
    return SRLHIP_OK;
}

}  // extern "C"
