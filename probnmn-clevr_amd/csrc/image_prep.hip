// Image front end of the feature extractor for gfx950: decoded uint8 images of any size -> the normalised, 4-channel
// NHWC fp32 tensor that the stem convolution (resnet.hip, Cin padded 3 -> 4) reads.
//
// The reference does this on the CPU (its scripts/preprocess/extract_features.py:60-73): PIL's
// Image.resize((224, 224), BILINEAR), then ToTensor and Normalize.  Pillow's 8-bit resampler is integer arithmetic -- per
// axis a table of 22-bit fixed-point taps, a horizontal pass rounded to uint8, then a vertical pass on that result -- so
// this kernel reproduces the reference's transform bit for bit.  The taps and their (first input index, count) bounds
// are computed by the host in double precision (probnmn.data.feature_extractor.resize_coefficients) and passed as int32
// device tables; the normalisation is a [3][256] fp32 table, so no float arithmetic happens here at all.
//
//   workgroup   one image x one band of output rows (16, or fewer when a strong downscale makes 16 rows' taps span more
//               input rows than the LDS holds)
//   pass 1      horizontal, for the input rows the band's vertical taps touch: one thread per (input row, output column),
//               byte loads from global memory (consecutive lanes read neighbouring pixels of one row), the three rounded
//               channels packed into one 32-bit word in LDS
//   pass 2      vertical, out of LDS: one thread per output pixel, one 32-bit LDS read per tap, table lookup (the table
//               is staged in LDS), one 16-byte store per lane, consecutive lanes -> consecutive pixels
//
// Every index that reaches memory is clamped: input rows and columns to the image, staged rows to the LDS buffer.  With
// tables that are not resize_coefficients' the result is meaningless but no byte outside the arguments is touched.
// Bound by HBM traffic (3 Hin Win bytes in, 16 Hout Wout bytes out per image).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int THREADS = 256;
constexpr int BAND = 16;               // output rows per workgroup, halved until the staged rows fit
constexpr int LUT_FLOATS = 3 * 256;
constexpr int LDS_BYTES = 64 * 1024;   // what a workgroup may take without opting in
constexpr int PRECISION_BITS = 22;     // Pillow's 8-bit coefficients: 32 - 8 - 2

struct PrepArgs {
    const uint8_t* images;
    const int32_t* kx;       // [Wout][ksx]
    const int32_t* xbounds;  // [Wout][2]: first input column, number of taps
    const int32_t* ky;       // [Hout][ksy]
    const int32_t* ybounds;  // [Hout][2]
    const float* lut;        // [3][256]
    float* out;              // [N][Hout][Wout][4]
    int64_t image_stride;    // bytes
    int Hin, Win, Hout, Wout, ksx, ksy, band, bands, cap_rows;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int round8(int acc) { return clampi(acc >> PRECISION_BITS, 0, 255); }

__global__ __launch_bounds__(THREADS) void image_prep_kernel(const PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float* lut = reinterpret_cast<float*>(lds);
    uint32_t* rows = reinterpret_cast<uint32_t*>(lds + LUT_FLOATS * sizeof(float));  // [cap_rows][Wout]: r | g << 8 | b << 16

    const int tid = threadIdx.x;
    const int image = blockIdx.x / a.bands, y0 = (blockIdx.x - image * a.bands) * a.band;
    if (y0 >= a.Hout) return;  // (a band past the image: the whole workgroup leaves)
    const int y1 = min(y0 + a.band, a.Hout);
    const uint8_t* img = a.images + (size_t)image * (size_t)a.image_stride;

    // the input rows this band's vertical taps touch: [r0, r0 + nrows)
    int r0 = a.Hin - 1, r1 = 0;
    for (int y = y0; y < y1; ++y) {
        const int first = clampi(a.ybounds[2 * y], 0, a.Hin), n = clampi(a.ybounds[2 * y + 1], 0, a.ksy);
        r0 = min(r0, first);
        r1 = max(r1, first + n);
    }
    r0 = clampi(r0, 0, a.Hin - 1);
    const int nrows = clampi(r1 - r0, 1, min(a.cap_rows, a.Hin - r0));

    for (int i = tid; i < LUT_FLOATS; i += THREADS) lut[i] = a.lut[i];

    // pass 1: horizontal, rounded to uint8 as Pillow's intermediate image is
    for (int i = tid; i < nrows * a.Wout; i += THREADS) {
        const int r = i / a.Wout, x = i - r * a.Wout;
        const int first = clampi(a.xbounds[2 * x], 0, a.Win), n = clampi(a.xbounds[2 * x + 1], 0, a.ksx);
        const int32_t* k = a.kx + (size_t)x * a.ksx;
        const uint8_t* row = img + (size_t)(r0 + r) * a.Win * 3;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < n; ++t) {
            const uint8_t* p = row + 3 * clampi(first + t, 0, a.Win - 1);
            const int w = k[t];
            s0 += p[0] * w;
            s1 += p[1] * w;
            s2 += p[2] * w;
        }
        rows[i] = (uint32_t)round8(s0) | (uint32_t)round8(s1) << 8 | (uint32_t)round8(s2) << 16;
    }
    __syncthreads();

    // pass 2: vertical out of LDS, normalise by table, one 16-byte pixel per lane
    float* out = a.out + ((size_t)image * a.Hout + y0) * (size_t)a.Wout * 4;
    for (int i = tid; i < (y1 - y0) * a.Wout; i += THREADS) {
        const int dy = i / a.Wout, x = i - dy * a.Wout, y = y0 + dy;
        const int first = clampi(a.ybounds[2 * y], 0, a.Hin) - r0, n = clampi(a.ybounds[2 * y + 1], 0, a.ksy);
        const int32_t* k = a.ky + (size_t)y * a.ksy;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < n; ++t) {
            const uint32_t v = rows[clampi(first + t, 0, nrows - 1) * a.Wout + x];
            const int w = k[t];
            s0 += (int)(v & 255u) * w;
            s1 += (int)((v >> 8) & 255u) * w;
            s2 += (int)((v >> 16) & 255u) * w;
        }
        const f32x4 px = {lut[round8(s0)], lut[256 + round8(s1)], lut[512 + round8(s2)], 0.f};
        *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = px;
    }
}

// Upper bound of the input rows that `band` consecutive output rows touch: the first tap of a row moves by Hin / Hout per
// output row, and a row has at most `ksy` taps (+ 1 for the truncations of the two ends).
int rows_for_band(int band, int Hin, int Hout, int ksy) {
    const int64_t travel = ((int64_t)(band - 1) * Hin + Hout - 1) / Hout;
    const int64_t rows = travel + ksy + 1;
    return (int)(rows < Hin ? rows : Hin);
}

}  // namespace

extern "C" int pnmn_image_prep(const uint8_t* images, int64_t image_stride, int N, int Hin, int Win, const int32_t* kx,
                               const int32_t* xbounds, int ksx, const int32_t* ky, const int32_t* ybounds, int ksy,
                               const float* lut, float* out, int Hout, int Wout, void* stream) {
    if (!images || !kx || !xbounds || !ky || !ybounds || !lut || !out) return PNMN_EINVAL;
    if (N < 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || ksx <= 0 || ksy <= 0) return PNMN_EINVAL;
    if (Hin > PNMN_IMAGE_PREP_MAX_SIZE || Win > PNMN_IMAGE_PREP_MAX_SIZE || Hout > PNMN_IMAGE_PREP_MAX_SIZE ||
        Wout > PNMN_IMAGE_PREP_MAX_WIDTH || ksx > PNMN_IMAGE_PREP_MAX_TAPS || ksy > PNMN_IMAGE_PREP_MAX_TAPS)
        return PNMN_EINVAL;
    if (image_stride < (int64_t)3 * Hin * Win) return PNMN_EINVAL;
    if (N == 0) return 0;
    int band = BAND, cap_rows = rows_for_band(band, Hin, Hout, ksy);
    const int64_t budget = (LDS_BYTES - LUT_FLOATS * (int)sizeof(float)) / (int)sizeof(uint32_t);
    while (band > 1 && (int64_t)cap_rows * Wout > budget) {
        band /= 2;
        cap_rows = rows_for_band(band, Hin, Hout, ksy);
    }
    if ((int64_t)cap_rows * Wout > budget) return PNMN_EINVAL;  // (not reached within the limits above: 34 x 448 words fit)
    const int bands = (Hout + band - 1) / band;
    if ((int64_t)bands * N > 0x7fffffffLL) return PNMN_EINVAL;
    PrepArgs a{images, kx, xbounds, ky, ybounds, lut, out, image_stride, Hin, Win, Hout, Wout, ksx, ksy, band, bands, cap_rows};
    const size_t lds = LUT_FLOATS * sizeof(float) + (size_t)cap_rows * Wout * sizeof(uint32_t);
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)(bands * N)), dim3(THREADS), lds,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
