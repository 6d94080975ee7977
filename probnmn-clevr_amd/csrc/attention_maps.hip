// Attention maps of the module programs for gfx950: collect the one-channel maps a batch of programs left in the
// activation arena, and paint them over the images the questions were asked about.
//
// Not in the reference: its interpreter keeps two registers and drops every intermediate output (probnmn/models/nmn.py:
// 197-238).  Here every executed module call has an arena slot of its own (host_trunk.hip: build_template), so the maps
// of `filter_*`, `relate`, `same_*`, `intersect` and `union` are still there after the forward pass;
// pnmn_trunk_last_attention says where.
//
// pnmn_attention_gather    one workgroup per map: HW floats copied out of the arena, or zeros for an offset of -1.
//
// pnmn_attention_overlay   integer arithmetic only (include/probnmn_hip.h states it; tests/helpers/overlay_reference.py is
//                          the same in numpy), so the result is the same bytes on every machine.
//   workgroup   one map x one band of 16 image rows
//   LDS         the map quantised to bytes (at most 64 x 64), the colour table as one packed word per entry, and the
//               horizontal tap of every output column (first map column | weight << 8): the two divisions per column
//               are done once per workgroup, not once per pixel; the vertical tap is wave-uniform
//   write-out   the kernel is bound by it (3 Hi Wi bytes per map).  A lane owns one ALIGNED dword of the output row, i.e.
//               the bytes of two neighbouring pixels; consecutive lanes own consecutive dwords, so a wave stores 256
//               contiguous bytes.  Only where a row does not begin or end on a dword boundary (3 Wi not a multiple of 4,
//               or an unaligned `out`) are the bytes at its ends stored one by one, by the row that owns them.
//   image       read as the bytes under each output byte; maps that share an image and are handed over next to each
//               other find it in L2 / the Infinity Cache after the first has read it.
// Every index that reaches memory is bounded: image_of is clamped to the images, taps to the map, bytes to their row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int BAND = 16;  // image rows per workgroup
constexpr int MAX_MAP = PNMN_ATTENTION_MAX_MAP * PNMN_ATTENTION_MAX_MAP;

__global__ __launch_bounds__(THREADS) void attention_gather_kernel(const float* __restrict__ act, const int64_t* __restrict__ offsets,
                                                                   float* __restrict__ out, int HW) {
    const int64_t off = offsets[blockIdx.x];
    float* dst = out + (size_t)blockIdx.x * HW;
    if (off < 0) {
        for (int i = threadIdx.x; i < HW; i += THREADS) dst[i] = 0.f;
    } else {
        const float* src = act + off;
        for (int i = threadIdx.x; i < HW; i += THREADS) dst[i] = src[i];
    }
}

struct OverlayArgs {
    const float* maps;
    const int32_t* image_of;
    const uint8_t* images;
    const uint8_t* lut;
    uint8_t* out;
    int64_t image_stride;
    int n_images, Hi, Wi, strength, H, W, bands;
};

// first map index and 8-bit weight of the second one for output index X of an axis (half-pixel centres)
__device__ __forceinline__ void axis_tap(int X, int n_in, int n_out, int& i0, int& f) {
    const int num = (2 * X + 1) * n_in - n_out, den = 2 * n_out;
    if (num < 0) {
        i0 = 0, f = 0;
    } else {
        i0 = num / den;
        f = ((num - i0 * den) * 256) / den;
    }
    i0 = min(i0, n_in - 1);
}

__global__ __launch_bounds__(THREADS) void attention_overlay_kernel(const OverlayArgs a) {
    __shared__ uint32_t lut[256];       // r | g << 8 | b << 16
    __shared__ uint8_t q[MAX_MAP];      // the quantised map
    extern __shared__ __attribute__((aligned(16))) uint16_t xtap[];  // [Wi]: i0 | fx << 8

    const int tid = threadIdx.x;
    const int item = blockIdx.x / a.bands, Y0 = (blockIdx.x - item * a.bands) * BAND;
    const int Y1 = min(Y0 + BAND, a.Hi);
    const int H = a.H, W = a.W, Wi = a.Wi;

    const float* map = a.maps + (size_t)item * H * W;
    for (int i = tid; i < H * W; i += THREADS) {
        const float v = fminf(fmaxf(map[i], 0.f), 1.f);  // (fmaxf returns the other operand for a NaN)
        q[i] = (uint8_t)(int)fmaf(v, 255.0f, 0.5f);
    }
    for (int i = tid; i < 256; i += THREADS)
        lut[i] = (uint32_t)a.lut[3 * i] | (uint32_t)a.lut[3 * i + 1] << 8 | (uint32_t)a.lut[3 * i + 2] << 16;
    for (int X = tid; X < Wi; X += THREADS) {
        int i0, f;
        axis_tap(X, W, Wi, i0, f);
        xtap[X] = (uint16_t)(i0 | f << 8);
    }
    __syncthreads();

    const int image = min(max(a.image_of[item], 0), a.n_images - 1);
    const uint8_t* img = a.images + (size_t)image * (size_t)a.image_stride;
    const int row_bytes = 3 * Wi;
    const int strength = a.strength;

    for (int Y = Y0; Y < Y1; ++Y) {  // (wave-uniform: the vertical tap costs scalar instructions)
        int y0, fy;
        axis_tap(Y, H, a.Hi, y0, fy);
        const uint8_t* q0 = q + y0 * W;
        const uint8_t* q1 = q + min(y0 + 1, H - 1) * W;
        auto value = [&](int X) {
            const int t = xtap[X], x0 = t & 255, fx = t >> 8, x1 = min(x0 + 1, W - 1);
            const int top = q0[x0] * (256 - fx) + q0[x1] * fx, bottom = q1[x0] * (256 - fx) + q1[x1] * fx;
            return (top * (256 - fy) + bottom * fy + 32768) >> 16;
        };
        const uint8_t* src = img + (size_t)Y * row_bytes;
        uint8_t* dst = a.out + ((size_t)item * a.Hi + Y) * (size_t)row_bytes;
        const int lead = (int)(reinterpret_cast<uintptr_t>(dst) & 3);  // bytes of the first dword that belong to the row before
        const int n_dwords = (lead + row_bytes + 3) >> 2;
        for (int d = tid; d < n_dwords; d += THREADS) {
            const int k0 = 4 * d - lead;                   // row byte of this dword's byte 0 (negative: before the row)
            const int xa = max(k0, 0) / 3, xb = min(xa + 1, Wi - 1);  // the two pixels the dword's bytes belong to
            const int va = value(xa), vb = value(xb);
            const int wa = (va * strength + 127) / 255, wb = (vb * strength + 127) / 255;
            const uint32_t ca = lut[va], cb = lut[vb];
            uint32_t word = 0;
            bool whole = true;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = k0 + b;
                if (k < 0 || k >= row_bytes) {
                    whole = false;
                    continue;
                }
                const int x = k / 3, c = k - 3 * x;
                const bool second = x != xa;
                const int w = second ? wb : wa;
                const int colour = ((second ? cb : ca) >> (8 * c)) & 255;
                word |= (uint32_t)((src[k] * (255 - w) + colour * w + 127) / 255) << (8 * b);
            }
            if (whole) {
                *reinterpret_cast<uint32_t*>(dst + k0) = word;
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (k0 + b >= 0 && k0 + b < row_bytes) dst[k0 + b] = (uint8_t)(word >> (8 * b));
            }
        }
    }
}

}  // namespace

extern "C" int pnmn_attention_gather(const float* act, const int64_t* offsets, float* out, int n, int HW, void* stream) {
    if (!act || !offsets || !out || HW <= 0 || n < 0) return PNMN_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(attention_gather_kernel, dim3((unsigned)n), dim3(THREADS), 0, static_cast<hipStream_t>(stream), act,
                       offsets, out, HW);
    return (int)hipGetLastError();
}

extern "C" int pnmn_attention_overlay(const float* maps, const int32_t* image_of, const uint8_t* images, int64_t image_stride,
                                      int n_images, int Hi, int Wi, const uint8_t* lut, int strength, uint8_t* out, int n, int H,
                                      int W, void* stream) {
    if (!maps || !image_of || !images || !lut || !out) return PNMN_EINVAL;
    if (n < 0 || n_images < 1 || H < 1 || W < 1 || H > PNMN_ATTENTION_MAX_MAP || W > PNMN_ATTENTION_MAX_MAP || Hi < 1 || Wi < 1 ||
        Hi > PNMN_ATTENTION_MAX_IMAGE || Wi > PNMN_ATTENTION_MAX_IMAGE || strength < 0 || strength > 255)
        return PNMN_EINVAL;
    if (image_stride < (int64_t)3 * Hi * Wi) return PNMN_EINVAL;
    if (n == 0) return 0;
    const int bands = (Hi + BAND - 1) / BAND;
    if ((int64_t)bands * n > 0x7fffffffLL) return PNMN_EINVAL;
    OverlayArgs a{maps, image_of, images, lut, out, image_stride, n_images, Hi, Wi, strength, H, W, bands};
    const size_t lds = (size_t)Wi * sizeof(uint16_t);  // at most 32 KB beside the 5 KB of static LDS
    hipLaunchKernelGGL(attention_overlay_kernel, dim3((unsigned)(bands * n)), dim3(THREADS), lds,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
