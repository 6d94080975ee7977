// LSTM dropout between an encoder's layers as a kernel of its own (include/probnmn_hip.h: pnmn_lstm_dropout): the eager
// path's mask between the persistent layer launches, the launch plan's between layer 1 and the input-projection GEMM of
// layer 2 where the wavefront launch does not serve the batch, and -- the same call on the gradient -- backward.
// Bandwidth-bound: one 16-byte load and store per thread and step of the grid-stride loop, four keep bits from Philox.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <stdint.h>

#include "../../include/probnmn_hip.h"
#include "dropout.h"

namespace {

typedef float f32x4_ __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void lstm_dropout_kernel(const float* x, float* y, int64_t n4, int T,
                                                           int H4, float keep_below, float scale, uint64_t seed, int64_t row_offset) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rt = i / H4;  // row * T + t
        const uint32_t u = (uint32_t)(i - rt * H4) * 4u, t = (uint32_t)(rt % T);
        const uint64_t row = (uint64_t)(row_offset + rt / T);
        const f32x4_ v = reinterpret_cast<const f32x4_*>(x)[i];
        f32x4_ o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = pnmn::dropout_apply(v[k], pnmn::dropout_keep(seed, row, t, u + k, keep_below), scale);
        reinterpret_cast<f32x4_*>(y)[i] = o;
    }
}

}  // namespace

extern "C" int pnmn_lstm_dropout(const float* x, float* y, int rows, int T, int H, float p, uint64_t seed, int64_t row_offset,
                                 void* stream) {
    if (rows < 0 || T < 0 || H < 0 || !(p >= 0.f && p <= 1.f) || row_offset < 0) return PNMN_EINVAL;
    if (rows == 0 || T == 0 || H == 0) return 0;
    if (!x || !y) return PNMN_EINVAL;
    if (H % 4 || (((uintptr_t)x | (uintptr_t)y) & 15)) return PNMN_ESHAPE;
    // (x == y is allowed: every element is read and written by the same thread)
    const float keep_below = 1.0f - p, scale = 1.0f / keep_below;
    const int64_t n4 = (int64_t)rows * T * (H / 4);
    const int64_t blocks = std::min<int64_t>((n4 + 255) / 256, 4096);
    hipLaunchKernelGGL(lstm_dropout_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n4, T, H / 4,
                       keep_below, scale, seed, row_offset);
    return (int)hipGetLastError();
}
