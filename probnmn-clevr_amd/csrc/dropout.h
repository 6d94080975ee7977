// The keep bit of LSTM dropout between an encoder's layers (include/probnmn_hip.h, pnmn_lstm_dropout): Philox4x32-10 (the
// generator of sampling.h) under key = the pass's seed with counter {row lo, row hi, step, unit}; output word 0 gives
// u = (x0 >> 8) * 2^-24 and the element is kept iff u < 1 - p (fp32).  A kept element is scaled by 1 / (1 - p).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sampling.h"

namespace pnmn {

__device__ __forceinline__ bool dropout_keep(uint64_t seed, uint64_t row, uint32_t t, uint32_t u, float keep_below) {
    uint32_t ctr[4] = {(uint32_t)row, (uint32_t)(row >> 32), t, u};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(ctr, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (float)(ctr[0] >> 8) * (1.0f / 16777216.0f) < keep_below;
}

// y = x * keep * scale as one product: x * scale where kept, x * 0 (a signed zero) where dropped -- also for p = 1, whose
// scale is +inf and which keeps nothing
__device__ __forceinline__ float dropout_apply(float x, bool keep, float scale) { return x * (keep ? scale : 0.f); }

}  // namespace pnmn
