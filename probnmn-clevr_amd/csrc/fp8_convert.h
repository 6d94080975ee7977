// Conversions of the 8-bit feature stores (PNMN_ELEM_F8E4M3 / PNMN_ELEM_F8E5M2), in bit arithmetic, so that the same
// lines compile for the host: there they were held against torch's Tensor.to(dtype) for every one of the 2^32 fp32
// patterns and against .float() for all 256 codes of either type, without a difference.  No 8-bit conversion
// instruction of the chip is involved, so what a code means does not depend on which flavour (OCP or fnuz) the hardware
// converts; tests/test_feature_store_fp8_gpu.py holds the kernels to torch's host conversion.
//
//   e4m3fn (OCP): 1-4-3, bias 7, no infinities, S.1111.111 is NaN, largest finite 448, smallest subnormal 2^-9
//   e5m2        : 1-5-2, bias 15, IEEE-like (infinities, NaNs), largest finite 57344, smallest subnormal 2^-16
//
// Widening is exact.  Narrowing is round to nearest even with subnormals kept; what lies beyond the largest finite
// value by half a unit of its last place or more becomes NaN (e4m3fn, which has no infinity) or infinity (e5m2).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNMN_F8_FN __host__ __device__ __forceinline__
#else
#define PNMN_F8_FN inline
#endif

namespace pnmn_f8 {

PNMN_F8_FN float from_bits(uint32_t u) { return __builtin_bit_cast(float, u); }
PNMN_F8_FN uint32_t to_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// An e5m2 code is the upper byte of a binary16.
PNMN_F8_FN float widen_e5m2(uint8_t b) { return (float)__builtin_bit_cast(_Float16, (uint16_t)((uint16_t)b << 8)); }

// An e4m3fn code below S.1111.111, its exponent and mantissa moved one place down into a binary16 (S.0eeee.mmm0000000),
// is the same number scaled by 2^-8 -- normal or subnormal alike (2^(e-15) against 2^(e-7), 2^-14 against 2^-6) -- and
// fp32 takes the 2^8 back without rounding.
// S.1111.111 itself goes in as a binary16 NaN and stays one (a select, not a branch: the gather's write-out converts
// with one wave per SIMD, where a divergent branch per element costs more than the conversion).
PNMN_F8_FN float widen_e4m3(uint8_t b) {
    const uint32_t m = b & 0x7fu;
    const uint16_t h = (uint16_t)(((b & 0x80u) << 8) | (m == 0x7fu ? 0x7e00u : m << 7));
    return (float)__builtin_bit_cast(_Float16, h) * 256.0f;
}

// fp32 -> 8 bits with E exponent and M mantissa bits (E + M = 7), exponent bias B.  `a` = |x| as bits.
//   normal results:    add half a unit of the last kept place (less one, plus the last kept bit: ties go to even) to the
//                      fp32 pattern, rebias the exponent, drop the 23 - M low bits; a carry out of the mantissa moves
//                      to the next exponent by itself, past the largest finite value into the code above it
//   subnormal results: the fp32 sum |x| + 2^(23 - M + 1 - B) is rounded to nearest even by the adder exactly at the
//                      subnormals' spacing 2^(1 - B - M); the code is that sum's distance from the constant, in units
template <int M, int B>
PNMN_F8_FN uint8_t narrow_finite(uint32_t a) {
    constexpr uint32_t drop = 23 - M;
    constexpr uint32_t smallest_normal = (uint32_t)(127 + 1 - B) << 23;
    constexpr uint32_t magic = (uint32_t)(127 + (int)drop + 1 - B) << 23;
    if (a < smallest_normal) return (uint8_t)(to_bits(from_bits(a) + from_bits(magic)) - magic);
    const uint32_t r = a + ((1u << (drop - 1)) - 1u) + ((a >> drop) & 1u);
    return (uint8_t)((r - ((uint32_t)(127 - B) << 23)) >> drop);
}

PNMN_F8_FN uint8_t narrow_e4m3(float x) {
    const uint32_t u = to_bits(x), a = u & 0x7fffffffu;
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    // 480 = 1.111 x 2^8 would be the code S.1111.111, which is NaN: everything from there on, infinities and NaNs too
    // (values in (464, 480) reach that code by the rounding's own carry)
    if (a >= 0x43f00000u) return sign | 0x7fu;
    return sign | narrow_finite<3, 7>(a);
}

PNMN_F8_FN uint8_t narrow_e5m2(float x) {
    const uint32_t u = to_bits(x), a = u & 0x7fffffffu;
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    if (a >= 0x47800000u) return sign | (a > 0x7f800000u ? 0x7fu : 0x7cu);  // 2^16 and beyond: infinity; NaN: quiet NaN
    return sign | narrow_finite<2, 15>(a);  // ([61440, 65536) carries into S.11111.00, infinity)
}

PNMN_F8_FN bool finite_e4m3(uint8_t b) { return (b & 0x7fu) != 0x7fu; }
PNMN_F8_FN bool finite_e5m2(uint8_t b) { return (b & 0x7fu) < 0x7cu; }
PNMN_F8_FN bool finite_f32(float x) { return (to_bits(x) & 0x7fffffffu) < 0x7f800000u; }

}  // namespace pnmn_f8
