// Launch shapes of the point-wise kernels (host side): how a layout change, a max-pool and the deferred feature-gradient
// gather are cut into workgroups.  Pure functions, no HIP: pointwise.hip launches by them, and
// tests/test_pointwise_reference.py compiles this header on its own to hold its restatement against them.
#pragma once
#include <stddef.h>

namespace pnmn {

// pixels per workgroup of the layout kernels: the whole map when 64 channels of it fit the LDS
// budget (14x14), otherwise the smallest number of equal chunks that do (28x28: two of 392)
inline int layout_chunk(int HW) {
    int parts = 1;
    while ((size_t)64 * ((HW + parts - 1) / parts + 1) * sizeof(float) > 112 * 1024) ++parts;
    return (HW + parts - 1) / parts;
}

// image rows per workgroup of the generic max-pool kernels (even; [rows*W][65] floats within the LDS budget)
inline int pool_band(int H, int W) {
    int rb = (H + 1) & ~1;
    while (rb > 2 && (size_t)rb * W * 65 * sizeof(float) > 112 * 1024) rb = ((rb / 2) + 1) & ~1;
    return rb;
}

// pooled rows per workgroup of the even-map max-pool backward (14x14: all 7, 28x28: two bands of 7; never more than the
// map has), and the LDS its band of pooled gradients takes: [rows * (W/2)][65] floats
inline int pool_bwd_even_rows(int H, int W) {
    const int PH = H / 2, PW = W / 2;
    if (PH * PW <= 64) return PH;
    return PH < 7 ? PH : 7;
}
inline size_t pool_bwd_even_lds(int H, int W) { return (size_t)pool_bwd_even_rows(H, W) * (W / 2) * 65 * sizeof(float); }
// The even kernel asks for no LDS opt-in: it runs the even maps whose band fits the 64 KB every launch gets, the generic
// kernel (banded by pool_band) every other shape -- so the backward accepts what the forward accepts.
inline bool pool_bwd_takes_even(int H, int W) {
    return (H % 2) == 0 && (W % 2) == 0 && pool_bwd_even_lds(H, W) <= 64 * 1024;
}

// pixel ranges per example of the feature-gradient gather: enough workgroups to fill the chip at small batches, ranges
// of >= 24 pixels
inline int gather_parts(int n_examples, int HW) {
    int parts = 1;
    while (n_examples * parts < 512 && parts < 8 && HW / (parts * 2) >= 24) parts *= 2;
    return parts;
}

// tiles of 32 x 32 a weight [cout][ntaps][cin] is transposed in; a workgroup walks them with the stride of the grid
inline int wtrans_tiles(int cout, int cin, int ntaps) { return ((cin + 31) / 32) * ((cout + 31) / 32) * ntaps; }
constexpr int WTRANS_GRID = 256;

}  // namespace pnmn
