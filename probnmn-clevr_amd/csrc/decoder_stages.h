// Matrix-core stages that the one-workgroup decoder kernels share (decoder.hip: attn_lstm_fwd_kernel; decoder_beam.hip):
// the attention weights of one row, the gate product of one step and the logits tile of one wave.  512 threads = 8 waves own a 16-row tile; the row
// operands come from LDS rows of LD floats, the weights of the gates in fragment order (seq2seq.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "recurrent_tile.h"
#include "sampling.h"

namespace pnmn {

// AllenNLP's masked_softmax over the S <= 64 encoder positions of one row, lane = position: softmax(score * mask) * mask,
// renormalised with 1e-13.  Returns the attention weight of this lane's position; `p` = the softmax before masking.
__device__ __forceinline__ float attention_weight(float score, float m, int S, int lane, float& p) {
    const float v = score * m;  // allennlp masked_softmax: softmax(vector * mask) ...
    const float mx = wmax(lane < S ? v : -INFINITY);
    const float ex = lane < S ? expf(v - mx) : 0.f;
    p = ex / wsum(ex);
    const float q = p * m;        // ... * mask, renormalised with 1e-13
    return q / (wsum(q) + 1e-13f);
}

// acc[gate][ut] += ctx W_c^T + h W_hh^T for the 16 rows x (4 gates x 2 tiles of 16 hidden units: 32 * wave + 16 * ut + ...)
// of this wave; `ctx`, `h`: [16][LD] in LDS.
template <int H, int LD>
__device__ __forceinline__ void gates_mfma(f32x4 (&acc)[4][2], const float (*ctx)[LD], const float (*h)[LD],
                                           const float* w_c, const float* w_hh, int wave, int lane) {
    const int li = lane & 15, g = lane >> 4;
#pragma unroll 2
    for (int kb = 0; kb < H / 16; ++kb) {
        const f32x4 ac = *reinterpret_cast<const f32x4*>(&ctx[li][kb * 16 + 4 * g]);
        const f32x4 ah = *reinterpret_cast<const f32x4*>(&h[li][kb * 16 + 4 * g]);
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int ut = 0; ut < 2; ++ut) {
                const size_t fo = ((size_t)((gate * (H / 16) + 2 * wave + ut) * (H / 16) + kb) * 64 + lane) * 4;
                const f32x4 bc = *reinterpret_cast<const f32x4*>(w_c + fo);  // weights are packed in
                const f32x4 bh = *reinterpret_cast<const f32x4*>(w_hh + fo);  // fragment order (seq2seq.hip)
                acc[gate][ut] = mfma4(ah, bh, mfma4(ac, bc, acc[gate][ut]));
            }
    }
}

// Logits of the 16 rows x vocabulary entries 16 * wave .. 16 * wave + 15 (without the bias): h [16][LD] in LDS times the
// row-major W_p [V][H] (tiny); entries at and past V read no weight.  For waves with 16 * wave < V.
template <int H, int LD>
__device__ __forceinline__ f32x4 logits_tile(const float (*h)[LD], const float* w_p, int V, int wave, int lane) {
    const int li = lane & 15, g = lane >> 4;
    f32x4 lacc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int vn = 16 * wave + li;
    const bool vok = vn < V;
#pragma unroll 4
    for (int kb = 0; kb < H / 16; ++kb) {
        const f32x4 ah = *reinterpret_cast<const f32x4*>(&h[li][kb * 16 + 4 * g]);
        f32x4 bp = f32x4{0.f, 0.f, 0.f, 0.f};
        if (vok) bp = *reinterpret_cast<const f32x4*>(w_p + (size_t)vn * H + kb * 16 + 4 * g);  // (row-major: tiny)
        lacc = mfma4(ah, bp, lacc);
    }
    return lacc;
}

}  // namespace pnmn
