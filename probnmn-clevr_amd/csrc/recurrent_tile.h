// Building blocks of the recurrent kernels (seq2seq.hip, lstm_stack.hip, decoder.hip, decoder_multi.hip, decoder_beam.hip,
// prior_sample.hip, decoder_stages.h): each exists once, here.  A workgroup of 512 threads = 8 waves owns a tile of 16
// batch rows; hidden size 256; v_mfma_f32_16x16x4_f32 with K consumed in the permuted order of the conv kernels (lane
// group g takes k = 4g .. 4g + 3 of each 16-block), so that an operand of four consecutive k is ONE 16-byte load.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace pnmn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE_ROWS = 16;         // batch rows of a tile
constexpr int TILE_H = 256;           // hidden size the recurrent kernels are built for
constexpr int TILE_LD = TILE_H + 4;   // LDS row stride (floats): 16-byte aligned, breaks the 1 KiB bank period

__device__ __forceinline__ float sigm(float z) { return 1.f / (1.f + expf(-z)); }

// acc += A B over 16 values of k: four MFMAs of K = 4, operands x, y, z, w in this order (the backward kernels pass the
// weights as A: the product comes out transposed)
__device__ __forceinline__ f32x4 mfma4(const f32x4 a, const f32x4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// Rows grouped by length (pnmn_lstm_seq_fwd_ordered / _bwd_ordered): `order` turns a tile's SLOT into the batch row it
// holds; null: slot = row.
__device__ __forceinline__ int batch_row(const int32_t* __restrict__ order, int slot) { return order ? order[slot] : slot; }

// Staging of a tile's 16 x 256 vector of one step of a [B][T][256] tensor into LDS: two 16-byte pieces per thread.
// stage_rows(): the batch rows of this thread's two pieces (rows past the batch re-read the last one), looked up once
// per launch.  stage_step(): both pieces are requested before the first LDS store -- written as one loop the compiler
// issues load, vmcnt(0), store, load, vmcnt(0), store: two L2 round trips on the step's critical path.
static_assert(TILE_ROWS * TILE_H / 4 == 2 * 512, "two 16-byte pieces per thread");
__device__ __forceinline__ void stage_rows(int (&rows)[2], const int32_t* __restrict__ order, int row0, int B) {
#pragma unroll
    for (int k = 0; k < 2; ++k) rows[k] = batch_row(order, min(row0 + (int)(threadIdx.x + 512 * k) / (TILE_H / 4), B - 1));
}
__device__ __forceinline__ void stage_step(const float* src, const int (&rows)[2], int T, int t, float (*dst)[TILE_LD]) {
    f32x4 piece[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c4 = (threadIdx.x + 512 * k) % (TILE_H / 4);
        piece[k] = *reinterpret_cast<const f32x4*>(src + ((size_t)rows[k] * T + t) * TILE_H + 4 * c4);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = threadIdx.x + 512 * k, rl = i / (TILE_H / 4), c4 = i % (TILE_H / 4);
        *reinterpret_cast<f32x4*>(&dst[rl][4 * c4]) = piece[k];
    }
}

// Weights come PRE-PACKED in fragment order (the layout: seq2seq.hip):
//     packed[n_tile][k_block][lane][4],  `kblocks` k blocks per n tile
// This lane's operands of N consecutive k blocks of one n tile, from kb0 on, into registers for the whole sequence.
template <int N>
__device__ __forceinline__ void load_wslice(f32x4* w, const float* packed, int ntile, int kblocks, int kb0, int lane) {
#pragma unroll
    for (int k = 0; k < N; ++k) w[k] = *reinterpret_cast<const f32x4*>(packed + ((size_t)(ntile * kblocks + kb0 + k) * 64 + lane) * 4);
}

}  // namespace pnmn
