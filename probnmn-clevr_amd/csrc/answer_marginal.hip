// The marginal answer over several programs for gfx950: p(a | x, image) = sum_z q(z | x) p(a | z, image), from the answer
// logits of every hypothesis row and the (unnormalised) log-weight of each.
//
// Not in the reference: it answers from ONE program (probnmn/models/nmn.py:245-269 takes the arg-max of one row of logits,
// scripts/inference.py:76-91 feeds it one sampled program per question).  include/probnmn_hip.h states the contract;
// tests/helpers/answer_marginal_reference.py is the same in fp64 numpy.
//
//   workgroup   256 threads = four wavefronts, one GROUP (one question's hypotheses) per wavefront; a wavefront never
//               looks at another group's rows, waits for nothing and uses no LDS and no atomics, so a group's outputs
//               are the same bits alone or inside a batch, and every loop is bounded by the clamped group bounds
//   lanes       run over the answers: lane l holds columns l, l + 64, ... (NPER = ceil(A / 64) registers per row), so a
//               row read is one coalesced segment and the per-answer accumulators never leave their lane
//   sweep 1     over the group's rows, 64 at a time: which are usable, the largest log-weight, then the sum of
//               exp(log-weight - largest): log w_r = (lw_r - largest) - log(sum), every term rounded at its own size
//   sweep 2     one row at a time (the next row's logits are loaded before this one's are reduced): row maximum and its
//               first position, log-sum-exp, then x = log w_r + (z - max) - log(sum exp) folded into a running
//               (maximum, sum) per answer column; log_marginal = maximum + log(sum)
// Wave reductions are xor butterflies: every lane ends with the same bits, in an order that depends on nothing but the lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int GROUPS_PER_BLOCK = THREADS / WAVE;
constexpr int MAX_ANSWERS = 1024;  // NPER <= 16 registers per row and lane

struct MarginalArgs {
    const float* logits;
    const int32_t* valid;
    const float* log_weight;
    const int32_t* group_start;
    float* log_marginal;
    int64_t* predictions;
    int64_t* row_predictions;
    float* row_weight;
    int32_t* support;
    int n_groups, n_rows, A, unknown_index;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v = fmaxf(v, __shfl_xor(v, d, WAVE));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// the largest value and the lowest index that holds it (the first maximum), in every lane
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const float ov = __shfl_xor(v, d, WAVE);
        const int oi = __shfl_xor(i, d, WAVE);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ bool finite(float x) { return fabsf(x) < INFINITY; }  // (false for a NaN)

template <int NPER>
__device__ __forceinline__ void load_row(const float* __restrict__ logits, int r, int A, int lane, float (&z)[NPER]) {
    const float* row = logits + (size_t)r * A;
#pragma unroll
    for (int k = 0; k < NPER; ++k) {
        const int a = lane + WAVE * k;
        z[k] = a < A ? row[a] : -INFINITY;
    }
}

template <int NPER>
__global__ __launch_bounds__(THREADS) void answer_marginal_kernel(const MarginalArgs p) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int g = blockIdx.x * GROUPS_PER_BLOCK + (threadIdx.x >> 6);  // wave-uniform
    if (g >= p.n_groups) return;
    const int A = p.A;
    // the group's rows, clamped into the arrays whatever group_start says
    const int start = min(max(p.group_start[g], 0), p.n_rows);
    const int end = max(min(max(p.group_start[g + 1], 0), p.n_rows), start);

    auto usable = [&](int r) {
        return (p.valid == nullptr || p.valid[r] != 0) && (p.log_weight == nullptr || finite(p.log_weight[r]));
    };

    // ---- sweep 1: the support and the normaliser of the weights ----
    int count = 0;
    float lw_max = -INFINITY;
    for (int r = start + lane; r < end; r += WAVE)
        if (usable(r)) {
            ++count;
            lw_max = fmaxf(lw_max, p.log_weight ? p.log_weight[r] : 0.f);
        }
    count = wave_sum(count);
    lw_max = wave_max(lw_max);
    float log_norm = 0.f;
    if (count > 0) {
        if (p.log_weight) {
            float se = 0.f;
            for (int r = start + lane; r < end; r += WAVE)
                if (usable(r)) se += expf(p.log_weight[r] - lw_max);
            log_norm = logf(wave_sum(se));
        } else {
            log_norm = logf((float)count);
        }
    }
    const float uniform = count > 0 ? 1.0f / (float)count : 0.f;

    // ---- sweep 2: fold every usable row into the running (maximum, sum) of each answer column ----
    float m[NPER], s[NPER], z[NPER], nxt[NPER];
#pragma unroll
    for (int k = 0; k < NPER; ++k) m[k] = -INFINITY, s[k] = 0.f, nxt[k] = -INFINITY;
    if (start < end) load_row<NPER>(p.logits, start, A, lane, nxt);
    for (int r = start; r < end; ++r) {
#pragma unroll
        for (int k = 0; k < NPER; ++k) z[k] = nxt[k];
        if (r + 1 < end) load_row<NPER>(p.logits, r + 1, A, lane, nxt);

        float best = z[0];
        int at = lane;
#pragma unroll
        for (int k = 1; k < NPER; ++k)
            if (z[k] > best) best = z[k], at = lane + WAVE * k;  // (columns grow with k: the lane's first maximum)
        wave_argmax(best, at);
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < NPER; ++k) se += expf(z[k] - best);  // (columns beyond A hold -inf: exp gives 0)
        const float log_z = logf(wave_sum(se));

        const bool row_valid = p.valid == nullptr || p.valid[r] != 0;
        const float lw = p.log_weight ? p.log_weight[r] : 0.f;
        const bool use = row_valid && finite(lw);
        const float log_w = (lw - lw_max) - log_norm;
        if (lane == 0) {
            if (p.row_predictions) p.row_predictions[r] = row_valid ? (int64_t)at : (int64_t)p.unknown_index;
            if (p.row_weight) p.row_weight[r] = !use ? 0.f : p.log_weight ? expf(log_w) : uniform;
        }
        if (use) {
#pragma unroll
            for (int k = 0; k < NPER; ++k) {
                const float x = log_w + ((z[k] - best) - log_z);
                if (x > m[k]) {
                    s[k] = s[k] * expf(m[k] - x) + 1.f;
                    m[k] = x;
                } else {
                    s[k] += expf(x - m[k]);
                }
            }
        }
    }

    // ---- the group's outputs ----
    float top = -INFINITY;
    int at = 0x7fffffff;
    float* out = p.log_marginal + (size_t)g * A;
#pragma unroll
    for (int k = 0; k < NPER; ++k) {
        const int a = lane + WAVE * k;
        if (a < A) {
            const float v = count > 0 ? m[k] + logf(s[k]) : -INFINITY;
            out[a] = v;
            if (v > top || at == 0x7fffffff) top = v, at = a;  // (the lane's first maximum, -inf included)
        }
    }
    wave_argmax(top, at);  // (of the values as stored; a lane without a column holds (-inf, int max) and never wins a tie)
    if (lane == 0) {
        p.predictions[g] = count > 0 ? (int64_t)at : (int64_t)p.unknown_index;
        if (p.support) p.support[g] = count;
    }
}

template <int NPER>
int launch(const MarginalArgs& a, void* stream) {
    const unsigned blocks = (unsigned)(((int64_t)a.n_groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK);
    hipLaunchKernelGGL(answer_marginal_kernel<NPER>, dim3(blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pnmn_answer_marginal(const float* logits, const int32_t* valid, const float* log_weight, const int32_t* group_start,
                                    float* log_marginal, int64_t* predictions, int64_t* row_predictions, float* row_weight,
                                    int32_t* support, int n_groups, int n_rows, int num_answers, int unknown_index, void* stream) {
    if (n_groups < 0 || n_rows < 0 || num_answers < 1) return PNMN_EINVAL;
    if (n_groups == 0) return 0;  // (nothing to read or to write)
    if (!group_start || !log_marginal || !predictions || (n_rows > 0 && !logits)) return PNMN_EINVAL;
    if (num_answers > MAX_ANSWERS) return PNMN_ESHAPE;
    const MarginalArgs a{logits, valid, log_weight, group_start, log_marginal, predictions, row_predictions, row_weight, support,
                         n_groups, n_rows, num_answers, unknown_index};
    const int nper = (num_answers + WAVE - 1) / WAVE;
    if (nper <= 1) return launch<1>(a, stream);
    if (nper <= 2) return launch<2>(a, stream);
    if (nper <= 4) return launch<4>(a, stream);
    if (nper <= 8) return launch<8>(a, stream);
    return launch<16>(a, stream);
}
