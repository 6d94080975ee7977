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
//   lanes       run over the answers (hypothesis_group.h: the column layout, the group bounds, the wave reductions), so a
//               row read is one coalesced segment and the per-answer accumulators never leave their lane
//   sweep 1     weight_normaliser(): the usable rows and log w_r = (lw_r - largest) - log(sum)
//   sweep 2     one row at a time (the next row's logits are loaded before this one's are reduced): row_softmax_stats(),
//               then x = log w_r + (z - max) - log(sum exp) folded into a running (maximum, sum) per answer column;
//               log_marginal = maximum + log(sum)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"
#include "hypothesis_group.h"

namespace {

using namespace pnmn::hypothesis;

constexpr int THREADS = 256;
constexpr int GROUPS_PER_BLOCK = THREADS / WAVE;

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

template <int NPER>
__global__ __launch_bounds__(THREADS) void answer_marginal_kernel(const MarginalArgs p) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int g = blockIdx.x * GROUPS_PER_BLOCK + (threadIdx.x >> 6);  // wave-uniform
    if (g >= p.n_groups) return;
    const int A = p.A;
    const Rows rows = group_rows(p.group_start, g, p.n_rows);
    const int start = rows.start, end = rows.end;

    // ---- sweep 1: the support and the normaliser of the weights ----
    const WeightNorm w = weight_normaliser(p.valid, p.log_weight, rows, lane);
    const int count = w.count;
    const float lw_max = w.lw_max, log_norm = w.log_norm;
    const float uniform = count > 0 ? 1.0f / (float)count : 0.f;

    // ---- sweep 2: fold every usable row into the running (maximum, sum) of each answer column ----
    float m[NPER], s[NPER], z[NPER], nxt[NPER];
#pragma unroll
    for (int k = 0; k < NPER; ++k) m[k] = -INFINITY, s[k] = 0.f, nxt[k] = -INFINITY;
    if (start < end) load_columns<NPER>(p.logits + (size_t)start * A, A, lane, nxt);
    for (int r = start; r < end; ++r) {
#pragma unroll
        for (int k = 0; k < NPER; ++k) z[k] = nxt[k];
        if (r + 1 < end) load_columns<NPER>(p.logits + (size_t)(r + 1) * A, A, lane, nxt);

        float best;
        int at;
        const float log_z = row_softmax_stats<NPER>(z, lane, best, at);

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

}  // namespace

extern "C" int pnmn_answer_marginal(const float* logits, const int32_t* valid, const float* log_weight, const int32_t* group_start,
                                    float* log_marginal, int64_t* predictions, int64_t* row_predictions, float* row_weight,
                                    int32_t* support, int n_groups, int n_rows, int num_answers, int unknown_index, void* stream) {
    if (n_groups < 0 || n_rows < 0 || num_answers < 1) return PNMN_EINVAL;
    if (n_groups == 0) return 0;  // (nothing to read or to write)
    if (!group_start || !log_marginal || !predictions || (n_rows > 0 && !logits)) return PNMN_EINVAL;
    if (num_answers > MAX_COLUMNS) return PNMN_ESHAPE;
    const MarginalArgs a{logits, valid, log_weight, group_start, log_marginal, predictions, row_predictions, row_weight, support,
                         n_groups, n_rows, num_answers, unknown_index};
    const unsigned blocks = (unsigned)(((int64_t)n_groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK);
    return with_nper(num_answers, [&](auto nper) {
        hipLaunchKernelGGL(answer_marginal_kernel<decltype(nper)::value>, dim3(blocks), dim3(THREADS), 0,
                           static_cast<hipStream_t>(stream), a);
        return (int)hipGetLastError();
    });
}
