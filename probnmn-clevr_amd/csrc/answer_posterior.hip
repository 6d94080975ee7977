// The posterior over a question's program hypotheses GIVEN ITS ANSWER, for gfx950:
//     p(z_r | x, a, image) ~ w_r  p(a | z_r, image)^w_a      over the rows r of the question's group
// from the answer logits of every hypothesis row, the given answer of each question and the (unnormalised) log-weight a row
// has before the answer is seen (log q(z | x), or the log-posterior under p(x | z) p(z)): per row log p(a | z_r, image) and
// the row's own answer, per group the normalised log-posterior, the log-evidence log p(a | x, image), the MAP row and the
// rows whose own answer is the given one.
//
// Not in the reference: it uses p(a | z, image) to answer from ONE sampled program (probnmn/models/nmn.py:245-269,
// scripts/inference.py:76-91) and never to judge the program.  include/probnmn_hip.h states the contract;
// tests/helpers/answer_posterior_reference.py is the same in fp64 numpy.
//
//   workgroup   64 threads = ONE wavefront = one GROUP (one question's hypotheses): it never looks at another group's rows,
//               waits for no other workgroup and uses no LDS and no atomics, so a group's outputs are the same bits alone or
//               inside a batch, and every loop is bounded by the clamped group bounds.  (The work is latency -- a row is a
//               chain of dependent wave reductions --, so the groups are spread over as many CUs as there are.)
//   lanes       run over the answers: lane l holds columns l, l + 64, ... (NPER = ceil(A / 64) registers per row), so a
//               row read is one coalesced segment
//   sweep 1     over the group's rows, 64 at a time: which are base-usable, the largest log-weight, then the sum of
//               exp(log-weight - largest): log w_r = (lw_r - largest) - log(sum), every term rounded at its own size
//   sweep 2     one row at a time (the next row's logits, validity and weight are loaded before this one's are reduced):
//               row maximum and its first position, log-sum-exp, the logit of the given answer (held by one lane, read
//               with a readlane), the score; every value is wave-uniform, so the support, the largest score and its first
//               row and the consistent rows are counted in scalars; lane 0 writes score[r] (-inf for a row that is not
//               usable) into log_posterior[r]
//   sweep 3     ONE __syncthreads() (the scores lane 0 stored are visible to the other lanes), then over the slots the scores
//               were in, 64 at a time: the sum of exp(score - largest), and log_posterior[r] = (score[r] - largest) - log(sum)
// Wave reductions are xor butterflies: every lane ends with the same bits, in an order that depends on nothing but the lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"

namespace {

constexpr int WAVE = 64;
constexpr int THREADS = WAVE;
constexpr int MAX_ANSWERS = 1024;  // NPER <= 16 registers per row and lane

struct AnswerPosteriorArgs {
    const float* logits;
    const int32_t* valid;
    const float* log_weight;
    const int64_t* answers;
    const int32_t* group_start;
    float w_a;
    float* log_answer;
    int64_t* row_predictions;
    float* log_posterior;
    float* log_evidence;
    int32_t* best_row;
    int32_t* support;
    int32_t* consistent_count;
    int32_t* first_consistent;
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
__global__ __launch_bounds__(THREADS) void answer_posterior_kernel(const AnswerPosteriorArgs p) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    const int A = p.A;
    // the group's rows, clamped into the arrays whatever group_start says
    const int start = min(max(p.group_start[g], 0), p.n_rows);
    const int end = max(min(max(p.group_start[g + 1], 0), p.n_rows), start);
    // the given answer: never an index unless it is one (wave-uniform)
    const int64_t answer = p.answers[g];
    const bool answer_known = answer >= 0 && answer < (int64_t)A;
    const int answer_at = __builtin_amdgcn_readfirstlane(answer_known ? (int)answer : 0);

    auto base_usable = [&](int r) {
        return (p.valid == nullptr || p.valid[r] != 0) && (p.log_weight == nullptr || finite(p.log_weight[r]));
    };

    // ---- sweep 1: the base-usable rows and the normaliser of their weights ----
    int base = 0;
    float lw_max = -INFINITY;
    for (int r = start + lane; r < end; r += WAVE)
        if (base_usable(r)) {
            ++base;
            lw_max = fmaxf(lw_max, p.log_weight ? p.log_weight[r] : 0.f);
        }
    base = wave_sum(base);
    lw_max = wave_max(lw_max);
    float log_norm_w = 0.f;
    if (base > 0) {
        if (p.log_weight) {
            float se = 0.f;
            for (int r = start + lane; r < end; r += WAVE)
                if (base_usable(r)) se += expf(p.log_weight[r] - lw_max);
            log_norm_w = logf(wave_sum(se));
        } else {
            log_norm_w = logf((float)base);
        }
    }

    // ---- sweep 2: every row's answer likelihood, own answer and score; the group's counts and its largest score ----
    int count = 0, consistent = 0, first_consistent = -1, best = -1;
    float top = -INFINITY;
    float z[NPER], nxt[NPER];
#pragma unroll
    for (int k = 0; k < NPER; ++k) nxt[k] = -INFINITY;
    int valid_nxt = 1;
    float lw_nxt = 0.f;
    if (start < end) {
        load_row<NPER>(p.logits, start, A, lane, nxt);
        if (p.valid) valid_nxt = p.valid[start];
        if (p.log_weight) lw_nxt = p.log_weight[start];
    }
    for (int r = start; r < end; ++r) {
#pragma unroll
        for (int k = 0; k < NPER; ++k) z[k] = nxt[k];
        const bool row_valid = valid_nxt != 0;
        const float lw = lw_nxt;
        if (r + 1 < end) {
            load_row<NPER>(p.logits, r + 1, A, lane, nxt);
            if (p.valid) valid_nxt = p.valid[r + 1];
            if (p.log_weight) lw_nxt = p.log_weight[r + 1];
        }

        float row_max = z[0];
        int at = lane;
#pragma unroll
        for (int k = 1; k < NPER; ++k)
            if (z[k] > row_max) row_max = z[k], at = lane + WAVE * k;  // (columns grow with k: the lane's first maximum)
        wave_argmax(row_max, at);
        float se = 0.f, held = 0.f;
#pragma unroll
        for (int k = 0; k < NPER; ++k) {
            se += expf(z[k] - row_max);  // (columns beyond A hold -inf: exp gives 0)
            if (k == (answer_at >> 6)) held = z[k];
        }
        const float log_z = logf(wave_sum(se));
        const float target = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(held), answer_at & (WAVE - 1)));
        const float log_answer = answer_known ? (target - row_max) - log_z : -INFINITY;

        const bool use_base = row_valid && finite(lw);
        float score = (lw - lw_max) - log_norm_w;
        if (p.w_a != 0.f) score += p.w_a * log_answer;  // (w_a == 0: the term is left out, no 0 * -inf)
        const bool use = use_base && finite(score);
        const int64_t prediction = row_valid ? (int64_t)at : (int64_t)p.unknown_index;
        if (use) {
            ++count;
            if (score > top || best < 0) top = score, best = r;  // (rows grow: the first maximum)
            if (prediction == answer) {
                ++consistent;
                if (first_consistent < 0) first_consistent = r;
            }
        }
        if (lane == 0) {
            if (p.log_answer) p.log_answer[r] = log_answer;
            if (p.row_predictions) p.row_predictions[r] = prediction;
            p.log_posterior[r] = use ? score : -INFINITY;
        }
    }
    __syncthreads();  // (workgroup scope: the scores lane 0 stored are visible to every lane of the wave)

    // ---- sweep 3: the normaliser of the scores, and the posterior over the slots the scores were in ----
    float log_norm = 0.f;
    if (count > 0) {
        float se = 0.f;
        for (int r = start + lane; r < end; r += WAVE) {
            const float s = p.log_posterior[r];
            if (finite(s)) se += expf(s - top);
        }
        log_norm = logf(wave_sum(se));
    }
    for (int r = start + lane; r < end; r += WAVE) {
        const float s = p.log_posterior[r];
        p.log_posterior[r] = finite(s) ? (s - top) - log_norm : -INFINITY;
    }
    if (lane == 0) {
        p.log_evidence[g] = count > 0 ? top + log_norm : -INFINITY;
        p.best_row[g] = count > 0 ? best : -1;
        if (p.support) p.support[g] = count;
        if (p.consistent_count) p.consistent_count[g] = consistent;
        if (p.first_consistent) p.first_consistent[g] = first_consistent;
    }
}

template <int NPER>
int launch(const AnswerPosteriorArgs& a, void* stream) {
    hipLaunchKernelGGL(answer_posterior_kernel<NPER>, dim3((unsigned)a.n_groups), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pnmn_answer_posterior(const float* logits, const int32_t* valid, const float* log_weight, const int64_t* answers,
                                     const int32_t* group_start, float w_a, float* log_answer, int64_t* row_predictions,
                                     float* log_posterior, float* log_evidence, int32_t* best_row, int32_t* support,
                                     int32_t* consistent_count, int32_t* first_consistent, int n_groups, int n_rows,
                                     int num_answers, int unknown_index, void* stream) {
    if (n_groups < 0 || n_rows < 0 || num_answers < 1) return PNMN_EINVAL;
    if (n_groups == 0) return 0;  // (nothing to read or to write)
    if (!group_start || !answers || !log_posterior || !log_evidence || !best_row || (n_rows > 0 && !logits)) return PNMN_EINVAL;
    if (!(fabsf(w_a) < INFINITY)) return PNMN_EINVAL;
    if (num_answers > MAX_ANSWERS) return PNMN_ESHAPE;
    const AnswerPosteriorArgs a{logits, valid, log_weight, answers, group_start, w_a, log_answer, row_predictions, log_posterior,
                                log_evidence, best_row, support, consistent_count, first_consistent, n_groups, n_rows, num_answers,
                                unknown_index};
    const int nper = (num_answers + WAVE - 1) / WAVE;
    if (nper <= 1) return launch<1>(a, stream);
    if (nper <= 2) return launch<2>(a, stream);
    if (nper <= 4) return launch<4>(a, stream);
    if (nper <= 8) return launch<8>(a, stream);
    return launch<16>(a, stream);
}
