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
//   lanes       run over the answers (hypothesis_group.h: the column layout, the group bounds, the wave reductions), so a
//               row read is one coalesced segment
//   sweep 1     weight_normaliser(): the base-usable rows and log w_r = (lw_r - largest) - log(sum)
//   sweep 2     one row at a time (the next row's logits, validity and weight are loaded before this one's are reduced):
//               row_softmax_stats(), the logit of the given answer (lane_held()), the score; every value is wave-uniform,
//               so the support, the largest score and its first row and the consistent rows are counted in scalars; lane 0
//               writes score[r] (-inf for a row that is not usable) into log_posterior[r]
//   sweep 3     ONE __syncthreads() (the scores lane 0 stored are visible to the other lanes), then score_normaliser()
//
// GRADIENT MODE (pnmn_answer_posterior without best_row and with a log_answer pointer, which is then d_logits [n_rows][A]):
// the same kernel body with GRAD set -- so the outputs the two modes share are the same bits -- and one more sweep.  The
// marginal-likelihood loss of a group is -log_evidence[g]; its gradient with respect to a row's logits is the row's
// cross-entropy gradient scaled by the row's posterior share:
//   sweep 4     a second __syncthreads() (the posteriors sweep 3 stored, a lane per row, are visible to every lane), then one
//               row at a time as in sweep 2 (the logits are in L2; the next row is loaded before this one is reduced):
//               row_softmax_stats() again -- the bits of sweep 2 --, share = w_a exp(log_posterior[r]), and
//               d_logits[r][c] = share (softmax_c - [c == answer]), one coalesced segment per register; the answer's column
//               is found by comparing c, never by indexing.  A row that is not usable, and every row when w_a is 0, is
//               written as zeros; no d_logits word outside the group's clamped rows is touched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"
#include "hypothesis_group.h"

namespace {

using namespace pnmn::hypothesis;

constexpr int THREADS = WAVE;

struct AnswerPosteriorArgs {
    const float* logits;
    const int32_t* valid;
    const float* log_weight;
    const int64_t* answers;
    const int32_t* group_start;
    float w_a;
    float* log_answer;
    float* d_logits;  // (gradient mode only: it arrives in log_answer's place)
    int64_t* row_predictions;
    float* log_posterior;
    float* log_evidence;
    int32_t* best_row;
    int32_t* support;
    int32_t* consistent_count;
    int32_t* first_consistent;
    int n_groups, n_rows, A, unknown_index;
};

template <int NPER, bool GRAD>
__global__ __launch_bounds__(THREADS) void answer_posterior_kernel(const AnswerPosteriorArgs p) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    const int A = p.A;
    const Rows rows = group_rows(p.group_start, g, p.n_rows);
    const int start = rows.start, end = rows.end;
    // the given answer: never an index unless it is one (wave-uniform)
    const int64_t answer = p.answers[g];
    const bool answer_known = answer >= 0 && answer < (int64_t)A;
    const int answer_at = __builtin_amdgcn_readfirstlane(answer_known ? (int)answer : 0);

    // ---- sweep 1: the base-usable rows and the normaliser of their weights ----
    const WeightNorm w = weight_normaliser(p.valid, p.log_weight, rows, lane);
    const float lw_max = w.lw_max, log_norm_w = w.log_norm;

    // ---- sweep 2: every row's answer likelihood, own answer and score; the group's counts and its largest score ----
    int count = 0, consistent = 0, first_consistent = -1, best = -1;
    float top = -INFINITY;
    float z[NPER], nxt[NPER];
#pragma unroll
    for (int k = 0; k < NPER; ++k) nxt[k] = -INFINITY;
    int valid_nxt = 1;
    float lw_nxt = 0.f;
    if (start < end) {
        load_columns<NPER>(p.logits + (size_t)start * A, A, lane, nxt);
        if (p.valid) valid_nxt = p.valid[start];
        if (p.log_weight) lw_nxt = p.log_weight[start];
    }
    for (int r = start; r < end; ++r) {
#pragma unroll
        for (int k = 0; k < NPER; ++k) z[k] = nxt[k];
        const bool row_valid = valid_nxt != 0;
        const float lw = lw_nxt;
        if (r + 1 < end) {
            load_columns<NPER>(p.logits + (size_t)(r + 1) * A, A, lane, nxt);
            if (p.valid) valid_nxt = p.valid[r + 1];
            if (p.log_weight) lw_nxt = p.log_weight[r + 1];
        }

        float row_max;
        int at;
        const float log_z = row_softmax_stats<NPER>(z, lane, row_max, at);
        const float target = lane_held<NPER>(z, answer_at);
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
    const float log_norm = score_normaliser(p.log_posterior, rows, lane, count, top);
    if (lane == 0) {
        p.log_evidence[g] = count > 0 ? top + log_norm : -INFINITY;
        if constexpr (!GRAD) p.best_row[g] = count > 0 ? best : -1;
        if (p.support) p.support[g] = count;
        if (p.consistent_count) p.consistent_count[g] = consistent;
        if (p.first_consistent) p.first_consistent[g] = first_consistent;
    }

    // ---- sweep 4 (gradient mode): d(-log_evidence[g]) / d logits of every row of the group ----
    if constexpr (GRAD) {
        __syncthreads();  // (the posteriors sweep 3 stored, a lane per row, are visible to every lane of the wave)
        float lp_nxt = -INFINITY;
        if (start < end) {
            load_columns<NPER>(p.logits + (size_t)start * A, A, lane, nxt);
            lp_nxt = p.log_posterior[start];
        }
        for (int r = start; r < end; ++r) {
#pragma unroll
            for (int k = 0; k < NPER; ++k) z[k] = nxt[k];
            const float lp = lp_nxt;
            if (r + 1 < end) {
                load_columns<NPER>(p.logits + (size_t)(r + 1) * A, A, lane, nxt);
                lp_nxt = p.log_posterior[r + 1];
            }
            float* __restrict__ d_row = p.d_logits + (size_t)r * A;
            // (a usable row has a finite maximum and a finite logit at the answer; every value here is wave-uniform)
            const bool use = finite(lp) && p.w_a != 0.f;
            float row_max = 0.f, log_z = 0.f, share = 0.f;
            if (use) {
                int at;
                log_z = row_softmax_stats<NPER>(z, lane, row_max, at);
                share = p.w_a * expf(lp);
            }
#pragma unroll
            for (int k = 0; k < NPER; ++k) {
                const int c = lane + WAVE * k;
                if (c < A) {
                    float d = 0.f;
                    if (use && z[k] > -INFINITY) {  // (a logit of -inf: probability 0, gradient 0)
                        const float prob = expf((z[k] - row_max) - log_z);  // (<= 1: both terms are <= 0)
                        d = share * (prob - ((answer_known && c == answer_at) ? 1.f : 0.f));
                    }
                    d_row[c] = d;
                }
            }
        }
    }
}

}  // namespace

extern "C" int pnmn_answer_posterior(const float* logits, const int32_t* valid, const float* log_weight, const int64_t* answers,
                                     const int32_t* group_start, float w_a, float* log_answer, int64_t* row_predictions,
                                     float* log_posterior, float* log_evidence, int32_t* best_row, int32_t* support,
                                     int32_t* consistent_count, int32_t* first_consistent, int n_groups, int n_rows,
                                     int num_answers, int unknown_index, void* stream) {
    if (n_groups < 0 || n_rows < 0 || num_answers < 1) return PNMN_EINVAL;
    if (n_groups == 0) return 0;  // (nothing to read or to write)
    // gradient mode: no best_row, and log_answer's place holds d_logits (refused until this mode existed: best_row was null)
    const bool grad = !best_row && log_answer;
    if (!group_start || !answers || !log_posterior || !log_evidence || (!best_row && !grad) || (n_rows > 0 && !logits))
        return PNMN_EINVAL;
    if (!(fabsf(w_a) < INFINITY)) return PNMN_EINVAL;
    if (num_answers > MAX_COLUMNS) return PNMN_ESHAPE;
    const AnswerPosteriorArgs a{logits, valid, log_weight, answers, group_start, w_a, grad ? nullptr : log_answer,
                                grad ? log_answer : nullptr, row_predictions, log_posterior, log_evidence, best_row, support,
                                consistent_count, first_consistent, n_groups, n_rows, num_answers, unknown_index};
    return with_nper(num_answers, [&](auto nper) {
        constexpr int NPER = decltype(nper)::value;
        const auto kernel = grad ? answer_posterior_kernel<NPER, true> : answer_posterior_kernel<NPER, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_groups), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
        return (int)hipGetLastError();
    });
}
