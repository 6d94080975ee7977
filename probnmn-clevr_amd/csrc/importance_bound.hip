// The importance-weighted bound of question coding and its VIMCO gradients, for gfx950:
//     log w_r = log p(x | z_r) + beta (log p(z_r) - log q(z_r | x))      over the K sampled programs z_r of a question
//     bound   = logsumexp_k(log w) - log K
// from the teacher-forced logits of the reconstructor (x), the prior (p) and the generator (q) and the tokens they score:
// per row the three sequence log-probabilities, log w, its share of the question's weight and the learning signal of the
// generator's score-function gradient (the bound minus the row's leave-one-out baseline); per question the bound, the
// effective sample size and the support; in gradient mode d(-bound) / d logits of the x and p terms and the VIMCO estimate
// for the q term.
//
// Not in the reference, which scores ONE sampled program per question through per-token mean losses
// (probnmn/modules/elbo.py:130-161).  include/probnmn_importance.h states the contract;
// tests/helpers/importance_bound_reference.py is the same in fp64 numpy.
//
//   workgroup   512 threads = eight wavefronts, one QUESTION (its K <= 64 rows g K .. g K + K - 1) per workgroup; no LDS, no
//               atomics, no wait on another workgroup, every loop bounded by the arguments
//   rows        wave w takes the question's rows w, w + 8, ...: a row's terms and its log w come from exactly one wave in a
//               fixed order (sequence_term.h: row_log_likelihood(), the function pnmn_hypothesis_posterior sums with)
//   log w       the wave's lane 0 parks it in log_weight[r]; ONE __syncthreads(); wave 0 then holds the question's K values,
//               one per lane, and computes bound, share, ess and signal in registers
//   baseline    lane k sums over j != k DIRECTLY, in ascending j, the values broadcast by __shfl -- never as a difference
//               from the question's totals, which cancels when one sample dominates; K^2 <= 4096 adds per question
//   gradients   (GRAD) a second __syncthreads() that every wave reaches -- waves 1..7 skip wave 0's epilogue and wait at it
//               -- then every wave takes ITS OWN rows again and writes them through row_gradient() with the coefficients
//               share, beta share and signal - beta share; a question without full support, and a term that is left out, is
//               one run of zeros.  No word outside the question's rows is touched.
//
// The same kernel body with the ANSWER TERM in the weight is pnmn_importance_bound_joint, the bound on log p(x, a | image) of
// joint training (include/probnmn_importance_joint.h; tests/helpers/importance_joint_reference.py):
//     log w_r = (log p(x | z_r) + beta (log p(z_r) - log q(z_r | x))) + gamma log p(a | z_r, image)
// The answer term is a Term of sequence_term.h with ONE step whose vocabulary is the answers and whose token is the
// question's answer: the wave that owns the row computes it with row_log_likelihood() after the other three and adds it
// last, and in gradient mode writes its d_a_logits row with row_gradient() and the coefficient gamma share.  The kernel is a
// template on the argument block: with BoundArgs no line of the answer term is compiled.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/probnmn_importance.h"
#include "../../include/probnmn_importance_joint.h"
#include "hypothesis_group.h"
#include "sequence_term.h"

namespace {

using namespace pnmn::hypothesis;

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / WAVE;
constexpr int MAX_SAMPLES = WAVE;  // wave 0 holds a question's log w one per lane

struct BoundArgs {
    Term x, p, q;  // (Term::w is not used: the coefficients are 1, beta and -beta; p.scored: the prior term enters log w)
    float beta;
    int samples;
    float* log_weight;
    float* share;
    float* signal;
    float* bound;
    float* ess;
    int32_t* support;
};

struct JointArgs : BoundArgs {  // ... and the answer term of pnmn_importance_bound_joint
    const float* a_logits;     // [n_rows][A]
    const int64_t* answers;    // [n_questions]: ONE per question
    const int32_t* valid;      // [n_rows] or null: every row is valid
    float* log_pa;             // [n_rows] or null
    int64_t* row_predictions;  // [n_rows] or null
    float* d_a_logits;         // gradient mode: [n_rows][A] or null
    int A;
    float gamma;               // the answer's weight; exactly 0 leaves the term out of log w
    float invalid_log_answer;
    int unknown_index;
};

constexpr int NO_PAD = -1;  // the answer term's padding value; the kernel never scores an answer outside [0, A) with it

// sequence_term.h's two functions, inlined at every call: with four terms the compiler otherwise keeps one copy of an
// instantiation out of line, and a call costs the kernel a stack (the build log's ScratchSize must stay 0).
template <int NPER, int U>
__device__ __forceinline__ float log_likelihood(const Term& k, int r, int lane) {
    [[clang::always_inline]] return row_log_likelihood<NPER, U>(k, r, lane);
}
template <int NPER, int U>
__device__ __forceinline__ void gradient(const Term& k, int r, int lane, bool use, float share) {
    [[clang::always_inline]] row_gradient<NPER, U>(k, r, lane, use, share);
}

template <int NPER, bool GRAD, class Args>
__global__ __launch_bounds__(THREADS) void importance_bound_kernel(const Args a) {
    constexpr bool ANSWER = std::is_same<Args, JointArgs>::value;
    constexpr int U = NPER <= 2 ? 8 : 16 / NPER;  // steps in flight per wave, as in hypothesis_posterior_kernel
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const int g = blockIdx.x;
    const int K = a.samples;
    const int start = g * K, end = start + K;
    // The answer term as a Term of ONE step over the answers, whose token -- for every row of the question -- is the
    // question's answer (stride 0).  Built here, inlined below: its constants fold and it never leaves the registers.
    // An answer outside [0, A) is decided HERE, never by the term's padding rule, and is never used as an index.
    [[maybe_unused]] Term ans{};
    [[maybe_unused]] bool answer_in_range = false;
    if constexpr (ANSWER) {
        ans = Term{a.a_logits, a.answers + g, 0, a.log_pa, a.d_a_logits, a.gamma, 1, a.A, NO_PAD, a.gamma != 0.f};
        const int64_t answer = a.answers[g];
        answer_in_range = answer >= 0 && answer < (int64_t)a.A;  // (uniform over the workgroup)
    }

    // ---- every wave: the three terms and log w of its rows ----
    for (int r = start + wave; r < end; r += WAVES) {
        const float lx = log_likelihood<NPER, U>(a.x, r, lane);
        const float lq = log_likelihood<NPER, U>(a.q, r, lane);
        bool whole = finite(lx);
        float lw = lx;
        if (a.p.scored) {  // (wave-uniform: the prior is given and beta != 0)
            const float lp = log_likelihood<NPER, U>(a.p, r, lane);
            if (lane == 0 && a.p.out) a.p.out[r] = lp;
            whole = whole && finite(lp) && finite(lq);
            lw += a.beta * (lp - lq);
        } else if (a.beta != 0.f) {
            whole = whole && finite(lq);
            lw -= a.beta * lq;
        }
        if constexpr (ANSWER) {
            // (wave-uniform throughout: r, the row's validity and the question's answer are the same in every lane)
            const bool valid = a.valid == nullptr || a.valid[r] != 0;
            float la = a.invalid_log_answer;
            int prediction = a.unknown_index;
            if (valid) {
                float z[NPER], best;
                load_columns<NPER>(a.a_logits + (size_t)r * a.A, a.A, lane, z);
                best = z[0];
                prediction = lane;
#pragma unroll
                for (int k = 1; k < NPER; ++k)
                    if (z[k] > best) best = z[k], prediction = lane + WAVE * k;  // (the lane's first maximum)
                wave_argmax(best, prediction);
                la = -INFINITY;
                if (answer_in_range) la = log_likelihood<NPER, 1>(ans, r, lane);  // (one step)
                if (!finite(la)) la = -INFINITY;  // (a -inf at the answer, a row without a finite logit: never a NaN)
            }
            if (lane == 0) {
                if (a.log_pa) a.log_pa[r] = la;
                if (a.row_predictions) a.row_predictions[r] = (int64_t)prediction;
            }
            if (a.gamma != 0.f) {  // (exactly 0: the term is left out, no 0 * -inf)
                whole = whole && finite(la);
                lw += a.gamma * la;
            }
        }
        if (lane == 0) {
            if (a.x.out) a.x.out[r] = lx;
            if (a.q.out) a.q.out[r] = lq;
            a.log_weight[r] = whole ? lw : -INFINITY;  // (a term that is not finite: -inf, never inf - inf)
        }
    }
    __syncthreads();  // (workgroup scope: the log w the other waves stored are visible to wave 0)
    if constexpr (!GRAD) {
        if (wave != 0) return;
    }

    // ---- wave 0: the question's K values, one per lane ----
    if (!GRAD || wave == 0) {  // (gradient mode: the other waves go on to the second barrier, none returns before it)
        const bool mine = lane < K;
        const float v = mine ? a.log_weight[start + lane] : -INFINITY;
        const int count = wave_sum(mine && finite(v) ? 1 : 0);
        const bool counts = count == K;  // (wave-uniform)
        float bound = -INFINITY, ess = 0.f, share = 0.f, signal = 0.f;
        if (counts) {
            const float log_k = logf((float)K);
            const float top = wave_max(v);  // (lanes beyond K hold -inf: they win no maximum and add exp(-inf) = 0)
            const float log_norm = logf(wave_sum(expf(v - top)));
            bound = (top + log_norm) - log_k;
            share = mine ? expf((v - top) - log_norm) : 0.f;
            ess = 1.f / wave_sum(share * share);
            signal = bound;  // (K = 1: no other sample to take a baseline from)
            if (K > 1) {
                // the leave-one-out terms of lane k, over j != k in ascending j
                float m = -INFINITY, sum_log = 0.f;
                for (int j = 0; j < K; ++j) {
                    const float vj = __shfl(v, j, WAVE);
                    if (j != lane) {
                        m = fmaxf(m, vj);
                        sum_log += vj;
                    }
                }
                const float mean_log = sum_log / (float)(K - 1);  // (<= m: a mean of values that are at most m)
                float se = 0.f;
                for (int j = 0; j < K; ++j) {
                    const float vj = __shfl(v, j, WAVE);
                    if (j != lane) se += expf(vj - m);
                }
                const float baseline = (m + logf(se + expf(mean_log - m))) - log_k;
                signal = bound - baseline;
            }
        }
        if (mine) {
            a.share[start + lane] = share;
            a.signal[start + lane] = counts ? signal : 0.f;
        }
        if (lane == 0) {
            a.bound[g] = bound;
            if (a.ess) a.ess[g] = ess;
            if (a.support) a.support[g] = count;
        }
    }

    // ---- gradient mode, every wave: the gradients of its rows ----
    if constexpr (GRAD) {
        __syncthreads();  // (what wave 0 stored, a lane per row, is visible to every wave; all 512 threads arrive)
        const bool counts = finite(a.bound[g]);  // (wave-uniform; -inf for a question without full support)
        for (int r = start + wave; r < end; r += WAVES) {
            const float share = counts ? a.share[r] : 0.f;
            const float signal = counts ? a.signal[r] : 0.f;
            if (a.x.d) gradient<NPER, U>(a.x, r, lane, counts, share);
            if (a.p.d) gradient<NPER, U>(a.p, r, lane, counts && a.p.scored, a.beta * share);
            if (a.q.d) gradient<NPER, U>(a.q, r, lane, counts, signal - a.beta * share);
            if constexpr (ANSWER) {
                // (a question that counts with gamma != 0 has its answer in range; an invalid row is zeros, not read)
                const bool valid = a.valid == nullptr || a.valid[r] != 0;
                if (a.d_a_logits)
                    gradient<NPER, 1>(ans, r, lane, counts && valid && ans.scored && answer_in_range,
                                                                   a.gamma * share);
            }
        }
    }
}

}  // namespace

// The argument checks of both entry points that answer PNMN_EINVAL, in the order include/probnmn_importance.h states.
static int check_arguments(const float* x_logits, const int64_t* x_tokens, int Tx, int Vx, const float* p_logits,
                           const int64_t* p_tokens, int Tp, int Vp, const float* q_logits, const int64_t* q_tokens, int Tq, int Vq,
                           float beta, const float* log_weight, const float* share, const float* signal, const float* bound,
                           const float* d_p_logits) {
    if (!x_logits || !x_tokens || !q_logits || !q_tokens || !log_weight || !share || !signal || !bound) return PNMN_EINVAL;
    if ((p_logits && !p_tokens) || (d_p_logits && !p_logits)) return PNMN_EINVAL;
    if (Tx < 1 || Vx < 1 || Tq < 1 || Vq < 1 || (p_logits && (Tp < 1 || Vp < 1))) return PNMN_EINVAL;
    if (!(beta >= 0.f && beta < INFINITY)) return PNMN_EINVAL;  // (false for a NaN)
    return 0;
}

// ... and those that answer PNMN_ESHAPE
static int check_shapes(int Vx, const float* p_logits, int Vp, int Vq, int n_questions, int samples) {
    if (Vx > MAX_COLUMNS || Vq > MAX_COLUMNS || (p_logits && Vp > MAX_COLUMNS)) return PNMN_ESHAPE;
    if ((int64_t)n_questions * samples > (int64_t)INT32_MAX) return PNMN_ESHAPE;  // (rows are indexed with an int)
    return 0;
}

template <class Args>
static int launch(const Args& a, int widest, bool grad, int n_questions, void* stream) {
    return with_nper(widest, [&](auto nper) {
        constexpr int NPER = decltype(nper)::value;
        const auto kernel = grad ? importance_bound_kernel<NPER, true, Args> : importance_bound_kernel<NPER, false, Args>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_questions), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
        return (int)hipGetLastError();
    });
}

static void fill(BoundArgs& a, const float* x_logits, const int64_t* x_tokens, int64_t x_token_stride, int pad_x, int Tx, int Vx,
                 const float* p_logits, const int64_t* p_tokens, int64_t p_token_stride, int pad_p, int Tp, int Vp,
                 const float* q_logits, const int64_t* q_tokens, int64_t q_token_stride, int pad_q, int Tq, int Vq, float beta,
                 int samples, float* log_px, float* log_pz, float* log_q, float* log_weight, float* share, float* signal,
                 float* bound, float* ess, int32_t* support, float* d_x_logits, float* d_p_logits, float* d_q_logits) {
    const bool score_p = p_logits && beta != 0.f;  // (otherwise the prior term is left out entirely: not read, not reported)
    a.x = Term{x_logits, x_tokens, x_token_stride, log_px, d_x_logits, 1.f, Tx, Vx, pad_x, true};
    a.p = Term{score_p ? p_logits : nullptr, p_tokens, p_token_stride, log_pz, d_p_logits, beta, Tp, Vp, pad_p, score_p};
    a.q = Term{q_logits, q_tokens, q_token_stride, log_q, d_q_logits, -beta, Tq, Vq, pad_q, beta != 0.f};
    a.beta = beta;
    a.samples = samples;
    a.log_weight = log_weight;
    a.share = share;
    a.signal = signal;
    a.bound = bound;
    a.ess = ess;
    a.support = support;
}

extern "C" int pnmn_importance_bound(const float* x_logits, const int64_t* x_tokens, int64_t x_token_stride, int pad_x, int Tx,
                                     int Vx, const float* p_logits, const int64_t* p_tokens, int64_t p_token_stride, int pad_p,
                                     int Tp, int Vp, const float* q_logits, const int64_t* q_tokens, int64_t q_token_stride,
                                     int pad_q, int Tq, int Vq, float beta, int n_questions, int samples, float* log_px,
                                     float* log_pz, float* log_q, float* log_weight, float* share, float* signal, float* bound,
                                     float* ess, int32_t* support, float* d_x_logits, float* d_p_logits, float* d_q_logits,
                                     void* stream) {
    if (n_questions < 0 || samples < 1 || samples > MAX_SAMPLES) return PNMN_EINVAL;
    if (n_questions == 0) return 0;  // (nothing to read or to write)
    if (const int rc = check_arguments(x_logits, x_tokens, Tx, Vx, p_logits, p_tokens, Tp, Vp, q_logits, q_tokens, Tq, Vq, beta,
                                       log_weight, share, signal, bound, d_p_logits))
        return rc;
    if (const int rc = check_shapes(Vx, p_logits, Vp, Vq, n_questions, samples)) return rc;
    const bool grad = d_x_logits || d_p_logits || d_q_logits;
    BoundArgs a;
    fill(a, x_logits, x_tokens, x_token_stride, pad_x, Tx, Vx, p_logits, p_tokens, p_token_stride, pad_p, Tp, Vp, q_logits,
         q_tokens, q_token_stride, pad_q, Tq, Vq, beta, samples, log_px, log_pz, log_q, log_weight, share, signal, bound, ess,
         support, d_x_logits, d_p_logits, d_q_logits);
    return launch(a, std::max(std::max(Vx, Vq), a.p.scored ? Vp : 1), grad, n_questions, stream);
}

extern "C" int pnmn_importance_bound_joint(const float* x_logits, const int64_t* x_tokens, int64_t x_token_stride, int pad_x,
                                           int Tx, int Vx, const float* p_logits, const int64_t* p_tokens, int64_t p_token_stride,
                                           int pad_p, int Tp, int Vp, const float* q_logits, const int64_t* q_tokens,
                                           int64_t q_token_stride, int pad_q, int Tq, int Vq, float beta, int n_questions,
                                           int samples, float* log_px, float* log_pz, float* log_q, float* log_weight,
                                           float* share, float* signal, float* bound, float* ess, int32_t* support,
                                           float* d_x_logits, float* d_p_logits, float* d_q_logits, const float* a_logits,
                                           const int32_t* valid, const int64_t* answers, int num_answers, float answer_weight,
                                           float invalid_log_answer, int unknown_index, float* log_pa, int64_t* row_predictions,
                                           float* d_a_logits, void* stream) {
    if (n_questions < 0 || samples < 1 || samples > MAX_SAMPLES) return PNMN_EINVAL;
    if (n_questions == 0) return 0;  // (nothing to read or to write)
    if (const int rc = check_arguments(x_logits, x_tokens, Tx, Vx, p_logits, p_tokens, Tp, Vp, q_logits, q_tokens, Tq, Vq, beta,
                                       log_weight, share, signal, bound, d_p_logits))
        return rc;
    if (!a_logits || !answers) return PNMN_EINVAL;
    if (num_answers < 1) return PNMN_EINVAL;
    if (!(answer_weight >= 0.f && answer_weight < INFINITY)) return PNMN_EINVAL;  // (false for a NaN)
    if (!(invalid_log_answer <= 0.f)) return PNMN_EINVAL;  // (false for a NaN, a positive value and +inf; -inf passes)
    if (num_answers > MAX_COLUMNS) return PNMN_ESHAPE;
    if (const int rc = check_shapes(Vx, p_logits, Vp, Vq, n_questions, samples)) return rc;
    const bool grad = d_x_logits || d_p_logits || d_q_logits || d_a_logits;
    JointArgs a;
    fill(a, x_logits, x_tokens, x_token_stride, pad_x, Tx, Vx, p_logits, p_tokens, p_token_stride, pad_p, Tp, Vp, q_logits,
         q_tokens, q_token_stride, pad_q, Tq, Vq, beta, samples, log_px, log_pz, log_q, log_weight, share, signal, bound, ess,
         support, d_x_logits, d_p_logits, d_q_logits);
    a.a_logits = a_logits;
    a.answers = answers;
    a.valid = valid;
    a.log_pa = log_pa;
    a.row_predictions = row_predictions;
    a.d_a_logits = d_a_logits;
    a.A = num_answers;
    a.gamma = answer_weight;
    a.invalid_log_answer = invalid_log_answer;
    a.unknown_index = unknown_index;
    return launch(a, std::max(std::max(std::max(Vx, Vq), a.p.scored ? Vp : 1), num_answers), grad, n_questions, stream);
}
