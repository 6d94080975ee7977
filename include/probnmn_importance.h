/*
 * probnmn_importance.h -- the importance-weighted extension of libprobnmn_hip.so: the K-sample bound on log p(x) of question
 * coding and its VIMCO gradients, from the teacher-forced logits of the reconstructor, the prior and the generator.  The
 * kernel is in csrc/importance_bound.hip and links into the same library.
 *
 * A further header on purpose, as include/probnmn_grammar.h is: include/probnmn_hip.h is the core ABI, whose version, entry
 * points, records and launch ops are pinned; what is declared here adds to the library without touching any of them.  The
 * conventions are the core header's, word for word -- device pointers, row strides in elements, asynchronous on `stream`,
 * 0 / negative PNMN_E* / positive hipError_t -- and so are the declaration conventions, so probnmn._hip.read_header reads
 * this file as it is; probnmn/_hip_importance.py binds it onto the handle the core binding returns.
 */
#ifndef PROBNMN_IMPORTANCE_H
#define PROBNMN_IMPORTANCE_H

#include <stdint.h>

#include "probnmn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The importance-weighted bound of a discrete latent (Burda et al. 2016) with the VIMCO gradient estimator (Mnih & Rezende
 * 2016).  Not in the reference, whose ELBO scores one sampled program per question through per-token mean losses
 * (probnmn/modules/elbo.py:130-161); replaces two gradient-mode pnmn_hypothesis_posterior launches, a torch composition for
 * the leave-one-out terms and a multiply per gradient tensor.
 *
 * Question g has `samples` = K programs z_1 .. z_K drawn from the generator, question-major: row r = g K + k, n_rows =
 * n_questions K.  Of row r, as pnmn_hypothesis_posterior computes a term (the sum over the steps whose token is not the
 * term's padding of log_softmax(logits[r][t])[token], in ascending step order; -inf when a scored token is no index into
 * the vocabulary, which is then never used as one; 0 for a row of padding; bit for bit its log_px for the same inputs):
 *   lx_r = log p(x_g | z_r)   the reconstructor's term (x)
 *   lp_r = log p(z_r)         the prior's term (p); left out -- not read, not reported -- when p_logits is NULL or beta == 0
 *   lq_r = log q(z_r | x_g)   the generator's term (q); always computed, it leaves log w when beta == 0
 *   log w_r  = lx_r + beta (lp_r - lq_r)  over the terms that enter; -inf when one of them is not finite (no inf - inf)
 *   support[g] = the rows of g with a finite log w.  A question COUNTS when support[g] == K; then, over its rows,
 *   bound[g]  = logsumexp_k(log w) - log K       (beta = 1: E[bound] <= log p(x_g), tightening as K grows)
 *   share[r]  = exp(log w_r - logsumexp_k(log w))
 *   ess[g]    = 1 / sum_k share^2
 *   b_r       = m + log(sum_{j != k} exp(log w_j - m) + exp(mean_{j != k} log w_j - m)) - log K,  m = max_{j != k} log w_j,
 *               each sum taken directly over j != k in ascending j, never as a difference from the question's total
 *   signal[r] = bound[g] - b_r for K >= 2;  bound[g] for K = 1
 * A question that does not count: bound = -inf, share = signal = 0 over its rows, ess = 0, every gradient row zeros;
 * log_weight keeps what its rows have.
 *
 * GRADIENT MODE (any of d_x_logits / d_p_logits / d_q_logits given; each needs its term's logits): with ce[t][v] =
 * softmax(logits[r][t])[v] - [v == token] on the scored steps (a logit of -inf gets exactly 0),
 *   d_x_logits[r][t] = share[r] ce                               = d(-bound[g]) / d x_logits, exact
 *   d_p_logits[r][t] = beta share[r] ce                          exact (zeros when the term is left out)
 *   d_q_logits[r][t] = (signal[r] - beta share[r]) ce            VIMCO: signal is a constant of the estimator
 * Every word of a given gradient tensor over the rows [0, n_rows) is written -- padding steps and questions that do not
 * count as zeros -- so the caller need not fill it first.  The outputs the two modes share are the same bits.
 *
 * One 512-thread workgroup per question; a question's outputs depend on its own K rows only (the same bits alone or in a
 * batch).  No LDS, no atomics, no workspace, no wait on another workgroup.  Logits: contiguous fp32 [n_rows][T][V]; tokens:
 * int64, row r at tokens + r * token_stride, T entries.  log_px / log_pz / log_q, log_weight / share / signal: fp32
 * [n_rows]; bound / ess: fp32 [n_questions]; support: int32 [n_questions].
 * Checked in this order, before any HIP call: n_questions < 0 or samples outside 1 .. 64: PNMN_EINVAL; n_questions == 0:
 * 0, nothing launched, whatever else is given; PNMN_EINVAL for a null x_logits / x_tokens / q_logits / q_tokens /
 * log_weight / share / signal / bound, p_logits without p_tokens, d_p_logits without p_logits, T < 1 or V < 1 of a given
 * term, beta negative or not finite; PNMN_ESHAPE for a given term's V > 1024 or n_questions * samples beyond int32.
 * ------------------------------------------------------------------------------------------- */
int pnmn_importance_bound(const float* x_logits, const int64_t* x_tokens, int64_t x_token_stride, int pad_x, int Tx, int Vx,
                          const float* p_logits /* may be NULL */, const int64_t* p_tokens, int64_t p_token_stride, int pad_p,
                          int Tp, int Vp, const float* q_logits, const int64_t* q_tokens, int64_t q_token_stride, int pad_q,
                          int Tq, int Vq, float beta, int n_questions, int samples, float* log_px /* may be NULL */,
                          float* log_pz /* may be NULL */, float* log_q /* may be NULL */, float* log_weight, float* share,
                          float* signal, float* bound, float* ess /* may be NULL */, int32_t* support /* may be NULL */,
                          float* d_x_logits, float* d_p_logits, float* d_q_logits /* all NULL: plain launch */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROBNMN_IMPORTANCE_H */
