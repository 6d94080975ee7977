/*
 * probnmn_importance_joint.h -- the joint importance-weighted extension of libprobnmn_hip.so: the K-sample bound on
 * log p(x, a | image) of joint training -- pnmn_importance_bound's weight with the answer likelihood of the module network
 * inside it -- its exact gradients and its VIMCO gradient.  The kernel is the one of csrc/importance_bound.hip, instantiated
 * with the answer term, and links into the same library.
 *
 * A further header on purpose, as include/probnmn_importance.h is: include/probnmn_hip.h is the core ABI, whose version,
 * entry points, records and launch ops are pinned, and include/probnmn_importance.h is pinned at its one entry point; what
 * is declared here adds to the library without touching either.  The conventions are the core header's, word for word --
 * device pointers, row strides in elements, asynchronous on `stream`, 0 / negative PNMN_E* / positive hipError_t -- and so
 * are the declaration conventions, so probnmn._hip.read_header reads this file as it is; probnmn/_hip_importance_joint.py
 * binds it onto the handle the core binding returns.
 */
#ifndef PROBNMN_IMPORTANCE_JOINT_H
#define PROBNMN_IMPORTANCE_JOINT_H

#include <stdint.h>

#include "probnmn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The importance-weighted bound on log p(x, a | image) over K sampled programs, with the VIMCO estimator for the generator.
 * Not in the reference, whose joint objective adds the answer's cross entropy of ONE sampled program to a single-sample ELBO
 * of per-token mean losses (probnmn/trainers/joint_training_trainer.py, modules/elbo.py:130-161); replaces two gradient-mode
 * pnmn_hypothesis_posterior launches, a torch composition for the leave-one-out terms, pnmn_answer_loss and a multiply per
 * gradient tensor.
 *
 * Everything pnmn_importance_bound takes, in its order and under its contract (include/probnmn_importance.h: rows
 * question-major, r = g K + k; the terms lx_r, lp_r, lq_r; support, bound, share, ess, baseline -- the leave-one-out sums
 * taken directly over j != k -- signal, and the rule for a question that does not count), then the ANSWER TERM of row r of
 * question g, with z = a_logits[r] and a = answers[g] (one answer per question, not per row):
 *   a valid row (valid NULL, or valid[r] != 0):
 *     la_r = (z[a] - max z) - log sum exp(z - max z)     = log p(a_g | z_r, image_g)
 *     -inf when answers[g] lies outside [0, num_answers) -- such an answer is never used as an index, and no value of it is
 *     taken for padding --, when the logit at the answer is -inf, and whenever the expression is not a finite number
 *   an invalid row (valid[r] == 0):
 *     la_r = invalid_log_answer (<= 0; or -inf, which rules the question out as any term that is not finite does); the row's
 *     logits are not read and its d_a_logits row is zeros
 *   log_pa[r] = la_r
 *   row_predictions[r] = the first arg-max of a_logits[r] (pnmn_answer_loss's rule: the lowest index that holds the largest
 *     value); unknown_index for an invalid row
 *   log w_r = pnmn_importance_bound's value for the same x / p / q inputs, with answer_weight * la_r added to it afterwards,
 *     in that order: (lx_r + beta (lp_r - lq_r)) + answer_weight la_r; -inf when any entering term is not finite
 * answer_weight EXACTLY 0: the answer term is left out entirely -- it rules nothing out and no 0 * -inf is formed; log_pa and
 * row_predictions are still reported, d_a_logits is zeros, and every output the two entry points share is the same bits as
 * pnmn_importance_bound gives.
 *
 * GRADIENT MODE (any of d_x_logits / d_p_logits / d_q_logits / d_a_logits given): d_x_logits, d_p_logits and d_q_logits keep
 * their formulas, share and signal now those of the joint weight, and
 *   d_a_logits[r][c] = answer_weight share[r] (softmax(z)[c] - [c == a])     = d(-bound[g]) / d a_logits, exact
 * for a valid row of a question that counts (a logit of -inf gets exactly 0; the answer's column is found by comparing c).
 * Every word of d_a_logits over the rows [0, n_rows) is written -- zeros for invalid rows and for questions that do not count
 * -- so the caller need not fill it first.  The outputs the plain launch and the gradient launch share are the same bits.
 *
 * One 512-thread workgroup per question; a question's outputs depend on its own K rows only (the same bits alone or in a
 * batch).  No LDS, no atomics, no workspace, no wait on another workgroup; every loop is bounded by the arguments.
 * a_logits / d_a_logits: contiguous fp32 [n_rows][num_answers]; valid: int32 [n_rows]; answers: int64 [n_questions]; log_pa:
 * fp32 [n_rows]; row_predictions: int64 [n_rows]; the rest as in pnmn_importance_bound.
 * Checked in this order, before any HIP call: n_questions < 0 or samples outside 1 .. 64: PNMN_EINVAL; n_questions == 0: 0,
 * nothing launched, whatever else is given; pnmn_importance_bound's PNMN_EINVAL checks (pointers, T and V of a given term,
 * beta); PNMN_EINVAL for a null a_logits or answers; for num_answers < 1; for an answer_weight that is negative or not
 * finite; for an invalid_log_answer that is NaN, positive or +inf; PNMN_ESHAPE for num_answers > 1024, a given term's V >
 * 1024 or n_questions * samples beyond int32.
 * ------------------------------------------------------------------------------------------- */
int pnmn_importance_bound_joint(const float* x_logits, const int64_t* x_tokens, int64_t x_token_stride, int pad_x, int Tx,
                                int Vx, const float* p_logits /* may be NULL */, const int64_t* p_tokens,
                                int64_t p_token_stride, int pad_p, int Tp, int Vp, const float* q_logits,
                                const int64_t* q_tokens, int64_t q_token_stride, int pad_q, int Tq, int Vq, float beta,
                                int n_questions, int samples, float* log_px /* may be NULL */, float* log_pz /* may be NULL */,
                                float* log_q /* may be NULL */, float* log_weight, float* share, float* signal, float* bound,
                                float* ess /* may be NULL */, int32_t* support /* may be NULL */, float* d_x_logits,
                                float* d_p_logits, float* d_q_logits, const float* a_logits,
                                const int32_t* valid /* may be NULL: every row is valid */, const int64_t* answers,
                                int num_answers, float answer_weight, float invalid_log_answer, int unknown_index,
                                float* log_pa /* may be NULL */, int64_t* row_predictions /* may be NULL */,
                                float* d_a_logits /* all four NULL: plain launch */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROBNMN_IMPORTANCE_JOINT_H */
