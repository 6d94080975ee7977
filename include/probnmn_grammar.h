/*
 * probnmn_grammar.h -- the grammar extension of libprobnmn_hip.so: the generator's step distributions renormalised over the
 * allowed sets of a token automaton, so that a trainer can score programs under the distribution the constrained sampler
 * draws from.  The kernels are in csrc/grammar_logits.hip and link into the same library.
 *
 * A second header on purpose: include/probnmn_hip.h is the core ABI, whose version, entry points, records and launch ops
 * are pinned; what is declared here adds to the library without touching any of them.  The conventions are the core
 * header's, word for word -- device pointers unless marked HOST, row strides in elements, asynchronous on `stream`, 0 /
 * negative PNMN_E* / positive hipError_t -- and so are the declaration conventions, so probnmn._hip.read_header reads this
 * file as it is; probnmn/_hip_grammar.py binds it onto the handle the core binding returns.
 */
#ifndef PROBNMN_GRAMMAR_H
#define PROBNMN_GRAMMAR_H

#include <stdint.h>

#include "probnmn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Grammar-masked logits.  Not in the reference, whose generator is trained on unconstrained samples (seq2seq_base.py:203-233);
 * replaces the torch composition where(mask, logits, -inf) over a mask built step by step on the host.
 *
 * q_c(z | x) = prod_t softmax over A_c(s_t, t) of the step's logits: the distribution the constrained sampler of
 * pnmn_attn_lstm_fwd draws from (unfiltered), which sums to one over the strings of at most `horizon` tokens the automaton
 * accepts.  log_softmax(masked)[token] = log q_c's step term, so every sequence loss of the library (pnmn_seq_nll_*, the
 * gradient mode of pnmn_hypothesis_posterior -- both specified for -inf logits) scores under q_c when it is given `masked`.
 *
 * Row b starts in state 0, not finished, and walks tokens[b][t] (the token emitted or targeted at step t), t = 0 .. T-1:
 *   S_t      = A_c(s_t, t) by the automaton rule beside pnmn_attn_lstm_fwd with T = horizon (at t >= horizon: end_index
 *              alone, and only in an accepting state; a finished row: end_index alone)
 *   outside[b] += 1  when the row has not finished, tokens[b][t] != pad_index and tokens[b][t] is not in S_t
 *   S_t     |= { tokens[b][t] }  when it lies in [0, V);  S_t = [0, V) (the step is copied unmasked) if it is still empty
 *   masked[b][t][v]  = the bits of logits[b][t][v] for v in S_t, -inf otherwise: no step is all -inf
 *   log_mass[b][t]   = logsumexp over S_t - logsumexp over [0, V)  <= 0, exactly 0 for an unmasked step: the share of the
 *                      unconstrained step distribution inside the grammar; log q = log q_c + sum of log_mass over the steps
 *   state:   as the decoders advance it (end_index finishes the row, any other token in [0, V) moves it); a token outside
 *            [0, V) leaves it as it is
 * The backward pass walks the same tokens to the same sets:
 *   d_logits[b][t][v] = d_masked[b][t][v] for v in S_t, exactly 0 otherwise.
 *
 * One wavefront per row; a row's outputs depend on that row alone (the same bits alone or in a batch).  No atomics, no
 * workspace.  logits / masked / d_masked / d_logits: fp32 [B][T][V], step stride V, row stride given; tokens: int64 [B][T],
 * row stride given; log_mass: fp32 [B][T] or NULL; outside: int32 [B] or NULL.  The tables are HOST pointers, checked entry by
 * entry and passed by value, as for the decoders.
 * Returns PNMN_EINVAL and launches nothing for: B, T or V negative; then, B == 0 or T == 0: 0, nothing launched, whatever
 * else is given; otherwise PNMN_EINVAL for V == 0, a null logits / tokens / masked (backward: d_masked / tokens / d_logits),
 * a missing table, a table entry out of range, n_states or n_classes outside their limits, end_index outside [0, V),
 * horizon < 1, min_left[0] > horizon.  V > 128 (the decoders' limit for automaton tables): PNMN_ESHAPE.
 * ------------------------------------------------------------------------------------------- */
int pnmn_grammar_logits(const float* logits, int64_t logits_bstride, const int64_t* tokens, int64_t tok_bstride,
                        float* masked, int64_t masked_bstride, float* log_mass, int32_t* outside, int B, int T, int V,
                        int horizon, int pad_index, int unk_index, int start_index, int end_index,
                        const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                        const uint8_t* min_left /* HOST */, int n_states, int n_classes, void* stream);
int pnmn_grammar_logits_bwd(const float* d_masked, int64_t d_masked_bstride, const int64_t* tokens, int64_t tok_bstride,
                            float* d_logits, int64_t d_logits_bstride, int B, int T, int V, int horizon, int pad_index,
                            int unk_index, int start_index, int end_index, const uint8_t* token_class /* HOST */,
                            const uint8_t* next_state /* HOST */, const uint8_t* min_left /* HOST */, int n_states,
                            int n_classes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROBNMN_GRAMMAR_H */
