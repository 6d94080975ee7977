"""Host reference of the grammar-constrained beam search (test infrastructure): the selection rule of
``pnmn_attn_lstm_beam`` with its tables (include/probnmn_hip.h) in torch on the CPU, fp64 by default.  It is the search of
tests/helpers/beam_reference.py with one more stage between the candidate table and the selection:

    state[b][k] = 0 at the start; at step t (0-based) of T, hypothesis k in state s, not finished:
      token v (not pad / unk / start / end) stays a candidate only if min_left[next_state[s][token_class[v]]] <= T - 1 - t
      @end@ stays a candidate only if min_left[s] == 0
    a finished hypothesis offers @end@ at its own score, as before, and keeps its state
    a survivor's state: next_state[state of its parent][token_class[token]]; on @end@ the parent's state

The automaton is taken as plain arrays (anything ``numpy.array`` reads): ``token_class`` [V], ``next_state``
[n_states, n_classes], ``min_left`` [n_states]."""
import os
import sys
from typing import List

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_reference as br  # noqa: E402

from oracle.seq2seq_oracle import END, START  # noqa: E402

NEG_INF = br.NEG_INF


def _tables(token_class, next_state, min_left):
    tc, ns, ml = (torch.from_numpy(np.array(a, dtype=np.int64)) for a in (token_class, next_state, min_left))  # (copies)
    tc, ml = tc.reshape(-1), ml.reshape(-1)
    assert ns.dim() == 2 and ml.numel() == ns.size(0)
    assert int(tc.max()) < ns.size(1) and int(ns.max()) < ns.size(0)
    return tc, ns, ml


def constrain(cand: torch.Tensor, last: torch.Tensor, state: torch.Tensor, left_after: int, tc, ns, ml) -> torch.Tensor:
    """cand [B, K*V] of ``beam_reference.candidate_table`` -> the same with every candidate the automaton rules out at
    -inf.  ``state`` [B, K]; ``left_after`` = T - 1 - t, the steps that remain after this one."""
    B, K = last.shape
    V = cand.size(1) // K
    assert tc.numel() == V
    after = ns[state.unsqueeze(-1), tc.view(1, 1, V)]  # [B, K, V]: the state every token leads to
    allowed = ml[after] <= left_after
    allowed[:, :, END] = ml[state] == 0
    allowed = allowed | (last == END).unsqueeze(-1)  # (a finished hypothesis: candidate_table left it @end@ alone)
    return torch.where(allowed.view(B, K * V), cand, torch.full_like(cand, NEG_INF))


def advance_state(state: torch.Tensor, tok: torch.Tensor, bp: torch.Tensor, tc, ns) -> torch.Tensor:
    parent = state.gather(1, bp)
    return torch.where(tok == END, parent, ns[parent, tc[tok]])


def _start(sd, source_tokens, K, dtype):
    enc, fmask, h0 = br.encode(sd, source_tokens)
    B = source_tokens.size(0)
    h = h0.unsqueeze(1).expand(B, K, -1).contiguous()
    last = torch.full((B, K), START, dtype=torch.long)
    score = torch.full((B, K), NEG_INF, dtype=dtype)
    score[:, 0] = 0.0
    return enc, fmask, h, torch.zeros_like(h), last, score, torch.zeros(B, K, dtype=torch.long)


@torch.no_grad()
def beam_search(sd, source_tokens: torch.Tensor, beam: int, steps: int, token_class, next_state, min_left,
                dtype=torch.float64):
    """As ``beam_reference.beam_search``, under the automaton; also returns "states" [B, K], the state of every slot
    after the last step.  "margin" is taken over the constrained candidates."""
    tc, ns, ml = _tables(token_class, next_state, min_left)
    sd = br._cast(sd, dtype)
    K = beam
    enc, fmask, h, c, last, score, state = _start(sd, source_tokens, K, dtype)
    toks, bps, scs = [], [], []
    margin = torch.full((source_tokens.size(0),), float("inf"), dtype=dtype)
    for t in range(steps):
        h2, c2, cand = br.candidates(sd, enc, fmask, h, c, last, score)
        cand = constrain(cand, last, state, steps - 1 - t, tc, ns, ml)
        tok, bp, score, ranked = br.select(cand, K)
        gap = ranked[:, :-1] - ranked[:, 1:]
        gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)  # (-inf) - (-inf): no candidate at all
        margin = torch.minimum(margin, gap.min(1)[0])
        h, c = br._advance(h2, c2, tok, bp)
        state = advance_state(state, tok, bp, tc, ns)
        last = tok
        toks.append(tok), bps.append(bp), scs.append(score)
    trace_tokens, trace_backptr, trace_scores = torch.stack(toks, 1), torch.stack(bps, 1), torch.stack(scs, 1)
    return {"tokens": br.backtrack(trace_tokens, trace_backptr), "scores": score, "trace_tokens": trace_tokens,
            "trace_backptr": trace_backptr, "trace_scores": trace_scores, "margin": margin, "states": state}


@torch.no_grad()
def replay(sd, source_tokens: torch.Tensor, trace_tokens: torch.Tensor, trace_backptr: torch.Tensor, token_class,
           next_state, min_left, dtype=torch.float64, live=None) -> List[torch.Tensor]:
    """As ``beam_reference.replay``: follow the given prefixes (and their states); per step the CONSTRAINED candidate
    table [B, K*V] of the hypotheses the trace kept up to that step.

    Under a constraint a beam can be wider than the number of accepted continuations, so slots WITHOUT a hypothesis occur
    (token @end@, back-pointer 0, score -inf) and must stay empty in the later steps: their score is -inf, not the entry
    of the table their (token, back-pointer) happens to name.  ``live`` [B, T, K] (bool) says which slots hold a
    hypothesis; ``None``: every slot but those that repeat the choice of an earlier slot of the same step (the rule's
    empty slot names slot 0's @end@, and two hypotheses never make the same choice)."""
    tc, ns, ml = _tables(token_class, next_state, min_left)
    sd = br._cast(sd, dtype)
    B, T, K = trace_tokens.shape
    enc, fmask, h, c, last, score, state = _start(sd, source_tokens, K, dtype)
    tables = []
    for t in range(T):
        h2, c2, cand = br.candidates(sd, enc, fmask, h, c, last, score)
        cand = constrain(cand, last, state, T - 1 - t, tc, ns, ml)
        tables.append(cand)
        V = cand.size(1) // K
        tok, bp = trace_tokens[:, t].long(), trace_backptr[:, t].long()
        flat = bp * V + tok
        if live is not None:
            holds = live[:, t].bool()
        else:
            earlier = (flat.unsqueeze(2) == flat.unsqueeze(1)) & torch.ones(K, K, dtype=torch.bool).tril(-1)
            holds = ~earlier.any(2)
        score = torch.where(holds, cand.gather(1, flat), torch.full_like(score, NEG_INF))
        h, c = br._advance(h2, c2, tok, bp)
        state = advance_state(state, tok, bp, tc, ns)
        last = tok
    return tables
