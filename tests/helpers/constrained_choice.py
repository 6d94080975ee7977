"""Host reference of the grammar-constrained token choice (the automaton rule beside ``pnmn_attn_lstm_fwd``), numpy only, fp64.

Written from the rule stated beside the entry point in include/probnmn_hip.h, not from device output.  A row carries an
automaton state (0 at the start) and a finished flag.  At step t of T its allowed set A_c holds

* token v (not pad / unk / start / end) iff ``min_left[next_state[s][token_class[v]]] <= T - 1 - t``,
* the end index iff ``min_left[s] == 0``,
* for a finished row the end index alone;

and the token is chosen as the unconstrained rules choose it with A_c in the place of "every index but pad / unk / start":

* sampling: ``filtered_choice.filtered_sample_ref`` on the row with every entry outside A_c at -inf (the same token, margin
  and kept set as the rule's "rank, top-k, top-p within A_c, inverse CDF in index order");
* greedy: the first index of the largest logit within A_c;
* a row that holds a NaN or +inf (greedy: a NaN): the first index of A_c with the largest logit, NaN counting as the largest;
  a row whose A_c weights all round to 0 in the fp32 softmax of the WHOLE row: the unfiltered draw within A_c.

The state update: unchanged on the end index (the row is finished from then on), else ``next_state[s][token_class[token]]``.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filtered_choice import filtered_sample_ref, kernel_uniform  # noqa: E402,F401  (kernel_uniform: re-exported)
from token_choice import _first_allowed_argmax  # noqa: E402

_FP32_ZERO = 2.0 ** -150     # exp() below this rounds to 0 in fp32 ...
_FP32_NORMAL = 2.0 ** -126   # ... and below this it is subnormal: a kernel may or may not flush it


class Tables:
    """The three tables of a token automaton as int64 arrays, and the end index."""

    def __init__(self, automaton, end):
        self.token_class = np.asarray(automaton.token_class, dtype=np.int64)
        self.next_state = np.asarray(automaton.next_state, dtype=np.int64)
        self.min_left = np.asarray(automaton.min_left, dtype=np.int64)
        self.end = int(end)


def trivial_automaton():
    """One state, one class, accepting: it constrains nothing but the finished rows."""
    from types import SimpleNamespace

    return SimpleNamespace(token_class=None, next_state=np.zeros((1, 1), np.uint8), min_left=np.zeros(1, np.uint8))


def trivial_tables(V, end):
    a = trivial_automaton()
    a.token_class = np.zeros(V, np.uint8)
    return Tables(a, end), a


def allowed_mask(tab, state, finished, t, T, V, pad, unk, start):
    """A_c [N, V] (bool) of N rows in ``state`` [N] / ``finished`` [N] at step ``t`` of ``T``."""
    state = np.asarray(state, dtype=np.int64)
    finished = np.asarray(finished, dtype=bool)
    after = tab.next_state[state[:, None], tab.token_class[None, :V]]            # [N, V]
    mask = tab.min_left[after] <= T - 1 - t
    for j in (pad, unk, start, tab.end):
        if 0 <= j < V:
            mask[:, j] = False
    mask[finished] = False
    mask[:, tab.end] = finished | (tab.min_left[state] == 0)
    return mask


def advance(tab, state, finished, token):
    """(state, finished) of the rows behind ``token`` [N]."""
    state = np.asarray(state, dtype=np.int64)
    finished = np.asarray(finished, dtype=bool)
    token = np.asarray(token, dtype=np.int64)
    ended = token == tab.end
    moved = tab.next_state[state, tab.token_class[token]]
    return np.where(finished | ended, state, moved), finished | ended


def states_of(tab, tokens):
    """(state [B, T], finished [B, T]) BEFORE every step of the rows ``tokens`` [B, T]: rebuilt from the rows' own tokens."""
    tokens = np.asarray(tokens, dtype=np.int64)
    B, T = tokens.shape
    state, finished = np.zeros((B, T), np.int64), np.zeros((B, T), bool)
    s, f = np.zeros(B, np.int64), np.zeros(B, bool)
    for t in range(T):
        state[:, t], finished[:, t] = s, f
        s, f = advance(tab, s, f, tokens[:, t])
    return state, finished


def constrained_sample_ref(logits, u, mask, pad, unk, start, temperature=1.0, top_k=0, top_p=1.0):
    """(token [N], margin [N], kept [N, V]) of the constrained draw of every row of ``logits`` [N, V] whose allowed set is
    ``mask`` [N, V]; margin and kept set as ``filtered_sample_ref`` reports them."""
    z = np.asarray(logits, dtype=np.float64)
    N, V = z.shape
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), (N,))
    masked = np.where(mask, z, -np.inf)
    token, margin, kept = filtered_sample_ref(masked, u, pad, unk, start, temperature, top_k, top_p)
    token, margin, kept = token.copy(), margin.copy(), kept & mask
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        unfit = (np.isnan(z) | (z == np.inf)).any(1)
        zmax = z.max(1)
        lse = zmax + np.log(np.exp(z - zmax[:, None]).sum(1))
        p_top = np.exp(masked.max(1) - lse)  # the largest A_c weight in the softmax of the WHOLE row
    if unfit.any():  # the first index of A_c with the largest logit, NaN largest
        token[unfit] = _first_allowed_argmax(z[unfit], mask[unfit])
        margin[unfit] = np.inf
        kept[unfit] = mask[unfit]
    vanish = ~unfit & (p_top < _FP32_ZERO)
    if vanish.any():  # the A_c weights sum to 0 on the device: the same distribution, unfiltered
        token[vanish], margin[vanish], k = filtered_sample_ref(masked[vanish], u[vanish], pad, unk, start)
        kept[vanish] = k & mask[vanish]
    margin[~unfit & (p_top >= 2.0 ** -160) & (p_top < _FP32_NORMAL)] = 0.0  # (either rule may apply)
    return token, margin, kept


def constrained_greedy_ref(logits, mask):
    """The first index of the largest logit within ``mask`` of every row (NaN largest), and the gap between the two largest
    logits within the mask (0: an exact tie; inf: one allowed index; NaN with a NaN in the set)."""
    z = np.asarray(logits, dtype=np.float64)
    token = _first_allowed_argmax(z, mask)
    with np.errstate(invalid="ignore"):
        top2 = -np.sort(-np.where(mask, z, -np.inf), 1)[:, :2]
        gap = top2[:, 0] - top2[:, 1] if z.shape[1] > 1 else np.full(len(z), np.inf)
    gap = np.where(mask.sum(1) < 2, np.inf, gap)
    gap[(np.isnan(z) & mask).any(1)] = np.nan
    return token, gap


def cut_at_end(row, end):
    """The tokens of ``row`` before its first ``end`` (all of it without one)."""
    row = [int(x) for x in row]
    return row[:row.index(end)] if end in row else row
