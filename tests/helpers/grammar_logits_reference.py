"""Host reference of the grammar-masked logits (``pnmn_grammar_logits``; the rule: include/probnmn_grammar.h), numpy fp64.

Written from the rule, on ``constrained_choice.allowed_mask`` / ``advance``, not from device output.  A row starts in state
0, not finished, and walks its tokens.  At step t its set S_t is A_c(s_t, t) with ``T = horizon`` (for t >= horizon that is
@end@ alone, in an accepting state only; a finished row: @end@ alone); the step counts for ``outside`` when the row has not
finished, the token is not pad and the token is not in S_t; then the token, when it lies in [0, V), joins S_t, and a set that
is still empty stands for all of [0, V).  ``masked`` is the logit inside S_t and -inf outside, ``log_mass`` the lse over S_t
minus the lse over the row.  The state moves as the decoders move it; a token outside [0, V) leaves it alone.

``enumerate_leaves`` walks every string the rule allows from the start state: the support of q_c."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_choice as cc  # noqa: E402


def _lse(z, axis=-1):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(z, axis=axis, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return (m + np.log(np.exp(z - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def grammar_sets(tokens, tab, horizon, V, pad, unk, start):
    """(sets [B, T, V] bool, unmasked [B, T] bool, outside [B] int) of the rows ``tokens`` [B, T]."""
    tokens = np.asarray(tokens, dtype=np.int64)
    B, T = tokens.shape
    sets, unmasked, outside = np.zeros((B, T, V), bool), np.zeros((B, T), bool), np.zeros(B, np.int64)
    s, f = np.zeros(B, np.int64), np.zeros(B, bool)
    rows = np.arange(B)
    for t in range(T):
        mask = cc.allowed_mask(tab, s, f, t, horizon, V, pad, unk, start)
        tok = tokens[:, t]
        in_range = (tok >= 0) & (tok < V)
        safe = np.where(in_range, tok, 0)
        inside = in_range & mask[rows, safe]
        outside += ~f & (tok != pad) & ~inside
        mask[rows[in_range], tok[in_range]] = True
        unmasked[:, t] = ~mask.any(1)
        mask[unmasked[:, t]] = True
        sets[:, t] = mask
        s2, f2 = cc.advance(tab, s, f, safe)
        s, f = np.where(in_range, s2, s), np.where(in_range, f2, f)
    return sets, unmasked, outside


def grammar_logits_ref(logits, tokens, tab, horizon, pad, unk, start):
    """(masked [B, T, V] fp64, sets [B, T, V] bool, log_mass [B, T] fp64, outside [B] int64)."""
    z = np.asarray(logits, dtype=np.float64)
    V = z.shape[2]
    sets, unmasked, outside = grammar_sets(tokens, tab, horizon, V, pad, unk, start)
    masked = np.where(sets, z, -np.inf)
    log_mass = np.where(unmasked, 0.0, _lse(masked) - _lse(z))
    return masked, sets, log_mass, outside


def log_softmax_at(masked, tokens):
    """log_softmax(masked)[token] per (row, step), 0 where the token is outside [0, V)."""
    tokens = np.asarray(tokens, dtype=np.int64)
    V = masked.shape[2]
    ok = (tokens >= 0) & (tokens < V)
    picked = np.take_along_axis(masked, np.where(ok, tokens, 0)[..., None], 2)[..., 0]
    return np.where(ok, picked - _lse(masked), 0.0)


def sequence_nll_ref(masked, tokens, mask_tokens, pad, eps):
    """``sequence_nll`` in fp64: (loss [B], d loss.sum() / d masked [B, T, V])."""
    w = (np.asarray(mask_tokens) != pad).astype(np.float64)
    den = w.sum(1) + eps
    loss = -(log_softmax_at(masked, tokens) * w).sum(1) / den
    with np.errstate(invalid="ignore"):
        soft = np.exp(masked - _lse(masked)[..., None])
    onehot = np.zeros_like(soft)
    np.put_along_axis(onehot, np.asarray(tokens, dtype=np.int64)[..., None], 1.0, 2)
    return loss, (w / den[:, None])[..., None] * (soft - onehot)


def prefix_logits(prefix, V, seed=0):
    """Random logits of the step behind ``prefix`` (a tuple of tokens): a function of the prefix alone."""
    return np.random.default_rng([seed, len(prefix), *prefix]).normal(0.0, 2.0, V)


def enumerate_leaves(tab, horizon, V, pad, unk, start, seed=0):
    """Every string the rule allows from the start state, as (tokens, log q_c, ended): a leaf ends with @end@ at a step
    t < horizon (``ended``) or holds ``horizon`` tokens without one.  log q_c sums log_softmax over S_t of
    ``prefix_logits``."""
    leaves = []

    def walk(prefix, s, logq):
        t = len(prefix)
        if t == horizon:
            leaves.append((prefix, logq, False))
            return
        mask = cc.allowed_mask(tab, [s], [False], t, horizon, V, pad, unk, start)[0]
        assert mask.any(), "an allowed set ran empty"
        z = prefix_logits(prefix, V, seed)
        lse = _lse(np.where(mask, z, -np.inf))
        assert lse <= _lse(z) + 1e-12
        for v in np.flatnonzero(mask):
            if v == tab.end:
                leaves.append((prefix + (int(v),), logq + z[v] - lse, True))
            else:
                walk(prefix + (int(v),), int(tab.next_state[s, tab.token_class[v]]), logq + z[v] - lse)

    walk((), 0, 0.0)
    return leaves
