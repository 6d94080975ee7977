"""Host reference of the filtered token choice (temperature, top-k, top-p), numpy only, fp64.

Written from the filter rule stated beside ``pnmn_sample_tokens`` in include/probnmn_hip.h, not from device output.
For one row of logits z and the filter (temperature, top_k, top_p):

* the allowed set A is every index but pad, unk and start; ``s_j = z_j / temperature``, ``w_j = exp(s_j - max_A s)``;
* j ranks before i when ``w_j > w_i``, or ``w_j == w_i`` and ``j < i``;
* ``top_k > 0`` keeps the ``top_k`` first-ranked indices; ``top_p < 1`` keeps, of those, index i iff the weight of the kept
  indices ranked before it is ``< top_p * total`` (total = what top-k kept), and always the first-ranked index;
* the draw is the index-order inverse CDF over the kept weights from the uniform of ``token_choice.kernel_uniform``;
* a row that holds a NaN or +inf, whose allowed logits are all -inf, or whose allowed softmax weights all round to 0 in
  fp32 (the unfiltered rule's total is then 0) ignores the filter: ``token_choice.sample_ref`` answers for it.

The kernels work in fp32, so a row may legitimately come out differently when it sits within round-off of one of the
rule's decisions.  ``filtered_sample_ref`` reports how far the row is from the nearest one (its margin), the smallest of
  1. the CDF margin of ``sample_ref`` taken over the kept weights: |u * total - inner boundary| / total;
  2. the gap in s between the last index top-k keeps and the first it drops;
  3. min over the indices inside the top-k cut of |mass before i / total - top_p|;
  4. the gap in s between the last index top-p keeps and the first it drops: two almost equal weights at the nucleus'
     edge may rank either way in fp32, which swaps WHICH of them is kept although no mass crosses top_p.
An exact tie (gap 0) is no ambiguity: equal logits give equal fp32 weights and the lower index ranks first on both sides.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from token_choice import kernel_uniform, sample_ref  # noqa: E402,F401  (kernel_uniform: re-exported for the tests)

_FP32_ZERO = 2.0 ** -150     # exp() below this rounds to 0 in fp32 (half the smallest subnormal) ...
_FP32_NORMAL = 2.0 ** -126   # ... and below this it is subnormal: a kernel may or may not flush it


def _allowed(N, V, pad, unk, start):
    allowed = np.ones((N, V), dtype=bool)
    for j in (pad, unk, start):
        if 0 <= j < V:
            allowed[:, j] = False
    return allowed


def ranks_within_allowed(logits, pad, unk, start, temperature):
    """rank [N, V] of every index within the allowed set of its row (0 = first ranked; indices that are not allowed rank
    behind all of them), by the rule above."""
    z = np.asarray(logits, dtype=np.float64)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    N, V = z.shape
    allowed = _allowed(N, V, pad, unk, start)
    with np.errstate(invalid="ignore", over="ignore"):
        key = np.where(allowed, z / temperature, -np.inf)
        key = np.where(allowed, np.nan_to_num(key, nan=-np.inf, posinf=np.inf, neginf=-1e300), -np.inf)
    order = np.argsort(-key, 1, kind="stable")  # (stable: equal weights keep index order)
    rank = np.empty((N, V), dtype=np.int64)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(V), (N, V)), 1)
    return rank


def filtered_sample_ref(logits, u, pad, unk, start, temperature=1.0, top_k=0, top_p=1.0):
    """(token [N], margin [N], kept [N, V] bool) of every row of ``logits`` [N, V] for the uniforms ``u`` [N].  ``kept`` is
    the set the draw is made from (for a row that ignores the filter: its allowed set, or all of it if nothing is allowed);
    the margin is described in the module docstring (inf where nothing depends on round-off)."""
    z = np.asarray(logits, dtype=np.float64)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    N, V = z.shape
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), (N,))
    allowed = _allowed(N, V, pad, unk, start)
    token, margin = sample_ref(z, u, pad, unk, start)
    token, margin = token.copy(), margin.copy()
    kept = np.where(allowed.any(1, keepdims=True), allowed, True)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        finite_row = ~(np.isnan(z) | (z == np.inf)).any(1)
        top_allowed = np.where(allowed, z, -np.inf).max(1)
        zmax = z.max(1)
        lse = zmax + np.log(np.exp(z - zmax[:, None]).sum(1))
        p_top = np.exp(top_allowed - lse)  # the largest allowed softmax weight of the UNMODIFIED distribution
    filtered = finite_row & np.isfinite(top_allowed) & (p_top >= _FP32_ZERO)
    # (between "rounds to 0" and "normal" the unfiltered total may or may not be 0 on the device: either rule may apply)
    either = finite_row & np.isfinite(top_allowed) & (p_top >= 2.0 ** -160) & (p_top < _FP32_NORMAL)
    margin[either] = 0.0
    rows = np.flatnonzero(filtered)
    if rows.size == 0:
        return token, margin, kept
    zf, af, uf = z[rows], allowed[rows], u[rows]
    n = rows.size
    s = np.where(af, zf / temperature, -np.inf)
    w = np.where(af, np.exp(s - s.max(1, keepdims=True)), 0.0)
    rank = ranks_within_allowed(zf, pad, unk, start, temperature)
    order = np.argsort(rank, 1)  # order[:, r] = the index of rank r
    n_allowed = af.sum(1)
    k_eff = n_allowed if top_k <= 0 else np.minimum(top_k, n_allowed)
    ws = np.take_along_axis(w, order, 1)
    ss = np.take_along_axis(s, order, 1)
    r = np.arange(V)[None, :]
    in_k = r < k_eff[:, None]
    wk = np.where(in_k, ws, 0.0)
    total = wk.sum(1)
    before = np.cumsum(wk, 1) - wk
    keep_sorted = in_k.copy()
    m_rule = np.full(n, np.inf)

    def gap_at(cut):
        """s of the last rank kept minus s of the first rank dropped, where ranks [0, cut) are kept of k_eff candidates;
        inf where nothing is dropped or the two tie exactly."""
        has = (cut >= 1) & (cut < n_allowed)
        c = np.clip(cut, 1, V - 1)
        with np.errstate(invalid="ignore"):
            g = ss[np.arange(n), c - 1] - ss[np.arange(n), c]
        g = np.where(np.isnan(g) | (g == 0.0), np.inf, g)
        return np.where(has, g, np.inf)

    if top_k > 0:
        m_rule = np.minimum(m_rule, gap_at(k_eff))
    if top_p < 1.0:
        keep_sorted &= (before < top_p * total[:, None]) | (r == 0)
        dist = np.where(in_k, np.abs(before / total[:, None] - top_p), np.inf)
        m_rule = np.minimum(m_rule, dist.min(1))
        m_rule = np.minimum(m_rule, gap_at(keep_sorted.sum(1)))
    kept_f = np.zeros((n, V), dtype=bool)
    np.put_along_axis(kept_f, order, keep_sorted, 1)
    # the draw: index-order inverse CDF over the kept weights (the scan of token_choice.sample_ref)
    wd = np.where(kept_f, w, 0.0)
    cdf = np.cumsum(wd, 1)
    tot = cdf[:, -1:]
    target = uf[:, None] * tot
    hit = (wd > 0) & (cdf > target)
    tok = hit.argmax(1)
    pos = wd > 0
    none_hit = ~hit.any(1)  # (u * total rounds past the end: the last positive weight)
    tok[none_hit] = (V - 1 - pos[none_hit][:, ::-1].argmax(1))
    inner = pos & (np.arange(V)[None, :] > pos.argmax(1)[:, None])
    m_cdf = np.where(inner, np.abs((cdf - wd) - target) / tot, np.inf).min(1)
    token[rows] = tok
    margin[rows] = np.where(either[rows], 0.0, np.minimum(m_cdf, m_rule))
    kept[rows] = kept_f
    return token, margin, kept
