"""``pnmn_importance_bound`` restated in fp64 numpy (include/probnmn_importance.h states the contract): per row the three
sequence log-probabilities as ``hypothesis_posterior_reference`` computes them and log w = lx + beta (lp - lq); per question
of K rows the bound logsumexp(log w) - log K, every row's share, the effective sample size and the VIMCO learning signal, the
leave-one-out terms by direct sums over the other rows; the gradients of the three logits tensors."""
import numpy as np

from hypothesis_posterior_reference import sequence_log_likelihood


def logsumexp(v):
    v = np.asarray(v, dtype=np.float64)
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def question_statistics(log_w):
    """One question's K finite log-weights -> (bound, share [K], ess, signal [K]): the contract's formulas, the baseline of
    sample k from the other K - 1 values only."""
    v = np.asarray(log_w, dtype=np.float64)
    K = v.size
    lse = logsumexp(v)
    bound = lse - np.log(K)
    share = np.exp(v - lse)
    ess = 1.0 / (share ** 2).sum()
    if K == 1:
        return bound, share, ess, np.array([bound])
    signal = np.empty(K)
    for k in range(K):
        others = np.delete(v, k)
        m = others.max()
        baseline = m + np.log(np.exp(others - m).sum() + np.exp(others.mean() - m)) - np.log(K)
        signal[k] = bound - baseline
    return bound, share, ess, signal


def cross_entropy_gradient(logits, tokens, pad):
    """ce [R, T, V] fp64: softmax(logits[r][t]) - onehot(token) on the steps whose token is an index and not ``pad``, zeros on
    the others; a logit of -inf gets exactly 0."""
    logits = np.asarray(logits, dtype=np.float64)
    R, T, V = logits.shape
    ce = np.zeros((R, T, V))
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(R):
            for t in range(T):
                tok = int(tokens[r, t])
                if tok == pad or not 0 <= tok < V:
                    continue
                z = logits[r, t]
                prob = np.exp(z - logsumexp(z))
                prob[tok] -= 1.0
                prob[np.isneginf(z)] = 0.0
                ce[r, t] = prob
    return ce


def importance_bound_reference(x, q, p, beta, samples, gradients=False):
    """``x`` / ``q`` / ``p``: (logits [R, T, V], tokens [R, T], pad), ``p`` or None; R = G ``samples``.  The prior's term is
    left out when ``p`` is None or ``beta`` == 0; with ``beta`` == 0 the generator's leaves log w as well.  log w is -inf when
    a term that enters is not finite.  Returns a dict: log_px, log_q fp64 [R], log_pz (None when left out), log_weight,
    share, signal [R], bound, ess [G], support int32 [G], ``scale`` [G] (max over the question's rows of |lx| + beta (|lp| +
    |lq|) over the finite terms that enter: what the tolerance of a comparison scales with) and, with ``gradients``, d_x, d_p
    (zeros when left out; None without ``p``), d_q, coefficient_x / _p / _q [R]."""
    beta, K = float(beta), int(samples)
    lx, lq = sequence_log_likelihood(*x), sequence_log_likelihood(*q)
    use_p = p is not None and beta != 0.0
    lp = sequence_log_likelihood(*p) if use_p else None
    R = lx.size
    G = R // K
    assert G * K == R
    whole = np.isfinite(lx)
    size = np.where(np.isfinite(lx), np.abs(lx), 0.0)
    log_w = lx.copy()
    with np.errstate(invalid="ignore"):
        if beta != 0.0:
            whole &= np.isfinite(lq)
            log_w = log_w - beta * lq
            size += beta * np.where(np.isfinite(lq), np.abs(lq), 0.0)
        if use_p:
            whole &= np.isfinite(lp)
            log_w = log_w + beta * lp
            size += beta * np.where(np.isfinite(lp), np.abs(lp), 0.0)
    log_w = np.where(whole, log_w, -np.inf)
    share, signal = np.zeros(R), np.zeros(R)
    bound, ess = np.full(G, -np.inf), np.zeros(G)
    support = np.zeros(G, np.int32)
    scale = np.zeros(G)
    for g in range(G):
        rows = slice(g * K, (g + 1) * K)
        support[g] = int(whole[rows].sum())
        scale[g] = size[rows].max()
        if support[g] == K:
            bound[g], share[rows], ess[g], signal[rows] = question_statistics(log_w[rows])
    out = {"log_px": lx, "log_pz": lp, "log_q": lq, "log_weight": log_w, "share": share, "signal": signal, "bound": bound,
           "ess": ess, "support": support, "scale": scale}
    if gradients:
        counts = np.repeat(support == K, K)
        c_x = np.where(counts, share, 0.0)
        c_q = np.where(counts, signal - beta * share, 0.0)
        out["coefficient_x"], out["coefficient_q"] = c_x, c_q
        out["d_x"] = c_x[:, None, None] * cross_entropy_gradient(*x)
        out["d_q"] = c_q[:, None, None] * cross_entropy_gradient(*q)
        out["d_p"] = out["coefficient_p"] = None
        if p is not None:
            c_p = beta * c_x if use_p else np.zeros(R)
            out["coefficient_p"] = c_p
            out["d_p"] = c_p[:, None, None] * cross_entropy_gradient(*p) if use_p else np.zeros(np.asarray(p[0]).shape)
    return out
