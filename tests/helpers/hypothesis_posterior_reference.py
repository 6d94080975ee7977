"""``pnmn_hypothesis_posterior`` restated in fp64 numpy (include/probnmn_hip.h states the contract): per row the
log-likelihood of its tokens under teacher-forced logits, for the reconstructor's term (x) and the prior's (z); per group of
rows the posterior over the rows whose score w_x lp_x + w_z lp_z + w_q log_q is finite."""
import numpy as np


def sequence_log_likelihood(logits, tokens, pad):
    """logits [R, T, V], tokens [R, T] -> lp fp64 [R]: the sum over the steps whose token is not ``pad`` of
    (z[token] - max z) - log sum exp(z - max z); -inf for a row with a non-pad token outside [0, V); 0 for an all-pad row."""
    logits = np.asarray(logits, dtype=np.float64)
    tokens = np.asarray(tokens, dtype=np.int64)
    R, T, V = logits.shape
    lp = np.zeros(R)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(R):
            for t in range(T):
                tok = int(tokens[r, t])
                if tok == pad:
                    continue
                if not 0 <= tok < V:
                    lp[r] = -np.inf
                    break
                z = logits[r, t]
                m = z.max()
                lp[r] += (z[tok] - m) - np.log(np.exp(z - m).sum())
    return lp


def hypothesis_posterior_reference(x, z, log_q, group_start, weights, n_rows=None):
    """``x`` / ``z``: (logits [R, T, V], tokens [R, T], pad) or None; ``log_q`` [R] or None; ``group_start`` [G + 1] (any
    integers: clamped as the kernel clamps them); ``weights`` = (w_x, w_z, w_q).  A term whose input is None or whose
    coefficient is exactly 0 is left out of the score.  Returns a dict: log_px, log_pz fp64 [R] (None for a term not given),
    score fp64 [R], usable bool [R], log_posterior fp64 [R], log_evidence fp64 [G], best_row int32 [G], support int32 [G],
    ``covered`` bool [R] (the rows some group holds, i.e. the rows the kernel writes) and ``max_abs_score`` fp64 [G] (the
    largest |score| among the group's usable rows, 0 without any: what the tolerance of a comparison scales with)."""
    w_x, w_z, w_q = (float(w) for w in weights)
    lp_x = None if x is None else sequence_log_likelihood(*x)
    lp_z = None if z is None else sequence_log_likelihood(*z)
    R = n_rows if n_rows is not None else next(len(a) for a in (lp_x, lp_z, log_q) if a is not None)
    score = np.zeros(R)
    with np.errstate(invalid="ignore"):
        if lp_x is not None and w_x != 0.0:
            score = score + w_x * lp_x
        if lp_z is not None and w_z != 0.0:
            score = score + w_z * lp_z
        if log_q is not None and w_q != 0.0:
            score = score + w_q * np.asarray(log_q, dtype=np.float64)
    usable = np.isfinite(score)
    start = np.asarray(group_start, dtype=np.int64)
    G = start.size - 1
    log_posterior = np.full(R, -np.inf)
    log_evidence = np.full(G, -np.inf)
    best_row = np.full(G, -1, np.int32)
    support = np.zeros(G, np.int32)
    max_abs_score = np.zeros(G)
    covered = np.zeros(R, bool)
    for g in range(G):
        lo = min(max(int(start[g]), 0), R)
        hi = max(min(max(int(start[g + 1]), 0), R), lo)
        covered[lo:hi] = True
        rows = np.arange(lo, hi)[usable[lo:hi]]
        support[g] = rows.size
        if rows.size == 0:
            continue
        s = score[rows]
        m = s.max()
        log_norm = np.log(np.exp(s - m).sum())
        log_evidence[g] = m + log_norm
        log_posterior[rows] = (s - m) - log_norm
        best_row[g] = rows[int(s.argmax())]  # (the first maximum)
        max_abs_score[g] = np.abs(s).max()
    return {"log_px": lp_x, "log_pz": lp_z, "score": score, "usable": usable, "log_posterior": log_posterior,
            "log_evidence": log_evidence, "best_row": best_row, "support": support, "covered": covered,
            "max_abs_score": max_abs_score}


def top_two_score_margin(score, usable, group_start) -> np.ndarray:
    """Per group the gap between the largest and the second-largest usable score (inf with fewer than two usable rows);
    bounds clamped as above."""
    score, usable = np.asarray(score, dtype=np.float64), np.asarray(usable, dtype=bool)
    start = np.asarray(group_start, dtype=np.int64)
    R = score.size
    out = np.full(start.size - 1, np.inf)
    for g in range(start.size - 1):
        lo = min(max(int(start[g]), 0), R)
        hi = max(min(max(int(start[g + 1]), 0), R), lo)
        s = np.sort(score[lo:hi][usable[lo:hi]])
        if s.size >= 2:
            out[g] = s[-1] - s[-2]
    return out
