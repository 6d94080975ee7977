"""``pnmn_answer_posterior`` restated in fp64 numpy (include/probnmn_hip.h states the contract): per hypothesis row the
log-likelihood of its question's given answer and the row's own answer; per group of rows the posterior over the rows whose
score log_w + w_a log p(a | z, image) is finite."""
import numpy as np


def _logsumexp(x: np.ndarray) -> float:
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def answer_posterior_reference(logits, valid, log_weight, answers, group_start, w_a, unknown_index):
    """logits [R, A]; valid [R] or None; log_weight [R] or None; answers [G] (any integers: one outside [0, A) is never an
    index); group_start [G + 1] (any integers: clamped as the kernel clamps them); ``w_a`` finite -- exactly 0 leaves the
    answer term out.  Returns a dict: log_answer fp64 [R] (NaN for a row no group covers: there is no answer to score it
    against), row_predictions int64 [R], score fp64 [R], usable bool [R], log_posterior fp64 [R], log_evidence fp64 [G],
    best_row, support, consistent_count, first_consistent int32 [G], ``covered`` bool [R] (the rows some group holds, i.e. the
    rows the kernel writes) and ``max_abs_score`` fp64 [G] (the largest |score| among the group's usable rows, 0 without any:
    what the tolerance of a comparison scales with).  A row that several groups cover holds the last one's values."""
    logits = np.asarray(logits, dtype=np.float64)
    R, A = logits.shape
    answers = np.asarray(answers, dtype=np.int64)
    start = np.asarray(group_start, dtype=np.int64)
    G = start.size - 1
    w_a = float(w_a)
    ok = np.ones(R, bool) if valid is None else np.asarray(valid) != 0
    base = ok.copy()
    if log_weight is not None:
        log_weight = np.asarray(log_weight, dtype=np.float64)
        base &= np.isfinite(log_weight)
    row_predictions = np.where(ok, logits.argmax(1) if R else np.zeros(0, np.int64), unknown_index).astype(np.int64)
    log_answer = np.full(R, np.nan)
    score = np.full(R, -np.inf)
    usable = np.zeros(R, bool)
    log_posterior = np.full(R, -np.inf)
    log_evidence = np.full(G, -np.inf)
    best_row = np.full(G, -1, np.int32)
    first_consistent = np.full(G, -1, np.int32)
    support = np.zeros(G, np.int32)
    consistent_count = np.zeros(G, np.int32)
    max_abs_score = np.zeros(G)
    covered = np.zeros(R, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(G):
            lo = min(max(int(start[g]), 0), R)
            hi = max(min(max(int(start[g + 1]), 0), R), lo)
            covered[lo:hi] = True
            a = int(answers[g])
            for r in range(lo, hi):
                z = logits[r]
                log_answer[r] = (z[a] - z.max()) - np.log(np.exp(z - z.max()).sum()) if 0 <= a < A else -np.inf
            rows = np.arange(lo, hi)[base[lo:hi]]
            usable[lo:hi] = False
            score[lo:hi] = -np.inf
            log_posterior[lo:hi] = -np.inf
            if rows.size:
                log_w = (log_weight[rows] - _logsumexp(log_weight[rows])) if log_weight is not None else np.full(rows.size, -np.log(rows.size))
                s = log_w + w_a * log_answer[rows] if w_a != 0.0 else log_w
                score[rows] = s
                usable[rows] = np.isfinite(s)
                rows = rows[np.isfinite(s)]
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
            agree = rows[row_predictions[rows] == a]
            consistent_count[g] = agree.size
            if agree.size:
                first_consistent[g] = agree[0]
    return {"log_answer": log_answer, "row_predictions": row_predictions, "score": score, "usable": usable,
            "log_posterior": log_posterior, "log_evidence": log_evidence, "best_row": best_row, "support": support,
            "consistent_count": consistent_count, "first_consistent": first_consistent, "covered": covered,
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
