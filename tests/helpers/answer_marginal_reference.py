"""``pnmn_answer_marginal`` restated in fp64 numpy (include/probnmn_hip.h states the contract): the marginal answer
distribution of each group of hypothesis rows, sum_r w_r softmax(logits[r]), in log space."""
import numpy as np


def _logsumexp(x: np.ndarray, axis=None) -> np.ndarray:
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def answer_marginal_reference(logits, valid, log_weight, group_start, unknown_index):
    """logits [R, A]; valid [R] or None; log_weight [R] or None; group_start [G + 1] (any integers: clamped as the kernel
    clamps them).  Returns a dict: log_marginal fp64 [G, A], predictions int64 [G], row_predictions int64 [R], row_weight
    fp64 [R], support int32 [G] and ``covered`` bool [R] -- the rows some group holds, i.e. the rows the kernel writes."""
    logits = np.asarray(logits, dtype=np.float64)
    R, A = logits.shape
    start = np.asarray(group_start, dtype=np.int64)
    G = start.size - 1
    ok = np.ones(R, bool) if valid is None else np.asarray(valid) != 0
    usable = ok.copy()
    if log_weight is not None:
        log_weight = np.asarray(log_weight, dtype=np.float64)
        usable &= np.isfinite(log_weight)
    log_marginal = np.full((G, A), -np.inf)
    predictions = np.full(G, unknown_index, np.int64)
    support = np.zeros(G, np.int32)
    row_weight = np.zeros(R)
    covered = np.zeros(R, bool)
    row_predictions = np.where(ok, logits.argmax(1) if R else np.zeros(0, np.int64), unknown_index).astype(np.int64)
    log_softmax = logits - _logsumexp(logits, axis=1)[:, None] if R else logits
    for g in range(G):
        lo = min(max(int(start[g]), 0), R)
        hi = max(min(max(int(start[g + 1]), 0), R), lo)
        covered[lo:hi] = True
        rows = np.arange(lo, hi)[usable[lo:hi]]
        support[g] = rows.size
        if rows.size == 0:
            continue
        lw = np.zeros(rows.size) if log_weight is None else log_weight[rows]
        log_w = lw - _logsumexp(lw)
        row_weight[rows] = np.exp(log_w)
        log_marginal[g] = _logsumexp(log_w[:, None] + log_softmax[rows], axis=0)
        predictions[g] = int(log_marginal[g].argmax())
    return {"log_marginal": log_marginal, "predictions": predictions, "row_predictions": row_predictions,
            "row_weight": row_weight, "support": support, "covered": covered}


def top_two_margin(log_marginal: np.ndarray, support: np.ndarray) -> float:
    """Smallest gap between the best and the second-best answer over the supported groups (inf when A == 1 or none is)."""
    rows = np.asarray(log_marginal)[np.asarray(support) > 0]
    if rows.shape[0] == 0 or rows.shape[1] < 2:
        return float("inf")
    top = np.sort(rows, axis=1)[:, -2:]
    return float((top[:, 1] - top[:, 0]).min())
