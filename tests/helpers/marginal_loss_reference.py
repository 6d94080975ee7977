"""``pnmn_answer_posterior`` in gradient mode restated in fp64 numpy (include/probnmn_hip.h states the contract):
``answer_posterior_reference`` plus the gradient of the marginal-likelihood loss -log_evidence[g] with respect to the logits,
    d_logits[r][c] = w_a exp(log_posterior[r]) (softmax(logits[r])[c] - [c == answers[g]])      for a usable row r,
exactly 0 for a covered row that is not usable, and NaN for a row no group covers (the kernel does not write it)."""
import numpy as np

from answer_posterior_reference import answer_posterior_reference


def marginal_loss_reference(logits, valid, log_weight, answers, group_start, w_a, unknown_index):
    """The arguments of ``answer_posterior_reference``.  Returns its dict and ``"d_logits"`` fp64 [R, A]."""
    out = answer_posterior_reference(logits, valid, log_weight, answers, group_start, w_a, unknown_index)
    z = np.asarray(logits, dtype=np.float64)
    R, A = z.shape
    answers = np.asarray(answers, dtype=np.int64)
    start = np.asarray(group_start, dtype=np.int64)
    d = np.full((R, A), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for g in range(start.size - 1):
            lo = min(max(int(start[g]), 0), R)
            hi = max(min(max(int(start[g + 1]), 0), R), lo)
            a = int(answers[g])
            for r in range(lo, hi):
                d[r] = 0.0
                if not out["usable"][r] or float(w_a) == 0.0:
                    continue
                p = np.exp(z[r] - z[r].max())
                p /= p.sum()
                if 0 <= a < A:
                    p[a] -= 1.0
                d[r] = float(w_a) * np.exp(out["log_posterior"][r]) * p
                d[r][np.isneginf(z[r])] = 0.0  # (probability 0: gradient 0)
    out["d_logits"] = d
    return out
