"""``pnmn_importance_bound_joint`` restated in fp64 numpy (include/probnmn_importance_joint.h states the contract): the terms
and the weight of ``importance_bound_reference`` with the answer term added to log w afterwards,
    log w = (lx + beta (lp - lq)) + gamma la,     la = log_softmax(a_logits[r])[answers[g]]
-- ``invalid_log_answer`` for an invalid row, -inf for an answer that is no index or whose logit is -inf; left out entirely
for gamma == 0 --, then per question the same statistics (``question_statistics``), and the gradients of the four logits
tensors."""
import numpy as np

from importance_bound_reference import cross_entropy_gradient, importance_bound_reference, logsumexp, question_statistics


def answer_log_likelihood(a_logits, answers, valid, samples, invalid_log_answer, unknown_index=0):
    """(la fp64 [R], first arg-max int64 [R]) of the contract: row r scores answers[r // samples]."""
    z = np.asarray(a_logits, dtype=np.float64)
    R, A = z.shape
    la, predictions = np.empty(R), np.empty(R, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(R):
            if valid is not None and valid[r] == 0:
                la[r], predictions[r] = invalid_log_answer, unknown_index
                continue
            predictions[r] = int(np.argmax(z[r]))          # (numpy's arg-max is the first one)
            a = int(answers[r // samples])
            value = z[r, a] - logsumexp(z[r]) if 0 <= a < A else -np.inf
            la[r] = value if np.isfinite(value) else -np.inf
    return la, predictions


def importance_joint_reference(x, q, p, beta, samples, answer, answer_weight=1.0, invalid_log_answer=None, unknown_index=0,
                               gradients=False):
    """``x`` / ``q`` / ``p``, ``beta``, ``samples``: as for ``importance_bound_reference``.  ``answer`` = (logits [R, A],
    answers [G], valid [R] or None).  ``invalid_log_answer`` None: -log A.  Returns ``importance_bound_reference``'s dict
    with the joint weight in it, plus log_pa fp64 [R], row_predictions int64 [R]; ``scale`` [G] is the largest |lx| +
    gamma |la| + beta (|lp| + |lq|) over the question's rows (finite terms that enter); with ``gradients`` also d_a [R, A]
    and coefficient_a [R] = gamma share (0 for an invalid row and for a question that does not count)."""
    beta, gamma, K = float(beta), float(answer_weight), int(samples)
    a_logits, answers, valid = answer
    a_logits = np.asarray(a_logits, dtype=np.float64)
    R, A = a_logits.shape
    G = R // K
    assert G * K == R and len(answers) == G
    if invalid_log_answer is None:
        invalid_log_answer = -np.log(A)
    base = importance_bound_reference(x, q, p, beta, K, gradients=gradients)
    la, predictions = answer_log_likelihood(a_logits, answers, valid, K, invalid_log_answer, unknown_index)
    out = dict(base, log_pa=la, row_predictions=predictions)
    if gamma == 0.0:     # the term is left out entirely: nothing it holds rules a row out
        if gradients:
            out["d_a"], out["coefficient_a"] = np.zeros((R, A)), np.zeros(R)
        return out
    whole = np.isfinite(base["log_weight"]) & np.isfinite(la)
    with np.errstate(invalid="ignore"):
        log_w = np.where(whole, base["log_weight"] + gamma * la, -np.inf)
    size = gamma * np.where(np.isfinite(la), np.abs(la), 0.0)
    # (the existing reference reports the largest size of the other terms per question, not per row: recompute per row)
    size += _row_size(base, beta)
    share, signal = np.zeros(R), np.zeros(R)
    bound, ess = np.full(G, -np.inf), np.zeros(G)
    support, scale = np.zeros(G, np.int32), np.zeros(G)
    for g in range(G):
        rows = slice(g * K, (g + 1) * K)
        support[g] = int(whole[rows].sum())
        scale[g] = size[rows].max()
        if support[g] == K:
            bound[g], share[rows], ess[g], signal[rows] = question_statistics(log_w[rows])
    out.update(log_weight=log_w, share=share, signal=signal, bound=bound, ess=ess, support=support, scale=scale)
    if gradients:
        counts = np.repeat(support == K, K)
        c_x = np.where(counts, share, 0.0)
        c_q = np.where(counts, signal - beta * share, 0.0)
        out["coefficient_x"], out["coefficient_q"] = c_x, c_q
        out["d_x"] = c_x[:, None, None] * cross_entropy_gradient(*x)
        out["d_q"] = c_q[:, None, None] * cross_entropy_gradient(*q)
        if p is not None:
            use_p = beta != 0.0
            c_p = beta * c_x if use_p else np.zeros(R)
            out["coefficient_p"] = c_p
            out["d_p"] = c_p[:, None, None] * cross_entropy_gradient(*p) if use_p else np.zeros(np.asarray(p[0]).shape)
        usable = counts if valid is None else counts & (np.asarray(valid) != 0)
        c_a = np.where(usable, gamma * share, 0.0)
        row_answers = np.repeat(np.asarray(answers, np.int64), K)
        ce = cross_entropy_gradient(a_logits[:, None, :], np.where(usable, row_answers, -1)[:, None], -1)[:, 0, :]
        out["coefficient_a"], out["d_a"] = c_a, c_a[:, None] * ce
    return out


def _row_size(base, beta):
    """|lx| + beta (|lp| + |lq|) of every row over the finite terms that enter, as ``importance_bound_reference`` sizes them."""
    size = np.where(np.isfinite(base["log_px"]), np.abs(base["log_px"]), 0.0)
    if beta != 0.0:
        size = size + beta * np.where(np.isfinite(base["log_q"]), np.abs(base["log_q"]), 0.0)
        if base["log_pz"] is not None:
            size = size + beta * np.where(np.isfinite(base["log_pz"]), np.abs(base["log_pz"]), 0.0)
    return size
