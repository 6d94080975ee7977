"""``pnmn_hypothesis_posterior``'s GRADIENT MODE restated in fp64 numpy (include/probnmn_hip.h states the contract), on top
of ``hypothesis_posterior_reference``: the loss of group g is -log_evidence[g], and its gradient with respect to the logits
of a sequence term is the row's per-step cross-entropy gradient scaled by the row's posterior share."""
import numpy as np

from hypothesis_posterior_reference import hypothesis_posterior_reference


def _term_gradient(term, w, share):
    """d(-log_evidence) / d logits of one term: fp64 [R, T, V].  ``share`` [R] = exp(log_posterior), 0 for a row that is not
    usable.  Zeros for padding steps, for rows that are not usable and for a coefficient of exactly 0; a logit of -inf gets 0."""
    logits, tokens, pad = term
    logits = np.asarray(logits, dtype=np.float64)
    tokens = np.asarray(tokens, dtype=np.int64)
    R, T, V = logits.shape
    d = np.zeros((R, T, V))
    if w == 0.0:
        return d
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in np.nonzero(share > 0)[0]:
            for t in range(T):
                tok = int(tokens[r, t])
                if tok == pad:
                    continue
                z = logits[r, t]
                m = z.max()
                prob = np.where(np.isneginf(z), 0.0, np.exp((z - m) - np.log(np.exp(z - m).sum())))
                hit = np.zeros(V)
                hit[tok] = 1.0  # (a usable row: every scored token is an index)
                d[r, t] = np.where(np.isneginf(z), 0.0, w * share[r] * (prob - hit))
    return d


def sequence_marginal_reference(x, z, log_q, group_start, weights, n_rows=None):
    """The arguments of ``hypothesis_posterior_reference``.  Returns its dict and ``d_x_logits`` fp64 [R, Tx, Vx] /
    ``d_z_logits`` fp64 [R, Tz, Vz] (None for a term not given) and ``d_log_q`` fp64 [R] (None without ``log_q``), the
    gradients of sum_g -log_evidence[g] over the supported groups: share_k[r] (softmax - one_hot) with share_k[r] = w_k
    exp(log_posterior[r]), and -w_q exp(log_posterior[r]).  Exact zeros where the contract says so (rows that are not usable,
    padding steps, logits of -inf, a coefficient of 0); rows no group covers are zeros here (the kernel does not write them:
    see ``covered``)."""
    ref = hypothesis_posterior_reference(x, z, log_q, group_start, weights, n_rows=n_rows)
    w_x, w_z, w_q = (float(w) for w in weights)
    with np.errstate(invalid="ignore"):
        share = np.where(ref["usable"] & np.isfinite(ref["log_posterior"]), np.exp(ref["log_posterior"]), 0.0)
    ref["d_x_logits"] = None if x is None else _term_gradient(x, w_x, share)
    ref["d_z_logits"] = None if z is None else _term_gradient(z, w_z, share)
    ref["d_log_q"] = None if log_q is None else -w_q * share
    return ref
