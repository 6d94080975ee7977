"""Host statement of the multi-sample ELBO estimator with the leave-one-out baseline, in fp64 numpy: what
the leave-one-out kernel of ``pnmn_joint_objective`` and the CPU path of ``probnmn.modules.elbo.*.combine`` are held to.

K programs are drawn per question; the N = n_questions * K sampled rows are question-major (row q * K + k).  Per row, with
the models' negative log-likelihoods pg, qr, prior, nmn (the reference's arithmetic, elbo.py:28-34,76-82,253-270):

    logq = -pg ; rec = -qr ; R = rec + beta * (-prior) - beta * logq + gamma * (-nmn)
    S_q = sum_k R_k ;  c_i = R_i - (S_q - R_i) / (K - 1)          (the mean reward of the question's OTHER samples)
    kl = logq * c - beta * logq ;  elbo = rec - kl

    J = w_u (gamma mean(nmn) - mean(elbo)) + w_s alpha (mean(pg_sup) + mean(qr_sup))
    dJ/dpg[i] = -w_u (c_i - beta) / N ; dJ/dqr[i] = w_u / N ; dJ/dnmn[i] = w_u gamma / N     (R is a constant)
    dJ/dpg_sup[j] = dJ/dqr[N + j] = w_s alpha / m
    reward_variance = mean_q sum_k (R_k - S_q / K)^2 / (K - 1)
"""
import numpy as np


def leave_one_out_centre(R, samples):
    """c[q, k] = R[q, k] - mean of the question's other samples, for R of shape [n_questions, samples] (or flat).

    Written as the mean of the differences to the other samples, sum_{j != k} (R_k - R_j) / (K - 1): the same number as
    R_k - (S_q - R_k) / (K - 1), but every difference of equal rewards is an exact zero, so a group of equal rewards centres
    to exactly 0 whatever the value (through S_q, 3 R rounds before R is taken off again and one ulp is left over).

    The PRODUCT paths -- the kernel and ``probnmn.modules.elbo.leave_one_out_rows`` -- keep the S_q form and do NOT have
    that property: for equal rewards they may return c of one ulp of R, not 0.  Nothing may rely on an exact zero there."""
    R = np.asarray(R, np.float64).reshape(-1, samples)
    return (R[:, :, None] - R[:, None, :]).sum(2) / (samples - 1)


def loo_objective_reference(pg, qr, prior, nmn, pg_sup, w_u, w_s, alpha, beta, gamma, n_questions, samples, m):
    """Everything the kernel returns, from the per-row losses (array-likes; ``prior`` / ``nmn`` / ``pg_sup`` may be None;
    ``qr`` holds the N sampled rows followed by the m supervised ones)."""
    if not 2 <= samples <= 64:
        raise ValueError("samples must be 2 .. 64")
    f = lambda x, k: np.zeros(k) if x is None else np.asarray(x, np.float64).reshape(-1)[:k]  # noqa: E731
    N = n_questions * samples
    qr = np.zeros(0) if qr is None else np.asarray(qr, np.float64).reshape(-1)
    pg, pr, nm, pgs = f(pg, N), f(prior, N), f(nmn, N), f(pg_sup, m)
    assert qr.size == N + m and pg.size == N and pgs.size == m
    logq, rec = -pg, -qr[:N]
    R = rec + beta * (-pr) - beta * logq + gamma * (-nm)
    c = leave_one_out_centre(R, samples).reshape(-1)
    kl = logq * c - beta * logq
    elbo = rec - kl
    mean = lambda x: float(x.mean()) if x.size else 0.0  # noqa: E731
    Rq = R.reshape(-1, samples)
    variance = ((Rq - Rq.mean(1, keepdims=True)) ** 2).sum(1) / (samples - 1)
    J = w_u * (gamma * mean(nm) - mean(elbo)) + w_s * alpha * (mean(pgs) + mean(qr[N:]))
    stats = {"reconstruction_likelihood": mean(rec), "kl_divergence": mean(kl), "elbo": mean(elbo), "reinforce_reward": mean(R),
             "nmn_loss": mean(nm), "sum_centred": float(c.sum()), "program_generation_gt": mean(pgs),
             "question_reconstruction_gt": mean(qr[N:]), "reward_variance": mean(variance)}
    d_qr = np.concatenate((np.full(N, w_u / max(N, 1)), np.full(m, w_s * alpha / max(m, 1))))
    grads = {"pg": -w_u * (c - beta) / max(N, 1), "qr": d_qr, "nmn": np.full(N, w_u * gamma / max(N, 1)),
             "pg_sup": np.full(m, w_s * alpha / max(m, 1))}
    return {"J": J, "stats": stats, "grads": grads, "R": R, "c": c, "kl": kl, "elbo": elbo}
