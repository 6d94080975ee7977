"""The importance-weighted bound on log p(x) over K programs sampled per question (Burda et al. 2016), trained with the
VIMCO estimator of a discrete latent (Mnih & Rezende 2016).  Not in the reference, whose ELBO scores one sampled program per
question through per-token MEAN losses (modules/elbo.py), so that it neither tightens with more samples nor bounds log p(x):

    log w_r  = log p(x_g | z_r) + beta (log p(z_r) - log q(z_r | x_g))          row r = g K + k, every term a SUM over tokens
    loss[g]  = -bound[g] = -(logsumexp_k(log w) - log K)

The loss, the per-row statistics, d loss / d logits of the reconstructor's and the prior's term and the VIMCO estimate for the
generator's come from ONE launch: ``pnmn_importance_bound`` (include/probnmn_importance.h).  The generator's gradient is an
ESTIMATOR -- (signal_r - beta share_r) grad log q(z_r | x), unbiased for the gradient of E[bound] when the rows were drawn
from q -- not the derivative of the reported loss."""
import math
from typing import Dict, Optional, Tuple

import torch

from probnmn import _hip, _hip_importance
from probnmn.modules.marginal_likelihood import Term

MAX_SAMPLES = 64  # (one lane of a wavefront per sample of a question)


def check_samples(samples, least: int = 1) -> int:
    """``samples`` as an integer in ``least`` .. 64; ``ValueError`` otherwise."""
    if isinstance(samples, bool) or not isinstance(samples, int) or not least <= samples <= MAX_SAMPLES:
        raise ValueError("samples must be an integer in %d .. %d, got %r" % (least, MAX_SAMPLES, samples))
    return samples


def check_beta(beta) -> float:
    """``beta`` as a finite float that is not negative; ``ValueError`` otherwise."""
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError("beta must be a finite number that is not negative, got %r" % (beta,))
    if isinstance(beta, bool) or not math.isfinite(b) or b < 0.0:
        raise ValueError("beta must be a finite number that is not negative, got %r" % (beta,))
    return b


def _checked_term(t, name, rows):
    """One term as the kernel takes it -- (contiguous logits, tokens with unit step stride, pad) or (None, None, 0) -- its row
    count added to ``rows``; ``ValueError`` for what is no (logits fp32 [R, T, V], tokens int64 [R, T], pad)."""
    if t is None:
        return None, None, 0
    logits, tokens, pad = t
    if logits.dim() != 3 or logits.dtype != torch.float32 or tokens.dim() != 2 or tokens.dtype != torch.long \
            or tuple(tokens.shape) != tuple(logits.shape[:2]) or tokens.device != logits.device:
        raise ValueError("%s = (logits fp32 [R, T, V], tokens int64 [R, T], pad); got %s %s and %s %s"
                         % (name, logits.dtype, tuple(logits.shape), tokens.dtype, tuple(tokens.shape)))
    if logits.size(0) and (logits.size(1) < 1 or logits.size(2) < 1):
        raise ValueError("%s: at least one step and one token; got %s" % (name, tuple(logits.shape)))
    rows.add(int(logits.size(0)))
    if tokens.size(1) and tokens.stride(1) != 1:
        tokens = tokens.contiguous()
    return logits.contiguous(), tokens, int(pad)


class _ImportanceWeightedBound(torch.autograd.Function):
    """``x_logits`` / ``q_logits`` fp32 [R, T, V], ``p_logits`` likewise or None, contiguous and on the device; the tokens
    int64 [R, T] (any row stride); R = G ``samples``.  Returns ``loss`` fp32 [G] = -bound -- ``INVALID_PROGRAM_LOSS``,
    without a gradient, for a question without full support -- and, not differentiable, log_weight, share, signal [R], ess
    [G], support int32 [G], log_px, log_pz, log_q [R] (log_pz NaN when the prior term is left out).  A gradient buffer is
    asked of the kernel only for a term whose logits require one; when none does the launch is the plain one, which reports
    the same bits."""

    @staticmethod
    def forward(ctx, x_logits, x_tokens, pad_x, p_logits, p_tokens, pad_p, q_logits, q_tokens, pad_q, beta, samples):
        from probnmn.models.nmn import INVALID_PROGRAM_LOSS

        dev, R = x_logits.device, int(x_logits.size(0))
        G = R // samples
        f = dict(dtype=torch.float32, device=dev)
        rows = {k: torch.empty(R, **f) for k in ("log_weight", "share", "signal", "log_px", "log_q")}
        rows["log_pz"] = torch.full((R,), float("nan"), **f)
        bound, ess = torch.empty(G, **f), torch.empty(G, **f)
        support = torch.empty(G, dtype=torch.int32, device=dev)
        # (not filled first: in gradient mode the kernel writes every word of the rows [0, R))
        d_x = torch.empty_like(x_logits) if ctx.needs_input_grad[0] else None
        d_p = torch.empty_like(p_logits) if p_logits is not None and ctx.needs_input_grad[3] else None
        d_q = torch.empty_like(q_logits) if ctx.needs_input_grad[6] else None
        ctx.samples = samples
        if G > 0:
            def term(logits, tokens, pad):
                if logits is None:
                    return 0, 0, 0, 0, 0, 0
                return logits.data_ptr(), tokens.data_ptr(), tokens.stride(0), int(pad), logits.size(1), logits.size(2)

            ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
            plain = d_x is None and d_p is None and d_q is None
            _hip.check(_hip_importance.lib().pnmn_importance_bound(
                *term(x_logits, x_tokens, pad_x), *term(p_logits, p_tokens, pad_p), *term(q_logits, q_tokens, pad_q),
                beta, G, samples, ptr(rows["log_px"]), ptr(rows["log_pz"]), ptr(rows["log_q"]), ptr(rows["log_weight"]),
                ptr(rows["share"]), ptr(rows["signal"]), ptr(bound), ptr(ess), ptr(support), ptr(d_x), ptr(d_p), ptr(d_q),
                _hip.stream_ptr(dev)), "importance_bound" + ("" if plain else " (gradient mode)"))
        loss = torch.where(support == samples, -bound, torch.full_like(bound, INVALID_PROGRAM_LOSS))
        ctx.save_for_backward(d_x, d_p, d_q)
        others = (rows["log_weight"], rows["share"], rows["signal"], ess, support, rows["log_px"], rows["log_pz"], rows["log_q"])
        ctx.mark_non_differentiable(*others)
        return (loss,) + others

    @staticmethod
    def backward(ctx, dloss, *_):
        d_x, d_p, d_q = ctx.saved_tensors
        # (a question without full support: its gradient rows are zeros, whatever its dloss)
        scale = dloss.repeat_interleave(ctx.samples).view(-1, 1, 1)
        g = [None if d is None else d * scale for d in (d_x, d_p, d_q)]
        return g[0], None, None, g[1], None, None, g[2], None, None, None, None


def importance_weighted_bound(x: Term, q: Term, p: Optional[Term] = None, *, samples: int,
                              beta: float = 1.0) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``x``, ``q``, ``p``: (logits fp32 [R, T, V], tokens int64 [R, T], pad) -- the teacher-forced logits of the
    reconstructor, the generator and (or None) the prior over the R = G ``samples`` sampled rows, question-major, and the
    tokens they score.  ``samples`` in 1 .. 64; ``beta`` finite, not negative: the weight of log p(z) - log q(z | x) in log w
    (0, or ``p`` None, leaves the prior's term out entirely; 0 leaves the generator's out of log w as well, and its gradient
    is then signal grad log q alone).

    Returns (``loss`` fp32 [G] = -bound, ``stats``): ``stats`` holds detached tensors -- ``log_weight``, ``share`` (a row's
    share of its question's weight), ``signal`` (the bound minus the row's leave-one-out baseline; the bound itself for one
    sample), ``log_px``, ``log_pz`` (NaN when the term is left out), ``log_q`` fp32 [R]; ``ess`` fp32 [G] (1 / sum share^2);
    ``support`` int32 [G] (rows with a finite log w).  A question counts when all its rows do; otherwise it pays
    ``INVALID_PROGRAM_LOSS`` without a gradient and its share, signal and ess are 0.  Gradients reach the three logits
    tensors, whichever require one: exact for ``x`` and ``p``, the VIMCO estimate for ``q``."""
    samples, beta = check_samples(samples), check_beta(beta)
    rows = set()
    if x is None or q is None:
        raise ValueError("the bound needs the reconstructor's term x and the generator's term q")
    x_logits, x_tokens, pad_x = _checked_term(x, "x", rows)
    q_logits, q_tokens, pad_q = _checked_term(q, "q", rows)
    p_logits, p_tokens, pad_p = _checked_term(p, "p", rows)
    if len(rows) != 1:
        raise ValueError("x, q and p must have the same number of rows; got %s" % sorted(rows))
    R = rows.pop()
    if R % samples:
        raise ValueError("%d rows are not a whole number of questions of %d samples" % (R, samples))
    devices = {t.device for t in (x_logits, q_logits, p_logits) if t is not None}
    dev = x_logits.device
    if dev.type != "cuda" or len(devices) != 1:
        raise _hip.HipLibraryError("importance_weighted_bound runs on the ROCm device its inputs are on (got %s); there is "
                                   "no CPU path" % sorted(str(d) for d in devices))
    out = _ImportanceWeightedBound.apply(x_logits, x_tokens, pad_x, p_logits, p_tokens, pad_p, q_logits, q_tokens, pad_q,
                                         beta, samples)
    names = ("log_weight", "share", "signal", "ess", "support", "log_px", "log_pz", "log_q")
    return out[0], dict(zip(names, out[1:]))


# ---- with the answer term: the bound on log p(x, a | image) of joint training ------------------------------------------------

def check_answer_weight(answer_weight) -> float:
    """``answer_weight`` as a finite float that is not negative; ``ValueError`` otherwise."""
    try:
        w = float(answer_weight)
    except (TypeError, ValueError):
        raise ValueError("answer_weight must be a finite number that is not negative, got %r" % (answer_weight,))
    if isinstance(answer_weight, bool) or not math.isfinite(w) or w < 0.0:
        raise ValueError("answer_weight must be a finite number that is not negative, got %r" % (answer_weight,))
    return w


def check_invalid_log_answer(invalid_log_answer, num_answers: int) -> float:
    """log p(a | an invalid program): None is -log A (an invalid program answers uniformly; at A = 28 that is -3.332, the
    reference's constant loss 3.33 before rounding); otherwise a number <= 0 or -inf, which rules out the question of every
    invalid row.  ``ValueError`` for a NaN, a positive value or what is no number."""
    if invalid_log_answer is None:
        return -math.log(num_answers) if num_answers > 0 else 0.0
    try:
        v = float(invalid_log_answer)
    except (TypeError, ValueError):
        raise ValueError("invalid_log_answer must be None, a number <= 0 or -inf, got %r" % (invalid_log_answer,))
    if isinstance(invalid_log_answer, bool) or not v <= 0.0:
        raise ValueError("invalid_log_answer must be None, a number <= 0 or -inf, got %r" % (invalid_log_answer,))
    return v


class _JointImportanceWeightedBound(torch.autograd.Function):
    """``_ImportanceWeightedBound`` with the answer term: ``a_logits`` fp32 [R, A] contiguous, ``answers`` int64 [G],
    ``valid`` int32 [R] or None, on the device of the rest.  Returns what ``_ImportanceWeightedBound`` returns, then
    ``log_pa`` fp32 [R] and ``row_predictions`` int64 [R]; a fourth gradient buffer, for the answer logits, is asked of the
    kernel only when they require one."""

    @staticmethod
    def forward(ctx, x_logits, x_tokens, pad_x, p_logits, p_tokens, pad_p, q_logits, q_tokens, pad_q, beta, samples, a_logits,
                answers, valid, answer_weight, invalid_log_answer, unknown_index):
        from probnmn import _hip_importance_joint
        from probnmn.models.nmn import INVALID_PROGRAM_LOSS

        dev, R = x_logits.device, int(x_logits.size(0))
        G = R // samples
        f = dict(dtype=torch.float32, device=dev)
        rows = {k: torch.empty(R, **f) for k in ("log_weight", "share", "signal", "log_px", "log_q", "log_pa")}
        rows["log_pz"] = torch.full((R,), float("nan"), **f)
        predictions = torch.empty(R, dtype=torch.long, device=dev)
        bound, ess = torch.empty(G, **f), torch.empty(G, **f)
        support = torch.empty(G, dtype=torch.int32, device=dev)
        # (not filled first: in gradient mode the kernel writes every word of the rows [0, R))
        d_x = torch.empty_like(x_logits) if ctx.needs_input_grad[0] else None
        d_p = torch.empty_like(p_logits) if p_logits is not None and ctx.needs_input_grad[3] else None
        d_q = torch.empty_like(q_logits) if ctx.needs_input_grad[6] else None
        d_a = torch.empty_like(a_logits) if ctx.needs_input_grad[11] else None
        ctx.samples = samples
        if G > 0:
            def term(logits, tokens, pad):
                if logits is None:
                    return 0, 0, 0, 0, 0, 0
                return logits.data_ptr(), tokens.data_ptr(), tokens.stride(0), int(pad), logits.size(1), logits.size(2)

            ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
            plain = d_x is None and d_p is None and d_q is None and d_a is None
            _hip.check(_hip_importance_joint.lib().pnmn_importance_bound_joint(
                *term(x_logits, x_tokens, pad_x), *term(p_logits, p_tokens, pad_p), *term(q_logits, q_tokens, pad_q),
                beta, G, samples, ptr(rows["log_px"]), ptr(rows["log_pz"]), ptr(rows["log_q"]), ptr(rows["log_weight"]),
                ptr(rows["share"]), ptr(rows["signal"]), ptr(bound), ptr(ess), ptr(support), ptr(d_x), ptr(d_p), ptr(d_q),
                a_logits.data_ptr(), ptr(valid), answers.data_ptr(), int(a_logits.size(1)), answer_weight, invalid_log_answer,
                int(unknown_index), ptr(rows["log_pa"]), predictions.data_ptr(), ptr(d_a), _hip.stream_ptr(dev)),
                "importance_bound_joint" + ("" if plain else " (gradient mode)"))
        loss = torch.where(support == samples, -bound, torch.full_like(bound, INVALID_PROGRAM_LOSS))
        ctx.save_for_backward(d_x, d_p, d_q, d_a)
        others = (rows["log_weight"], rows["share"], rows["signal"], ess, support, rows["log_px"], rows["log_pz"], rows["log_q"],
                  rows["log_pa"], predictions)
        ctx.mark_non_differentiable(*others)
        return (loss,) + others

    @staticmethod
    def backward(ctx, dloss, *_):
        d_x, d_p, d_q, d_a = ctx.saved_tensors
        # (a question without full support: its gradient rows are zeros, whatever its dloss)
        rows = dloss.repeat_interleave(ctx.samples)
        g = [None if d is None else d * rows.view(-1, 1, 1) for d in (d_x, d_p, d_q)]
        g_a = None if d_a is None else d_a * rows.view(-1, 1)
        return (g[0], None, None, g[1], None, None, g[2], None, None, None, None, g_a, None, None, None, None, None)


def joint_importance_weighted_bound(x: Term, q: Term, p: Optional[Term] = None, *, answer, samples: int, beta: float = 1.0,
                                    answer_weight: float = 1.0, invalid_log_answer: Optional[float] = None,
                                    unknown_index: int = 0) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``importance_weighted_bound`` with the answer inside the weight: the K-sample bound on log p(x, a | image),
        log w_r = log p(x_g | z_r) + beta (log p(z_r) - log q(z_r | x_g)) + answer_weight log p(a_g | z_r, image_g)
    from ONE ``pnmn_importance_bound_joint`` launch (include/probnmn_importance_joint.h).

    ``x``, ``q``, ``p``, ``samples``, ``beta``: as for ``importance_weighted_bound``.  ``answer`` = (logits fp32 [R, A] -- the
    module network's answer logits of every sampled row, ``NeuralModuleNetwork.hypothesis_answer_logits`` --, answers int64
    [G], ONE per question, valid int32 [R] or None: every row is a valid program).  ``answer_weight``: finite, not negative;
    exactly 0 leaves the answer out of log w (the statistics below are still reported).  ``invalid_log_answer``: log p(a | z)
    of a row whose program is invalid; None is -log A (such a program answers uniformly; 3.332 nats at A = 28, the
    reference's constant 3.33 before rounding), -inf rules the row's question out.  ``unknown_index``: the prediction
    reported for an invalid row.

    Returns (``loss`` fp32 [G] = -bound, ``stats``): ``stats`` is ``importance_weighted_bound``'s keys plus ``log_pa`` fp32
    [R] (-inf for an answer that is no index or whose logit is -inf) and ``row_predictions`` int64 [R] (each row's own
    answer).  A question counts when all its rows have a finite weight; otherwise it pays ``INVALID_PROGRAM_LOSS`` without a
    gradient.  Gradients reach the four logits tensors, whichever require one: exact for ``x``, ``p`` and the answer logits,
    the VIMCO estimate for ``q`` -- with share and signal those of the joint weight, so the generator learns from answers."""
    samples, beta, answer_weight = check_samples(samples), check_beta(beta), check_answer_weight(answer_weight)
    if x is None or q is None:
        raise ValueError("the bound needs the reconstructor's term x and the generator's term q")
    if not isinstance(answer, (tuple, list)) or len(answer) != 3:
        raise ValueError("answer = (logits fp32 [R, A], answers int64 [G], valid int32 [R] or None); got %r" % (type(answer),))
    a_logits, answers, valid = answer
    if not torch.is_tensor(a_logits) or a_logits.dim() != 2 or a_logits.dtype != torch.float32 or a_logits.size(1) < 1:
        raise ValueError("answer logits fp32 [R, A] with at least one answer; got %s"
                         % ("%s %s" % (a_logits.dtype, tuple(a_logits.shape)) if torch.is_tensor(a_logits) else type(a_logits)))
    R, A = int(a_logits.size(0)), int(a_logits.size(1))
    if A > 1024:
        raise ValueError("at most 1024 answers, got %d" % A)
    if R % samples:
        raise ValueError("%d rows are not a whole number of questions of %d samples" % (R, samples))
    if not torch.is_tensor(answers) or answers.dim() != 1 or answers.dtype != torch.long or answers.size(0) != R // samples:
        raise ValueError("answers int64 [%d], one per question; got %s"
                         % (R // samples, "%s %s" % (answers.dtype, tuple(answers.shape)) if torch.is_tensor(answers) else type(answers)))
    if valid is not None and (not torch.is_tensor(valid) or valid.dtype != torch.int32 or tuple(valid.shape) != (R,)):
        raise ValueError("valid int32 [%d] or None; got %s"
                         % (R, "%s %s" % (valid.dtype, tuple(valid.shape)) if torch.is_tensor(valid) else type(valid)))
    invalid_log_answer = check_invalid_log_answer(invalid_log_answer, A)
    if isinstance(unknown_index, bool) or not isinstance(unknown_index, int):
        raise ValueError("unknown_index must be an integer, got %r" % (unknown_index,))
    rows = {R}

    x_logits, x_tokens, pad_x = _checked_term(x, "x", rows)
    q_logits, q_tokens, pad_q = _checked_term(q, "q", rows)
    p_logits, p_tokens, pad_p = _checked_term(p, "p", rows)
    if len(rows) != 1:
        raise ValueError("x, q, p and the answer logits must have the same number of rows; got %s" % sorted(rows))
    devices = {t.device for t in (x_logits, q_logits, p_logits, a_logits, answers, valid) if t is not None}
    dev = x_logits.device
    if dev.type != "cuda" or len(devices) != 1:
        raise _hip.HipLibraryError("joint_importance_weighted_bound runs on the ROCm device its inputs are on (got %s); there "
                                   "is no CPU path" % sorted(str(d) for d in devices))
    out = _JointImportanceWeightedBound.apply(
        x_logits, x_tokens, pad_x, p_logits, p_tokens, pad_p, q_logits, q_tokens, pad_q, beta, samples, a_logits.contiguous(),
        answers.contiguous(), None if valid is None else valid.contiguous(), answer_weight, invalid_log_answer, unknown_index)
    names = ("log_weight", "share", "signal", "ess", "support", "log_px", "log_pz", "log_q", "log_pa", "row_predictions")
    return out[0], dict(zip(names, out[1:]))
