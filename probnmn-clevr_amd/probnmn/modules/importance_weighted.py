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

    def term(t, name):
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

    if x is None or q is None:
        raise ValueError("the bound needs the reconstructor's term x and the generator's term q")
    x_logits, x_tokens, pad_x = term(x, "x")
    q_logits, q_tokens, pad_q = term(q, "q")
    p_logits, p_tokens, pad_p = term(p, "p")
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
