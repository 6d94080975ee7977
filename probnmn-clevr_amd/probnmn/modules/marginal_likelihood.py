"""The marginal likelihood over a question's candidate programs as a loss whose SEQUENCE terms are trained (not in the
reference, which trains the program generator by REINFORCE on one sampled program: modules/elbo.py):
    loss[g] = -log sum_r exp(w_x lp_x[r] + w_z lp_z[r] + w_q log_q[r])        over the rows r of group g
with lp_k[r] the teacher-forced log-probability (a true sum over the row's tokens) of row r under the logits of term k.  The
loss, the posterior over the rows and d loss / d logits of both terms come from ONE launch: ``pnmn_hypothesis_posterior`` in
gradient mode (include/probnmn_hip.h) -- a step's cross-entropy gradient scaled by its row's posterior share."""
from typing import Optional, Sequence, Tuple

import torch

from probnmn import _hip

Term = Tuple[torch.Tensor, torch.Tensor, int]  # (logits fp32 [R, T, V], tokens int64 [R, T], pad)


def _coefficients(weights) -> Tuple[float, float, float]:
    import math

    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError("weights must be three finite numbers (w_x, w_z, w_q), got %r" % (weights,))
    if len(w) != 3 or not all(math.isfinite(v) for v in w):
        raise ValueError("weights must be three finite numbers (w_x, w_z, w_q), got %r" % (weights,))
    return w


class _SequenceMarginalLoss(torch.autograd.Function):
    """``x_logits`` / ``z_logits`` fp32 [R, T, V] or None, ``log_q`` fp32 [R] or None, all contiguous and on the device;
    ``x_tokens`` / ``z_tokens`` int64 [R, T] (any row stride); ``group_start`` int32 [G + 1] on the device
    (``hypothesis_rows.group_start``: from 0 to R, non-decreasing).  Returns ``loss`` fp32 [G] = -log_evidence --
    ``INVALID_PROGRAM_LOSS``, without a gradient, where no row of the group counts -- and, not differentiable,
    ``log_posterior`` fp32 [R] and ``support`` int32 [G].  A gradient buffer is asked of the kernel only for a term whose logits
    require one; when nothing does (``log_q`` needs none from the kernel: its gradient is -w_q exp(log_posterior)) the launch
    is the plain one, which reports the same bits."""

    @staticmethod
    def forward(ctx, x_logits, x_tokens, pad_x, z_logits, z_tokens, pad_z, log_q, group_start, w_x, w_z, w_q):
        from probnmn.models.nmn import INVALID_PROGRAM_LOSS

        given = [t for t in (x_logits, z_logits, log_q) if t is not None]
        dev, R = given[0].device, int(given[0].size(0))
        G = int(group_start.numel()) - 1
        f = dict(dtype=torch.float32, device=dev)
        log_posterior, log_evidence = torch.full((R,), -float("inf"), **f), torch.full((G,), -float("inf"), **f)
        support = torch.zeros(G, dtype=torch.int32, device=dev)
        # (zero-filled: a row that no group covers is not written)
        d_x = torch.zeros_like(x_logits) if x_logits is not None and ctx.needs_input_grad[0] else None
        d_z = torch.zeros_like(z_logits) if z_logits is not None and ctx.needs_input_grad[3] else None
        ctx.buffers = (d_x is not None, d_z is not None)
        if R > 0 and G > 0:
            def term(logits, tokens):
                if logits is None:
                    return (0, 0, 0), (0, 0)
                return (logits.data_ptr(), tokens.data_ptr(), tokens.stride(0)), (logits.size(1), logits.size(2))

            x_args, (Tx, Vx) = term(x_logits, x_tokens)
            z_args, (Tz, Vz) = term(z_logits, z_tokens)
            plain = d_x is None and d_z is None
            best_row = torch.empty(G, dtype=torch.int32, device=dev) if plain else None
            _hip.check(_hip.lib().pnmn_hypothesis_posterior(
                *x_args, *z_args, 0 if log_q is None else log_q.data_ptr(), group_start.data_ptr(), w_x, w_z, w_q,
                int(pad_x), int(pad_z), 0 if d_x is None else d_x.data_ptr(), 0 if d_z is None else d_z.data_ptr(),
                log_posterior.data_ptr(), log_evidence.data_ptr(), best_row.data_ptr() if plain else 0, support.data_ptr(),
                G, R, Tx, Vx, Tz, Vz, _hip.stream_ptr(dev)), "hypothesis_posterior" + ("" if plain else " (gradient mode)"))
        loss = torch.where(support > 0, -log_evidence, torch.full_like(log_evidence, INVALID_PROGRAM_LOSS))
        # the group of every row: how many groups end at or before it
        group_of_row = torch.searchsorted(group_start[1:].long(), torch.arange(R, device=dev), right=True).clamp_(max=max(G - 1, 0))
        ctx.w_q = w_q
        ctx.save_for_backward(d_x, d_z, log_posterior, group_of_row)
        ctx.mark_non_differentiable(log_posterior, support)
        return loss, log_posterior, support

    @staticmethod
    def backward(ctx, dloss, *_):
        d_x, d_z, log_posterior, group_of_row = ctx.saved_tensors
        scale = dloss[group_of_row] if dloss.numel() else dloss.new_zeros(group_of_row.shape)
        g_x = d_x * scale.view(-1, 1, 1) if d_x is not None else None
        g_z = d_z * scale.view(-1, 1, 1) if d_z is not None else None
        g_q = None
        if ctx.needs_input_grad[6]:
            # (exp(-inf) = 0: a row that does not count gets exactly 0 -- and no 0 * inf with a scale that is not finite)
            share = torch.exp(log_posterior)
            g_q = torch.where(share > 0, -ctx.w_q * share * scale, torch.zeros_like(share))
        return g_x, None, None, g_z, None, None, g_q, None, None, None, None


def sequence_marginal_loss(x: Optional[Term] = None, z: Optional[Term] = None, log_q: Optional[torch.Tensor] = None, *,
                           group_start: torch.Tensor, weights: Sequence[float] = (1.0, 1.0, 1.0)):
    """``x`` / ``z``: (logits fp32 [R, T, V], tokens int64 [R, T], pad) or None -- the teacher-forced logits of a sequence
    model over the R candidate rows and the tokens they score; ``log_q`` fp32 [R] or None: any further log-score of a row
    (the answer's log-likelihood under the row's program, say).  ``group_start`` int32 [G + 1] on the device; ``weights`` =
    (w_x, w_z, w_q), finite; a term that is None, or whose coefficient is exactly 0, is left out of the score and gets a
    gradient of zeros.  Returns (``loss`` fp32 [G], ``log_posterior`` fp32 [R], ``support`` int32 [G]): see
    ``_SequenceMarginalLoss``.  Gradients reach ``x``'s logits, ``z``'s logits and ``log_q``, whichever require one."""
    w_x, w_z, w_q = _coefficients(weights)
    if x is None and z is None and log_q is None:
        raise ValueError("nothing to score the rows with: no x, no z and no log_q")
    if group_start.dtype != torch.int32 or group_start.dim() != 1 or group_start.numel() < 1:
        raise ValueError("group_start int32 [G + 1]; got %s %s" % (group_start.dtype, tuple(group_start.shape)))
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

    x_logits, x_tokens, pad_x = term(x, "x")
    z_logits, z_tokens, pad_z = term(z, "z")
    if log_q is not None:
        if log_q.dim() != 1 or log_q.dtype != torch.float32:
            raise ValueError("log_q fp32 [R]; got %s %s" % (log_q.dtype, tuple(log_q.shape)))
        rows.add(int(log_q.size(0)))
        log_q = log_q.contiguous()
    if len(rows) != 1:
        raise ValueError("x, z and log_q must have the same number of rows; got %s" % sorted(rows))
    dev = next(t for t in (x_logits, z_logits, log_q) if t is not None).device
    if dev.type != "cuda" or group_start.device != dev:
        raise _hip.HipLibraryError("sequence_marginal_loss runs on the ROCm device its inputs are on (got %s and %s); there is "
                                   "no CPU path" % (dev, group_start.device))
    return _SequenceMarginalLoss.apply(x_logits, x_tokens, pad_x, z_logits, z_tokens, pad_z, log_q, group_start.contiguous(),
                                       w_x, w_z, w_q)
