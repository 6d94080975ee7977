"""The generator's distribution renormalised over the program grammar, as a differentiable function of its logits.

``q_c(z | x) = prod_t softmax over A_c(s_t, t) of the step's logits``: the distribution the constrained sampler
(``decoding_strategy="constrained_sampling"``, unfiltered) draws from.  It sums to one over the programs of at most
``horizon`` tokens the token automaton accepts, so samples and targets scored under it make every estimator of the
trainers correct with every sample a valid program.  ``grammar_logits`` returns the logits with everything outside the
allowed set of each step at ``-inf``: ``log_softmax`` of them is ``log q_c``'s step term, and ``sequence_nll`` /
``sequence_marginal_loss`` take them as they take any logits.  The rule and the kernels: include/probnmn_grammar.h,
csrc/grammar_logits.hip (``pnmn_grammar_logits`` / ``pnmn_grammar_logits_bwd``)."""
import torch

from probnmn import _hip, _hip_grammar
from probnmn.modules.seq2seq_base import constraint_tables


def _rows(t: torch.Tensor, V: int) -> torch.Tensor:
    """[B, T, V] with unit column stride and step stride V (any row stride: ``logits[:, :-1]`` passes without a copy)."""
    return t if (t.stride(2) == 1 and t.stride(1) == V) else t.contiguous()


def _automaton_arguments(tables):
    tc, ns, ml, end = tables  # (host arrays: the library checks every entry and passes them by value)
    return end, tc.ctypes.data, ns.ctypes.data, ml.ctypes.data, ns.shape[0], ns.shape[1]


class _GrammarLogits(torch.autograd.Function):
    """``pnmn_grammar_logits`` / ``_bwd``: logits [B, T, V], tokens [B, T] -> (masked [B, T, V], log_mass [B, T], outside [B]);
    the gradient of ``masked`` is copied inside each step's set and 0 outside it."""

    @staticmethod
    def forward(ctx, logits, tokens, tables, horizon, pad, unk, start):
        B, T, V = logits.shape
        dev = logits.device
        logits = _rows(logits, V)
        if tokens.dtype != torch.long or (T > 1 and tokens.stride(1) != 1):
            tokens = tokens.long().contiguous()
        masked = torch.empty(B, T, V, dtype=torch.float32, device=dev)
        log_mass = torch.empty(B, T, dtype=torch.float32, device=dev)
        outside = torch.empty(B, dtype=torch.int32, device=dev)
        _hip.check(_hip_grammar.lib().pnmn_grammar_logits(
            logits.data_ptr(), logits.stride(0), tokens.data_ptr(), tokens.stride(0), masked.data_ptr(), T * V,
            log_mass.data_ptr(), outside.data_ptr(), B, T, V, horizon, pad, unk, start, *_automaton_arguments(tables),
            _hip.stream_ptr(dev)), "grammar_logits")
        ctx.save_for_backward(tokens)
        ctx.tables, ctx.args = tables, (horizon, pad, unk, start)
        ctx.mark_non_differentiable(log_mass, outside)
        return masked, log_mass, outside

    @staticmethod
    def backward(ctx, d_masked, _mass, _outside):
        (tokens,) = ctx.saved_tensors
        B, T, V = d_masked.shape
        d_masked = _rows(d_masked, V)
        d_logits = torch.empty(B, T, V, dtype=torch.float32, device=d_masked.device)
        _hip.check(_hip_grammar.lib().pnmn_grammar_logits_bwd(
            d_masked.data_ptr(), d_masked.stride(0), tokens.data_ptr(), tokens.stride(0), d_logits.data_ptr(), T * V,
            B, T, V, *ctx.args, *_automaton_arguments(ctx.tables), _hip.stream_ptr(d_masked.device)), "grammar_logits_bwd")
        return d_logits, None, None, None, None, None, None


def grammar_logits(logits: torch.Tensor, tokens: torch.Tensor, constraint, horizon: int, pad: int, unk: int, start: int,
                   end: int):
    """(masked [B, T, V], log_mass [B, T], outside [B]) of ``logits`` [B, T, V] fp32 along the rows ``tokens`` [B, T] (the
    token emitted or targeted at each step) under the token automaton ``constraint``
    (``ProgramCompiler.decoding_automaton``, or the tuple ``constraint_tables`` made of one) with ``horizon`` steps.

    ``masked``: the logit itself inside the step's allowed set -- with the step's own token added, so no target is ever at
    ``-inf`` -- and ``-inf`` outside it; differentiable in ``logits``.  ``log_mass`` (detached): the log of the share of the
    unconstrained step distribution inside the set, ``<= 0``; ``log q = log q_c + sum_t log_mass`` along a row.  ``outside``
    (detached, int32): steps at which an unfinished row's non-padding token was not in its allowed set -- 0 for every row
    the constrained sampler emits.  ``ValueError``: tables of another vocabulary size, a horizon the shortest accepted
    string does not fit; more than 128 tokens: ``NotImplementedError``."""
    if logits.device.type != "cuda":
        raise _hip.HipLibraryError("grammar_logits input on %s: the HIP path needs a ROCm device" % logits.device)
    if logits.dim() != 3 or tokens.dim() != 2 or tokens.shape != logits.shape[:2] or logits.dtype != torch.float32:
        raise ValueError("grammar_logits: logits fp32 [B, T, V] and tokens [B, T], got %s %s and %s"
                         % (logits.dtype, tuple(logits.shape), tuple(tokens.shape)))
    V = logits.size(2)
    tables = constraint if isinstance(constraint, tuple) else constraint_tables(constraint, V, end)
    check_horizon(tables, horizon)
    if V > 128:
        raise NotImplementedError("grammar_logits: %d target tokens -- the automaton tables cover at most 128" % V)
    masked, log_mass, outside = _GrammarLogits.apply(logits, tokens, tables, int(horizon), pad, unk, start)
    return masked, log_mass.detach(), outside.detach()


def check_horizon(tables, horizon: int) -> None:
    """``ValueError`` unless ``horizon`` is an int >= 1 in which the shortest string of the automaton ``tables``
    (``constraint_tables``) fits -- what the entry points refuse with ``PNMN_EINVAL``, said before the launch."""
    if isinstance(horizon, bool) or not isinstance(horizon, int) or horizon < 1:
        raise ValueError("horizon must be an int >= 1, got %r" % (horizon,))
    if int(tables[2][0]) > horizon:
        raise ValueError("constraint: the shortest accepted string takes %d tokens, the horizon is %d" % (int(tables[2][0]), horizon))


def scored_log_mass(log_mass: torch.Tensor, mask_tokens: torch.Tensor, pad: int) -> torch.Tensor:
    """[B]: the sum of ``log_mass`` [B, T] over the steps a sequence loss scores (``mask_tokens != pad``)."""
    return (log_mass * (mask_tokens != pad)).sum(1)
