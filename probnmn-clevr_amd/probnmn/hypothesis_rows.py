"""The layout of hypothesis rows, stated once: R program hypotheses of G questions lie in ``question_rows`` [R] order --
non-decreasing, in 0 .. G - 1; hypothesis r belongs to question ``question_rows[r]`` and a question may have none -- which
is what ``group_hypotheses`` returns and what ``pnmn_answer_marginal``, ``pnmn_hypothesis_posterior`` and
``pnmn_answer_posterior`` read as ``group_start`` [G + 1]: question g owns rows group_start[g] .. group_start[g + 1].
``NeuralModuleNetwork.marginal_answers`` / ``answer_posterior`` and ``evaluators.hypothesis_posterior`` take their arguments
through here.  ``queue_hypotheses`` / ``awaited_hypotheses`` are the two stages that turn a generator pass into such rows --
the evaluators (``probnmn.evaluators``), marginal-likelihood module training (``probnmn.trainers.module_training``) and joint
marginal-likelihood training (``probnmn.trainers.marginal_training``) share them.  Of the layout functions only ``group_start_on_device`` and ``row_vector`` touch a device."""
from typing import Any, Dict

import numpy as np
import torch

from probnmn import _hip


def on_host(question_rows) -> np.ndarray:
    """``question_rows`` (a sequence, an array, a host or device tensor) as a contiguous host int64 array."""
    return np.ascontiguousarray(torch.as_tensor(question_rows).detach().cpu().numpy(), dtype=np.int64)


def check(qrows: np.ndarray, n_groups: int) -> None:
    """``ValueError`` unless the host rows [R] are non-decreasing and in 0 .. n_groups - 1."""
    if qrows.size and (int(qrows.min()) < 0 or int(qrows.max()) >= n_groups or bool((np.diff(qrows) < 0).any())):
        raise ValueError("question_rows must be non-decreasing and in 0 .. %d" % (n_groups - 1))


def group_start(qrows: np.ndarray, n_groups: int) -> np.ndarray:
    """Host int64 [n_groups + 1]: question g owns rows group_start[g] .. group_start[g + 1] of checked ``qrows``."""
    return np.searchsorted(qrows, np.arange(n_groups + 1))


def group_start_on_device(qrows: np.ndarray, n_groups: int, device: torch.device) -> torch.Tensor:
    """``group_start`` as the kernels read it: int32 [n_groups + 1] on the device, uploaded without a synchronisation."""
    return _hip.small_to_device(group_start(qrows, n_groups).tolist(), torch.int32, device)


def row_vector(values, name: str, n_rows: int, device: torch.device) -> torch.Tensor:
    """One number per hypothesis row (``log_weights``, ``log_q``) as contiguous fp32 [n_rows] on the device."""
    vector = torch.as_tensor(values).detach().to(device=device, dtype=torch.float32).contiguous()
    if tuple(vector.shape) != (n_rows,):
        raise ValueError("%s [%d]; got %s" % (name, n_rows, tuple(vector.shape)))
    return vector


def group_hypotheses(tokens, log_weights, valid):
    """The hypotheses of a batch of questions as the rows ``NeuralModuleNetwork.marginal_answers`` takes.  Host numpy:
    ``tokens`` [B, K, T] (K programs per question), ``log_weights`` [B, K] or None (uniform), ``valid`` [B, K].

    Per question: hypotheses that are invalid or have a weight that is not finite are dropped, identical token rows are
    merged in first-occurrence order, the merged log-weight being the logsumexp of the merged rows' (``log count`` for
    uniform weights).  A trained generator's samples are mostly the same program: merging is what keeps the NMN near B
    rows instead of B * K.  Returns (programs int64 [R, T], question_rows int64 [R] -- non-decreasing; a question with
    nothing left has no row --, log_weights float64 [R], first_slot int64 [R]: the slot k a merged row first appeared in)."""
    tokens = np.asarray(tokens)
    if tokens.ndim != 3:
        raise ValueError("tokens [B, K, T]; got shape %s" % (tokens.shape,))
    B, K, T = tokens.shape
    valid = np.asarray(valid).reshape(B, K) != 0
    weights = np.zeros((B, K)) if log_weights is None else np.asarray(log_weights, dtype=np.float64).reshape(B, K)
    keep = valid & np.isfinite(weights)
    programs, question_rows, merged, first_slot = [], [], [], []
    for b in range(B):
        seen: Dict[bytes, int] = {}
        for k in np.nonzero(keep[b])[0].tolist():
            row = np.ascontiguousarray(tokens[b, k], dtype=np.int64)
            at = seen.setdefault(row.tobytes(), len(programs))
            if at == len(programs):
                programs.append(row)
                question_rows.append(b)
                merged.append([weights[b, k]])
                first_slot.append(k)
            else:
                merged[at].append(weights[b, k])
    out_weights = np.zeros(len(programs))
    for i, w in enumerate(merged):
        w = np.asarray(w)
        out_weights[i] = w.max() + np.log(np.exp(w - w.max()).sum())
    return (np.stack(programs).astype(np.int64) if programs else np.zeros((0, T), np.int64),
            np.asarray(question_rows, dtype=np.int64), out_weights, np.asarray(first_slot, dtype=np.int64))


class HostCopies:
    """Device tensors copied into page-locked buffers, two sets in turn (batch i + 1 is queued before batch i is read)."""

    def __init__(self):
        self._pinned: Dict[Any, torch.Tensor] = {}

    def copy(self, name, iteration, t):
        key = (name, iteration & 1, tuple(t.shape), t.dtype)
        if key not in self._pinned:
            self._pinned[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        self._pinned[key].copy_(t, non_blocking=True)
        return self._pinned[key]


def queue_hypotheses(program_generator, batch, iteration, copies, beam_size, num_programs, constraint, constrained_sampling,
                     sampling, on_device, without_replacement=None):
    """First stage of a marginal batch: the generator pass that yields K hypotheses per question and the asynchronous copy
    of them to the host.  Returns (tokens [B, K, T], log-weights [B, K] or None, event or None, perturbed [B, K] or None).
    ``without_replacement`` ("probability" / "importance", or None): the ``num_programs`` hypotheses are ONE stochastic beam
    search's, weighted by their log-probabilities or by ``without_replacement_weights``."""
    question = batch["question"]
    perturbed = None
    if without_replacement is not None:
        extra = {} if constraint is None else {"constraint": constraint}
        out = program_generator(question, decoding_strategy="stochastic_beam", beam_size=num_programs, **extra)
        tokens, weights, perturbed = out["beam_predictions"], out["beam_log_probabilities"], out["beam_perturbed"]
        if without_replacement == "importance":
            from probnmn.evaluators import without_replacement_weights  # (evaluators imports this module)

            weights = without_replacement_weights(weights, perturbed)
    elif num_programs is not None:  # every question num_programs times in ONE call: the rows draw independently
        repeated = question.repeat_interleave(num_programs, 0)
        if constrained_sampling:
            out = program_generator(repeated, decoding_strategy="constrained_sampling", constraint=constraint, **sampling)
        else:
            out = program_generator(repeated, **sampling)
        tokens = out["predictions"]
        tokens, weights = tokens.reshape(question.size(0), num_programs, tokens.size(-1)), None
    else:
        extra = {} if constraint is None else {"constraint": constraint}
        out = program_generator(question, decoding_strategy="beam", beam_size=beam_size, **extra)
        tokens, weights = out["beam_predictions"], out["beam_log_probabilities"]
    if not (tokens.is_cuda and on_device):
        return tokens, weights, None, perturbed
    tokens = copies.copy("tokens", iteration, tokens)
    if weights is not None:
        weights = copies.copy("weights", iteration, weights)
    if perturbed is not None:
        perturbed = copies.copy("perturbed", iteration, perturbed)
    copied = torch.cuda.Event()
    copied.record()
    return tokens, weights, copied, perturbed


def awaited_hypotheses(nmn, queued, rerank=None):
    """What ``queue_hypotheses`` queued, awaited and grouped: wait for the copy, keep the valid hypotheses (merged:
    ``group_hypotheses``) and, with ``rerank`` = (question_reconstructor, program_prior, coefficients, questions [B, Tq]),
    replace their weights by their posterior under the generative model (``hypothesis_posterior``, the merged generator
    weight as its ``log_q``).  Returns (B, programs [R, T], question_rows [R], log-weights [R] -- host float64, or reranked
    the device ``"log_posterior"`` --, first_slot [R], reranked ``hypothesis_posterior``'s ``"log_reconstruction"``,
    ``"log_prior"`` and ``"best_row"`` as device tensors, else ``{}``)."""
    tokens, weights, copied, _ = queued
    if copied is not None:
        copied.synchronize()
    arr = tokens.cpu().numpy()
    B, K, T = arr.shape
    valid = np.array([c.valid for c in nmn.engine.compiler.compile_batch(arr.reshape(B * K, T))], dtype=bool).reshape(B, K)
    programs, question_rows, log_weights, first_slot = group_hypotheses(arr, None if weights is None else weights.cpu().numpy(),
                                                                        valid)
    scored = {}
    if rerank is not None:
        from probnmn.evaluators import hypothesis_posterior  # (evaluators imports this module)

        question_reconstructor, program_prior, coefficients, questions = rerank
        posterior = hypothesis_posterior(question_reconstructor, program_prior, questions, torch.from_numpy(programs),
                                         question_rows, log_q=log_weights, weights=coefficients)
        log_weights = posterior["log_posterior"]
        scored = {k: posterior[k] for k in ("log_reconstruction", "log_prior", "best_row")}
    return B, programs, question_rows, log_weights, first_slot, scored
