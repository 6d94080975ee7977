"""Validation and inference loops over the MI355X models, as the reference runs them (reference:
probnmn/evaluators/_evaluator.py:67-115 and the four phase evaluators; scripts/inference.py:76-91).

Stand-alone layout only (when the models are grafted onto the reference's package, its own
``probnmn.evaluators`` keeps working on them).  Semantics kept:
  * models in ``eval()`` mode, no gradients, back to ``train()`` afterwards;
  * the loop stops when the batch counter EXCEEDS ``num_batches`` -- it sees ``num_batches + 2`` batches;
  * the ProgramGenerator is called WITH the ground-truth programs as targets and "greedy" decoding, so its
    predictions are the arg-max of the teacher-forced distributions (seq2seq_base.py:188-198), and the NMN
    answers on those; accuracy = #(prediction == answer) / N (an invalid program predicts @@UNKNOWN@@);
  * inference samples programs (``program_generator(question)`` with the default strategy, in eval mode)
    and lets the NMN answer without gold answers; with ``beam_size`` it beam-searches them instead (not in the
    reference) and can prefer the best-ranked hypothesis that is a valid program; with ``marginal`` / ``num_programs`` (not
    in the reference either) the answer is the MARGINAL over several programs, sum_z q(z | x) p(a | z, image), with its
    probability and the hypotheses that voted; with ``rerank`` (not in the reference either) the hypotheses are weighted by
    their posterior under the generative model, p(x | z) p(z), from the reconstructor and the prior (``hypothesis_posterior``);
  * ``infer_programs`` (not in the reference either) asks the reverse question on batches that carry the answer: which of a
    question's hypotheses explains the question AND its known answer, p(z | x, a, image) over the candidates
    (``NeuralModuleNetwork.answer_posterior``); ``evaluate_program_inference`` and ``mine_supervision`` are built on it;
  * ``explain`` (not in the reference either) adds to each answer where its program looked: the attention map of every
    step, and that map painted over the question's image (``attention_overlay``).
Batches are dicts of DEVICE tensors with the reference's keys (a ``PrefetchingLoader`` yields them)."""
from typing import Any, Callable, Dict, Iterable, List, Optional

import numpy as np
import torch

from probnmn import _hip, hypothesis_rows
from probnmn.hypothesis_rows import HostCopies as _HostCopies
from probnmn.hypothesis_rows import awaited_hypotheses as _awaited_hypotheses
from probnmn.hypothesis_rows import group_hypotheses  # noqa: F401  (its public home is still here too)
from probnmn.hypothesis_rows import queue_hypotheses as _queue_hypotheses
from probnmn.modules.seq2seq_base import Seq2SeqBase, sampling_filter


class Evaluator:
    """``_Evaluator``: ``models`` name -> module (the trainer's dict, shared by reference), ``do_iteration(batch)``
    runs the phase's forward passes (which accumulate metrics inside the models)."""

    def __init__(self, models: Dict[str, torch.nn.Module], do_iteration: Callable[[Dict[str, torch.Tensor]], Any],
                 stages: Optional[tuple] = None):
        self.models = models
        self._do_iteration = do_iteration
        # (queue, finish): an iteration cut in two so that batch i + 1 is QUEUED before batch i is FINISHED -- same batches,
        # same order per model; what it buys is that the host's wait for a device result of batch i (the NMN needs the
        # generator's programs on the host) is spent with batch i + 1's kernels already in the queue
        self._stages = stages

    @torch.no_grad()
    def evaluate(self, batches: Iterable[Dict[str, torch.Tensor]], num_batches: Optional[int] = None) -> Dict[str, Dict[str, float]]:
        was_training = {k: m.training for k, m in self.models.items()}
        for m in self.models.values():
            m.eval()
            if hasattr(m, "get_metrics"):
                m.get_metrics(reset=True)
        try:
            if self._stages is None:
                for iteration, batch in enumerate(batches):
                    self._do_iteration(batch)
                    if num_batches is not None and iteration > num_batches:
                        break
            else:
                queue, finish = self._stages
                pending = None
                for iteration, batch in enumerate(batches):
                    queued = queue(batch, iteration)
                    if pending is not None:
                        finish(*pending)
                    pending = (batch, queued)
                    if num_batches is not None and iteration > num_batches:
                        break
                if pending is not None:
                    finish(*pending)
            return {k: m.get_metrics() for k, m in self.models.items() if hasattr(m, "get_metrics")}
        finally:
            for k, m in self.models.items():
                m.train(was_training[k])


def program_prior_evaluator(program_prior) -> Evaluator:
    """program_prior_evaluator.py: perplexity of the prior on validation programs."""
    return Evaluator({"program_prior": program_prior}, lambda b: program_prior(b["program"]))


def question_coding_evaluator(program_generator, question_reconstructor) -> Evaluator:
    """question_coding_evaluator.py:150-160: both models teacher-forced, "greedy"."""
    def it(b):
        return {"program_generator": program_generator(b["question"], b["program"], decoding_strategy="greedy"),
                "question_reconstructor": question_reconstructor(b["program"], b["question"], decoding_strategy="greedy")}
    return Evaluator({"program_generator": program_generator, "question_reconstructor": question_reconstructor}, it)


def answering_evaluator(program_generator, nmn) -> Evaluator:
    """module_training_evaluator.py:81-109 / joint_training_evaluator.py:74-103."""
    def it(b):
        pg_out = program_generator(b["question"], b["program"], decoding_strategy="greedy")
        return {"program_generator": pg_out, "nmn": nmn(b["image"], pg_out["predictions"], b["answer"])}

    # On the device the NMN's launch schedule depends on the programs, which it therefore reads back to the host
    # (models/nmn.py forward_trunk; the reference reads them back per example, nmn.py:203).  One batch at a time that is
    # generator -> wait -> plan -> NMN -> generator ...: the GPU idles while the host plans and the host idles while the
    # generator decodes.  Two stages instead: queue = generator pass + an asynchronous copy of the predictions into
    # one of two page-locked buffers; finish = wait for THAT copy, then the NMN on the host-side programs.
    pinned: Dict[Any, torch.Tensor] = {}

    def queue(b, iteration):
        pg_out = program_generator(b["question"], b["program"], decoding_strategy="greedy")
        pred = pg_out["predictions"]
        if not (pred.is_cuda and b["image"].is_cuda):
            return pg_out, None, None
        key = (iteration & 1, tuple(pred.shape), pred.dtype)
        if key not in pinned:
            pinned[key] = torch.empty(pred.shape, dtype=pred.dtype, pin_memory=True)
        host = pinned[key]
        host.copy_(pred, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record()
        return pg_out, host, copied

    def finish(b, queued):
        pg_out, host, copied = queued
        if host is None:
            return nmn(b["image"], pg_out["predictions"], b["answer"])
        copied.synchronize()
        # (the whole NMN pass here, stem included: the engine has ONE activation arena, and a stem launched for batch i + 1
        # would overwrite batch i's before its module programs have run.  The trunk on the process's trunk stream, beside
        # batch i + 1's generator pass, measured the same: 4.23 / 4.61 against 4.42 / 4.44 ms per 256-question batch)
        return nmn(b["image"], host, b["answer"])

    return Evaluator({"program_generator": program_generator, "nmn": nmn}, it, stages=(queue, finish))


def evaluate_answer_accuracy(program_generator, nmn, batches: Iterable[Dict[str, torch.Tensor]],
                             num_batches: Optional[int] = None) -> Dict[str, Dict[str, float]]:
    """Validation answer accuracy (the metric joint / module training select checkpoints on)."""
    return answering_evaluator(program_generator, nmn).evaluate(batches, num_batches)


def default_colormap() -> torch.Tensor:
    """uint8 [256, 3], the ramp ``attention_overlay`` colours a map through when none is given -- black, red, yellow, white,
    one channel after the other: entry v is (min(3v, 255), min(max(3v - 255, 0), 255), min(max(3v - 510, 0), 255))."""
    v = 3 * torch.arange(256)
    return torch.stack([(v - 255 * c).clamp(0, 255) for c in range(3)], dim=1).to(torch.uint8)


_COLORMAPS: Dict[Any, torch.Tensor] = {}  # the default ramp, once per device


@torch.no_grad()
def attention_overlay(attention: torch.Tensor, attention_mask: torch.Tensor, pixels: torch.Tensor, strength: int = 160,
                      colormap: Optional[torch.Tensor] = None):
    """The attention maps of ``NeuralModuleNetwork.forward(..., return_attention=True)`` painted over the images the
    questions were asked about, on the device (``pnmn_attention_overlay``, one launch): returns (overlays uint8
    [M, Hi, Wi, 3], index int64 [M, 2]) for the M true entries of ``attention_mask`` in row-major order, ``index[m]`` =
    (question, token position) of overlay m.

    ``attention`` fp32 [B, T, H, W], ``attention_mask`` bool [B, T], ``pixels`` uint8 [B, Hi, Wi, 3], all on the device.
    Each map is clamped to [0, 1], resized to the image (bilinear, half-pixel centres, 8-bit weights), coloured through
    ``colormap`` (uint8 [256, 3]; default ``default_colormap()``) and blended over the image with weight
    value * ``strength`` / 255**2 (``strength`` 0 .. 255: 0 leaves the image, 255 shows the pure colour where a map is 1).
    The arithmetic is integer and stated in include/probnmn_hip.h.  Reading M costs one device -> host synchronisation."""
    if attention.dim() != 4 or attention.dtype != torch.float32 or attention_mask.shape != attention.shape[:2] \
            or attention_mask.dtype != torch.bool:
        raise ValueError("attention fp32 [B, T, H, W] and attention_mask bool [B, T]; got %s %s and %s %s"
                         % (attention.dtype, tuple(attention.shape), attention_mask.dtype, tuple(attention_mask.shape)))
    if pixels.dim() != 4 or pixels.dtype != torch.uint8 or pixels.size(0) != attention.size(0) or pixels.size(3) != 3:
        raise ValueError("pixels uint8 [%d, Hi, Wi, 3]; got %s %s" % (attention.size(0), pixels.dtype, tuple(pixels.shape)))
    if not 0 <= int(strength) <= 255:
        raise ValueError("strength %r is not in 0 .. 255" % (strength,))
    dev = attention.device
    if dev.type != "cuda" or attention_mask.device != dev or pixels.device != dev:
        raise _hip.HipLibraryError("attention_overlay runs on the ROCm device the maps are on (got %s, %s, %s); there is no "
                                   "CPU path" % (dev, attention_mask.device, pixels.device))
    if colormap is None:
        colormap = _COLORMAPS.get(dev)
        if colormap is None:
            colormap = _COLORMAPS[dev] = default_colormap().to(dev)
    elif tuple(colormap.shape) != (256, 3) or colormap.dtype != torch.uint8:
        raise ValueError("colormap uint8 [256, 3]; got %s %s" % (colormap.dtype, tuple(colormap.shape)))
    colormap = colormap.to(dev).contiguous()
    B, T, H, W = attention.shape
    Hi, Wi = pixels.shape[1:3]
    if pixels.stride()[1:] != (Wi * 3, 3, 1) or (B > 1 and pixels.stride(0) < Hi * Wi * 3):
        pixels = pixels.contiguous()
    index = attention_mask.nonzero()  # row-major: the maps of a question are neighbours, so its image is read from HBM once
    M = index.size(0)
    out = torch.empty(M, Hi, Wi, 3, dtype=torch.uint8, device=dev)
    if M:
        maps = attention[attention_mask].contiguous()
        image_of = index[:, 0].to(torch.int32).contiguous()
        _hip.check(_hip.lib().pnmn_attention_overlay(
            maps.data_ptr(), image_of.data_ptr(), pixels.data_ptr(), pixels.stride(0) if B > 1 else Hi * Wi * 3, B, Hi, Wi,
            colormap.data_ptr(), int(strength), out.data_ptr(), M, H, W, _hip.stream_ptr(dev)), "attention_overlay")
    return out, index


def _marginal_options(beam_size, marginal, num_programs, explain) -> bool:
    """The argument rules of ``marginal`` / ``num_programs`` (``predict_answers`` states them); true when the answers are
    marginals."""
    if num_programs is not None:
        if isinstance(num_programs, bool) or not isinstance(num_programs, int):
            raise ValueError("num_programs must be an int in 2 .. 64, got %r" % (num_programs,))
        if not 2 <= num_programs <= 64:
            raise ValueError("num_programs must be in 2 .. 64, got %d" % num_programs)
        if beam_size is not None:
            raise ValueError("num_programs samples the hypotheses; with beam_size they are searched (marginal=True)")
    elif marginal and beam_size is None:
        raise ValueError("marginal=True marginalises over the beam's hypotheses: give a beam_size (or num_programs)")
    if (marginal or num_programs is not None) and explain:
        raise ValueError("explain=True explains the one program an answer came from; a marginal answer has several")
    return bool(marginal) or num_programs is not None


SAMPLE_WEIGHTS = ("probability", "importance")


def _scaled_exp1(c: torch.Tensor) -> torch.Tensor:
    """exp(c) E1(c) = int_0^inf exp(-x) / (x + c) dx for c > 0 (float64): the power series of E1 up to c = 1, the continued
    fraction 1 / (c + 1 - 1 / (c + 3 - 4 / (c + 5 - ...))) above (evaluated bottom up, 80 levels: 1e-15 at c = 1)."""
    small = c.clamp(min=1e-300, max=1.0)
    term, series = torch.ones_like(small), torch.zeros_like(small)
    for k in range(1, 26):
        term = term * (-small) / k  # (-c)^k / k!
        series = series - term / k
    low = torch.exp(small) * (-0.5772156649015329 - torch.log(small) + series)
    big = c.clamp(min=1.0, max=1e300)
    tail = big + (2 * 80 + 1)
    for k in range(80, 0, -1):
        tail = big + (2 * k - 1) - k * k / tail
    return torch.where(c <= 1.0, low, 1.0 / tail)


_LAGUERRE = np.polynomial.laguerre.laggauss(48)  # nodes and weights of int_0^inf exp(-x) f(x) dx


def without_replacement_weights(log_probabilities: torch.Tensor, perturbed: torch.Tensor) -> torch.Tensor:
    """Log importance weights of a sample without replacement (Kool, van Hoof and Welling 2019, section 4.2), from what
    ``Seq2SeqBase.decode_stochastic_beam`` returns: ``log_probabilities`` = phi and ``perturbed`` = G, both [B, K], best
    first: sum_i w_i f(z_i) is an unbiased estimate of E_p[f], and divided by sum_i w_i (what
    ``NeuralModuleNetwork.marginal_answers`` does with any weights) it is the paper's normalised estimator.  The K-th
    perturbed value is the threshold kappa = G[:, K-1]; slot K-1 gets -inf.

    The paper's w_i = p_i / q_i(kappa), q_i(kappa) = 1 - exp(-exp(phi_i - kappa)), holds for UNCONDITIONED Gumbels.  The search
    starts from G = 0 at the root, so its G are conditioned on the largest being 0, and that formula would come out biased
    low (sum_i w_i averages 0.75 at K = 2).  The root's free value M ~ Gumbel(0) is independent of the sample, and given M
    the unconditioned values follow from the returned ones: exp(-G'_i) = exp(-M) - 1 + exp(-G_i).  With E = exp(-M) ~ Exp(1)
    and c = exp(-kappa) - 1, the threshold becomes exp(-kappa') = E + c, and the weight is the paper's, averaged over E:

        w_i = p_i  int_0^inf exp(-x) / (1 - exp(-p_i (x + c))) dx          for i < K-1,      p_i = exp(phi_i)

    -- a function of (phi_i, kappa) alone, unbiased, and of smaller variance than a drawn M.  Evaluated as
    exp(c) E1(c) + p_i int exp(-x) r(p_i (x + c)) dx with r(y) = 1 / (1 - exp(-y)) - 1 / y, which is smooth and lies in
    [1/2, 1): a 48-point Gauss-Laguerre rule; the first term carries the logarithmic singularity of c -> 0.
    kappa = -inf (fewer than K sequences exist: the whole support was enumerated): log w_i = phi_i for every finite slot.  A
    slot without a sequence (phi = -inf) gets -inf.  Pure torch, any device, computed in float64 and returned in the dtype of
    ``log_probabilities``; no overflow or NaN for any finite phi_i and kappa < 0."""
    phi, g = log_probabilities, perturbed
    if phi.dim() != 2 or phi.shape != g.shape:
        raise ValueError("log_probabilities and perturbed are [B, K] each; got %s and %s" % (tuple(phi.shape), tuple(g.shape)))
    phi64, kappa = phi.double(), g[:, -1:].double()
    finite = torch.isfinite(phi64)
    p = torch.exp(torch.where(finite, phi64, torch.zeros_like(phi64)))
    c = torch.expm1(-kappa).clamp(min=1e-300).expand_as(p)  # (+inf where kappa = -inf; kappa = 0: the only slot, K = 1)
    whole = torch.isinf(c)
    c_ = torch.where(whole, torch.ones_like(c), c)
    nodes = torch.as_tensor(_LAGUERRE[0], dtype=torch.float64, device=phi.device)
    weights = torch.as_tensor(_LAGUERRE[1], dtype=torch.float64, device=phi.device)
    y = (p * c_).unsqueeze(-1) + p.unsqueeze(-1) * nodes  # p (x + c), the product first: c may be 1e300
    y_ = y.clamp(min=1e-4)
    r = torch.where(y < 1e-4, 0.5 + y / 12.0, -1.0 / torch.expm1(-y_) - 1.0 / y_)
    w = _scaled_exp1(c_) + p * (r * weights).sum(-1)
    out = torch.where(finite, torch.where(whole, phi64, torch.log(w)), torch.full_like(phi64, float("-inf")))
    out[:, -1] = float("-inf")
    return out.to(phi.dtype)


def _without_replacement_options(without_replacement, sample_weights, beam_size, num_programs) -> Optional[str]:
    """The argument rules of ``without_replacement`` / ``sample_weights`` (``predict_answers`` states them): None, or the
    weights a without-replacement sample hands on."""
    if sample_weights not in SAMPLE_WEIGHTS:
        raise ValueError("sample_weights must be one of %s, got %r" % (SAMPLE_WEIGHTS, sample_weights))
    if not without_replacement:
        if sample_weights != "probability":
            raise ValueError("sample_weights=%r weighs a sample without replacement: give without_replacement=True" % (sample_weights,))
        return None
    if beam_size is not None:
        raise ValueError("without_replacement=True samples num_programs hypotheses; with beam_size they are searched")
    sizes = tuple(k for k in Seq2SeqBase.BEAM_SIZES if k >= 2)
    if isinstance(num_programs, bool) or not isinstance(num_programs, int) or num_programs not in sizes:
        raise ValueError("without_replacement=True draws num_programs hypotheses in one stochastic beam search: num_programs must be "
                         "one of %s, got %r" % (sizes, num_programs))
    return sample_weights


def _rerank_weights(weights):
    """``(w_x, w_z, w_q)`` of ``hypothesis_posterior`` as three finite floats; ``ValueError`` otherwise."""
    import math

    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError("weights must be three numbers (w_x, w_z, w_q), got %r" % (weights,))
    if len(w) != 3 or not all(math.isfinite(v) for v in w):
        raise ValueError("weights must be three finite numbers (w_x, w_z, w_q), got %r" % (weights,))
    return w


def _rerank_options(rerank, beam_size, num_programs, explain, question_reconstructor, program_prior, rerank_weights):
    """The argument rules of ``rerank`` (``predict_answers`` states them), checked before any model is touched; the three
    coefficients, or None when the hypotheses are not reranked."""
    if not rerank:
        return None
    if beam_size is None and num_programs is None:
        raise ValueError("rerank=True reranks several hypotheses per question: give a beam_size or num_programs")
    if explain:
        raise ValueError("explain=True explains the one program an answer came from; a reranked answer has several")
    w = _rerank_weights(rerank_weights)
    if question_reconstructor is None and w[0] != 0.0:
        raise ValueError("rerank_weights[0] = %r weighs log p(x | z): give the question_reconstructor (or make it 0)" % (w[0],))
    if program_prior is None and w[1] != 0.0:
        raise ValueError("rerank_weights[1] = %r weighs log p(z): give the program_prior (or make it 0)" % (w[1],))
    return w


@torch.no_grad()
def hypothesis_posterior(question_reconstructor, program_prior, questions: torch.Tensor, programs: torch.Tensor, question_rows,
                         log_q=None, weights=(1.0, 1.0, 0.0), max_rows: int = 1024) -> Dict[str, torch.Tensor]:
    """The posterior over each question's program hypotheses under the generative model (not in the reference, which
    scores sampled programs with the three models in training only: modules/elbo.py):
        log p(z_r | x) = w_x log p(x | z_r) + w_z log p(z_r) + w_q log q(z_r | x) - log of the sum over the question's rows
    with ``weights`` = (w_x, w_z, w_q).  The default (1, 1, 0) is the exact posterior of p(x | z) p(z) restricted to the
    candidate set; ``w_q`` mixes the generator's own weight back in.  Inference only, no gradient.

    ``questions`` [G, Tq] on the device; ``programs`` [R, T] (host or device) with ``question_rows`` [R], non-decreasing, in
    0 .. G - 1 -- the layout ``group_hypotheses`` returns; the programs as the decoders return them (trimmed behind their
    @end@), fed as the ELBO passes feed sampled programs.  ``log_q`` [R] or None (then ``w_q`` must be 0).  Either model may
    be None; its coefficient must then be 0 (``ValueError``), and its per-row output is NaN.  A term whose coefficient is 0
    is left out of the score entirely.

    Program row r is scored against ``questions[question_rows[r]]`` by ``QuestionReconstructor.teacher_forced_logits`` and
    ``ProgramPrior.teacher_forced_logits`` in passes of at most ``max_rows`` rows -- scoring passes: no metric of either
    model moves, no seed is drawn from the torch generator, and their ``train()`` / ``eval()`` state comes back as it was
    -- then ONE ``pnmn_hypothesis_posterior`` launch (the rule: include/probnmn_hip.h).

    Returns device tensors: ``"log_posterior"``, ``"log_reconstruction"`` (log p(x | z_r), a sum over the question's
    tokens), ``"log_prior"`` (log p(z_r)) fp32 [R]; ``"log_evidence"`` fp32 [G] (log of the summed unnormalised scores; -inf
    where no hypothesis has a finite score), ``"best_row"`` int32 [G] (the MAP hypothesis's row, first of equals; -1 there)
    and ``"support"`` int32 [G] (hypotheses with a finite score)."""
    w = _rerank_weights(weights)
    if question_reconstructor is None and w[0] != 0.0:
        raise ValueError("weights[0] = %r weighs log p(x | z): give the question_reconstructor (or make it 0)" % (w[0],))
    if program_prior is None and w[1] != 0.0:
        raise ValueError("weights[1] = %r weighs log p(z): give the program_prior (or make it 0)" % (w[1],))
    if log_q is None and w[2] != 0.0:
        raise ValueError("weights[2] = %r weighs log q(z | x): give log_q (or make it 0)" % (w[2],))
    if question_reconstructor is None and program_prior is None and log_q is None:
        raise ValueError("nothing to score the hypotheses with: no question_reconstructor, no program_prior and no log_q")
    if max_rows < 1:
        raise ValueError("max_rows must be at least 1, got %r" % (max_rows,))
    dev = questions.device
    if dev.type != "cuda":
        raise _hip.HipLibraryError("hypothesis_posterior runs on the ROCm device the questions are on (got %s); there is no "
                                   "CPU path" % dev)
    G = int(questions.size(0))
    qrows = hypothesis_rows.on_host(question_rows)
    R = int(qrows.size)
    if questions.dim() != 2 or programs.dim() != 2 or programs.size(0) != R or qrows.ndim != 1:
        raise ValueError("questions [G, Tq], programs [R, T] and question_rows [R]; got %s, %s and %s"
                         % (tuple(questions.shape), tuple(programs.shape), qrows.shape))
    hypothesis_rows.check(qrows, G)
    f = dict(dtype=torch.float32, device=dev)
    out = {"log_posterior": torch.empty(R, **f), "log_reconstruction": torch.full((R,), float("nan"), **f),
           "log_prior": torch.full((R,), float("nan"), **f), "log_evidence": torch.full((G,), -float("inf"), **f),
           "best_row": torch.full((G,), -1, dtype=torch.int32, device=dev),
           "support": torch.zeros(G, dtype=torch.int32, device=dev)}
    if R == 0 or G == 0:  # (no row anywhere: what the kernel writes for a group without rows)
        return out
    q = None if log_q is None else hypothesis_rows.row_vector(log_q, "log_q", R, dev)
    programs = programs.detach().to(device=dev, dtype=torch.long)
    rows_dev = _hip.to_device(qrows, dev).view(torch.long)
    models = [m for m in (question_reconstructor, program_prior) if m is not None]
    was_training = [m.training for m in models]
    for m in models:
        m.eval()
    x = z = None  # (logits [R, T, V], tokens [R, T]) of each term, filled pass by pass
    try:
        for lo in range(0, R, max_rows):
            hi = min(lo + max_rows, R)
            if question_reconstructor is not None:
                logits, tokens = question_reconstructor.teacher_forced_logits(programs[lo:hi],
                                                                              questions.index_select(0, rows_dev[lo:hi]))
                if x is None:
                    x = (torch.empty((R,) + tuple(logits.shape[1:]), **f), torch.empty(R, tokens.size(1), dtype=torch.long, device=dev))
                x[0][lo:hi], x[1][lo:hi] = logits, tokens
            if program_prior is not None:
                logits, tokens = program_prior.teacher_forced_logits(programs[lo:hi])
                if z is None:
                    z = (torch.empty((R,) + tuple(logits.shape[1:]), **f), torch.empty(R, tokens.size(1), dtype=torch.long, device=dev))
                z[0][lo:hi], z[1][lo:hi] = logits, tokens
    finally:
        for m, training in zip(models, was_training):
            m.train(training)
    group_start = hypothesis_rows.group_start_on_device(qrows, G, dev)

    def term(t, model):
        if t is None:
            return (0, 0, 0), (0, 0, 0)
        return (t[0].data_ptr(), t[1].data_ptr(), t[1].stride(0)), (t[0].size(1), t[0].size(2), model._pad_index)

    (x_args, (Tx, Vx, pad_x)), (z_args, (Tz, Vz, pad_z)) = term(x, question_reconstructor), term(z, program_prior)
    _hip.check(_hip.lib().pnmn_hypothesis_posterior(
        *x_args, *z_args, 0 if q is None else q.data_ptr(), group_start.data_ptr(), w[0], w[1], w[2], pad_x, pad_z,
        out["log_reconstruction"].data_ptr() if x is not None else 0, out["log_prior"].data_ptr() if z is not None else 0,
        out["log_posterior"].data_ptr(), out["log_evidence"].data_ptr(), out["best_row"].data_ptr(), out["support"].data_ptr(),
        G, R, Tx, Vx, Tz, Vz, _hip.stream_ptr(dev)), "hypothesis_posterior")
    return out


def _finish_hypotheses(nmn, image, queued, rerank=None):
    """Second stage: wait for the copy, keep the valid hypotheses (merged), run the NMN over them and marginalise.
    ``rerank`` = (question_reconstructor, program_prior, coefficients, questions [B, Tq]) or None: the hypotheses' weights
    are their posterior under the generative model (``hypothesis_posterior``, the merged generator weight as its ``log_q``)
    instead of the generator's own.  Returns (``marginal_answers``' dict as host numpy -- reranked: and
    ``hypothesis_posterior``'s ``"log_reconstruction"``, ``"log_prior"`` and ``"best_row"``; a sample without replacement: and
    ``"perturbed"`` [R], G of every row's first slot --, programs [R, T], group_start [B + 1])."""
    perturbed = queued[3]
    B, programs, question_rows, log_weights, first_slot, scored = _awaited_hypotheses(nmn, queued, rerank)
    out = nmn.marginal_answers(image, torch.from_numpy(programs), question_rows, log_weights)
    out.update(scored)
    if perturbed is not None:
        out["perturbed"] = perturbed.cpu()[torch.from_numpy(question_rows), torch.from_numpy(first_slot)]
    return ({k: v.cpu().numpy() for k, v in out.items()}, programs, hypothesis_rows.group_start(question_rows, B))


@torch.no_grad()
def predict_answers(program_generator, nmn, batches: Iterable[Dict[str, torch.Tensor]], vocabulary,
                    beam_size: Optional[int] = None, prefer_valid: bool = True,
                    constrained: bool = False, extractor=None, temperature: float = 1.0, top_k: int = 0,
                    top_p: float = 1.0, constrained_sampling: bool = False, explain: bool = False,
                    overlay_strength: int = 160, colormap: Optional[torch.Tensor] = None, marginal: bool = False,
                    num_programs: Optional[int] = None, rerank: bool = False, question_reconstructor=None, program_prior=None,
                    rerank_weights=(1.0, 1.0, 0.0), without_replacement: bool = False,
                    sample_weights: str = "probability") -> List[Dict[str, Any]]:
    """scripts/inference.py:76-91: sampled programs -> NMN -> answer strings, one record per question
    (``question_index`` from the batch when present, else a running index).

    ``beam_size`` (1, 2, 4, 8 or 16): the generator decodes with beam search instead (``decoding_strategy="beam"``) and
    the NMN gets, per question, the most probable hypothesis -- or, with ``prefer_valid``, the best-ranked hypothesis
    that the program compiler accepts (the most probable one when none is valid).  Validity is decided on the host from
    the [B, K, T] tokens the loop copies out anyway.  Each record then also names ``"program"`` (token strings of the
    chosen hypothesis, without padding), its ``"beam_rank"`` and whether it is a ``"program_valid"`` one.

    ``constrained`` (needs ``beam_size``): the beam kernel searches under the program compiler's validity rule
    (``nmn.engine.compiler.decoding_automaton``), so every hypothesis it returns is a valid program: ``program_valid`` is
    always true, and ``beam_rank`` is 0 under ``prefer_valid``.  The record layout is the same.

    ``extractor`` (a ``ResNet101Stage3`` on the device): a batch without ``"image"`` features but with ``"pixels"`` --
    decoded uint8 images [B, H, W, 3] of any size, on the device -- gets its features from ``extractor.forward_pixels``
    (resize, normalisation and the network, all on the device), queued with the generator pass; the NMN reads the
    ``channels_last`` result in place.  A batch with neither key, or with pixels but no extractor, is a ``ValueError``.

    ``temperature``, ``top_k``, ``top_p``: the sampling filter of the generator's sampled programs (``Seq2SeqBase.decode``);
    the record layout is unchanged.  Values out of range, or a filter other than (1, 0, 1) together with ``beam_size``
    (a beam search draws nothing), are a ``ValueError``.

    ``constrained_sampling``: the programs are SAMPLED under the program compiler's validity rule
    (``decoding_strategy="constrained_sampling"`` with ``nmn.engine.compiler.decoding_automaton``; ``temperature``, ``top_k``
    and ``top_p`` apply), on the multi-CU decoder kernels the plain sampled decode runs on, so no question is answered
    ``@@UNKNOWN@@`` for want of a valid program.  Each record also names its ``"program"`` and whether it is a
    ``"program_valid"`` one (decided on the host, as for the beams: always true).  Together with ``beam_size`` it is a
    ``ValueError``.

    ``explain``: each record also names its ``"program"`` (with every decoding option) and its ``"steps"``: one entry per
    module call of the program the NMN ran that wrote a one-channel attention map (``NMNEngine.attention_maps``), in
    execution order -- right to left over the program -- as ``{"position": token position, "token": its string,
    "attention": float32 numpy [H, W]}``.  When the batch has ``"pixels"`` an entry also has ``"overlay"``: uint8 numpy
    [Hi, Wi, 3], the map painted over the question's image (``attention_overlay`` with ``overlay_strength`` and
    ``colormap``).  An invalid program has no steps.  The answers are those of ``explain=False``: the maps are copied out
    of the activations the pass leaves behind.

    ``marginal`` (needs ``beam_size``; works with ``constrained``): the answer is the marginal over the K hypotheses of the
    beam, sum_z q(z | x) p(a | z, image), with q = ``beam_log_probabilities`` renormalised over the hypotheses that are
    valid programs (``NeuralModuleNetwork.marginal_answers``; identical hypotheses are merged first: ``group_hypotheses``).
    ``num_programs`` = N (2 .. 64, without ``beam_size``): each question is decoded N times in one generator call -- the
    sampling options apply -- and the answer is the marginal over the draws, uniformly weighted.  A record then holds
    ``"question_index"``, ``"answer"`` (the marginal prediction; ``@@UNKNOWN@@`` when no hypothesis is valid), its
    ``"answer_probability"`` (0.0 then), the ``"support"`` (how many distinct valid hypotheses voted) and the
    ``"hypotheses"``: ``{"program": token strings, "weight": its share, "answer": its own answer}`` each, in group order.
    ``marginal`` without ``beam_size``, ``num_programs`` with it, either with ``explain``, or a ``num_programs`` that is
    not an int in range, are a ``ValueError``.

    ``rerank`` (needs the hypotheses of ``beam_size`` or ``num_programs`` and implies the marginal answer): the generator only
    PROPOSES the hypotheses; their weights are the posterior under the generative model, p(z | x) ~ p(x | z)^w_x p(z)^w_z
    q(z | x)^w_q over the distinct valid hypotheses of a question, from ``question_reconstructor`` (p(x | z)), ``program_prior``
    (p(z)) and ``rerank_weights`` = (w_x, w_z, w_q) (``hypothesis_posterior``; q is the merged weight of ``group_hypotheses``:
    the beam score, or ``log count`` for samples).  The default (1, 1, 0) is the exact posterior restricted to the candidate
    set; (0, 0, 1) gives the answers of ``rerank=False``.  A record's ``"weight"`` is then the posterior share, each
    hypothesis also names its ``"log_reconstruction"`` (log p(x | z)) and ``"log_prior"`` (log p(z)) (None for a model that
    was not given), and the record gains ``"map_program"`` and ``"map_answer"``: the hypothesis with the largest posterior
    and its own answer (``[]`` and ``@@UNKNOWN@@`` when there is none).  The models are left as they were: no metric, no
    seed, their ``train()`` / ``eval()`` state.  ``rerank`` without hypotheses, with ``explain``, with coefficients that are
    not three finite numbers, or without a model whose coefficient is not 0, is a ``ValueError``, raised before any model
    is touched.

    ``without_replacement`` (with ``num_programs`` = N in 2, 4, 8 or 16): the N hypotheses of a question are a sample WITHOUT
    replacement from the generator -- N distinct programs from ONE stochastic beam search
    (``decoding_strategy="stochastic_beam"``) instead of N independent decodes that mostly repeat each other; with
    ``constrained_sampling`` they are drawn under the validity rule.  ``sample_weights``: ``"probability"`` hands their
    log-probabilities to ``group_hypotheses`` / ``marginal_answers`` exactly as the beam path hands its scores;
    ``"importance"`` hands ``without_replacement_weights`` (the N-th hypothesis sets the threshold and weighs nothing).
    Everything downstream, ``rerank`` included, is unchanged; each hypothesis of a record also names its ``"perturbed"``
    log-probability.  ``without_replacement`` with ``beam_size``, with a ``num_programs`` outside those sizes or with a
    sampling filter, and ``sample_weights`` without ``without_replacement``, are a ``ValueError``."""
    draw = _without_replacement_options(without_replacement, sample_weights, beam_size, num_programs)
    coefficients = _rerank_options(rerank, beam_size, num_programs, explain, question_reconstructor, program_prior, rerank_weights)
    marginalise = _marginal_options(beam_size, marginal or (rerank and num_programs is None), num_programs, explain)
    if constrained and beam_size is None:
        raise ValueError("constrained=True constrains the beam search: give a beam_size")
    if constrained_sampling and beam_size is not None:
        raise ValueError("constrained_sampling=True samples the programs; with beam_size they are searched (constrained=True)")
    filt = sampling_filter(temperature, top_k, top_p)
    if filt is not None and beam_size is not None:
        raise ValueError("temperature / top_k / top_p filter sampled programs; with beam_size the programs are searched, not drawn")
    if filt is not None and draw is not None:
        raise ValueError("temperature / top_k / top_p filter independent draws; a sample without replacement takes no filter")
    sampling = {} if filt is None else dict(temperature=filt[0], top_k=filt[1], top_p=filt[2])
    was_training = (program_generator.training, nmn.training)
    program_generator.eval()
    nmn.eval()
    records: List[Dict[str, Any]] = []
    try:
        # (as in answering_evaluator: batch i + 1's generator pass is queued before batch i's programs are awaited on the host)
        pinned: Dict[Any, torch.Tensor] = {}
        pad = getattr(program_generator, "_pad_index", 0)
        constraint = None
        if constrained or constrained_sampling:  # built once (and cached on the compiler): the tokens the decoder never emits do not count
            exclude = [getattr(program_generator, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
            constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)

        def features(batch):
            if "image" in batch:
                return batch["image"]
            if "pixels" not in batch:
                raise ValueError("a batch needs \"image\" features or \"pixels\" (uint8 [B, H, W, 3]); it has %s" % sorted(batch))
            if extractor is None:
                raise ValueError("a batch of \"pixels\" needs an extractor (predict_answers(..., extractor=ResNet101Stage3))")
            return extractor.forward_pixels(batch["pixels"])

        copies = _HostCopies()

        def queue(batch, iteration):
            image = features(batch)
            if marginalise:
                return _queue_hypotheses(program_generator, batch, iteration, copies, beam_size, num_programs, constraint,
                                         constrained_sampling, sampling, image.is_cuda, draw), image
            if constrained_sampling:
                programs = program_generator(batch["question"], decoding_strategy="constrained_sampling", constraint=constraint,
                                             **sampling)["predictions"]
            elif beam_size is None:
                programs = program_generator(batch["question"], **sampling)["predictions"]
            else:
                extra = {} if constraint is None else {"constraint": constraint}
                programs = program_generator(batch["question"], decoding_strategy="beam", beam_size=beam_size,
                                             **extra)["beam_predictions"]
            if not (programs.is_cuda and image.is_cuda):
                return programs, None, image
            key = (iteration & 1, tuple(programs.shape), programs.dtype)
            if key not in pinned:
                pinned[key] = torch.empty(programs.shape, dtype=programs.dtype, pin_memory=True)
            pinned[key].copy_(programs, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
            return pinned[key], copied, image

        def choose(beams):
            """[B, K, T] host tokens -> (programs [B, T], rank per question, validity of the chosen program)."""
            B, K, T = beams.shape
            arr = beams.cpu().numpy()
            # (the NMN decides the validity of the B chosen programs again on its own: host work, microseconds per program)
            if prefer_valid:
                compiled = nmn.engine.compiler.compile_batch(arr.reshape(B * K, T))
                ok = [[compiled[b * K + k].valid for k in range(K)] for b in range(B)]
                ranks = [row.index(True) if True in row else 0 for row in ok]
                valid = [row[r] for row, r in zip(ok, ranks)]
            else:
                ranks = [0] * B
                valid = [c.valid for c in nmn.engine.compiler.compile_batch(arr[:, 0])]
            return beams[torch.arange(B), torch.tensor(ranks, dtype=torch.long)], ranks, valid

        def token_strings(row):
            return [vocabulary.get_token_from_index(int(t), namespace="programs") for t in row if t != pad]

        def finish_marginal(batch, queued):
            hypotheses, image = queued
            reranked = None if coefficients is None else (question_reconstructor, program_prior, coefficients, batch["question"])
            out, programs, start = _finish_hypotheses(nmn, image, hypotheses, reranked)
            B = len(start) - 1
            index = batch["question_index"].cpu().tolist() if "question_index" in batch else range(len(records), len(records) + B)
            for i, qi in enumerate(index):
                a, n = int(out["predictions"][i]), int(out["support"][i])
                records.append({
                    "question_index": int(qi), "answer": vocabulary.get_token_from_index(a, namespace="answers"),
                    "answer_probability": float(np.exp(out["log_probabilities"][i, a])) if n > 0 else 0.0, "support": n,
                    "hypotheses": [{"program": token_strings(programs[r]), "weight": float(out["hypothesis_weights"][r]),
                                    "answer": vocabulary.get_token_from_index(int(out["hypothesis_predictions"][r]), namespace="answers")}
                                   for r in range(start[i], start[i + 1])]})
                if draw is not None:
                    for h, r in zip(records[-1]["hypotheses"], range(start[i], start[i + 1])):
                        h["perturbed"] = float(out["perturbed"][r])
                if reranked is not None:
                    for h, r in zip(records[-1]["hypotheses"], range(start[i], start[i + 1])):
                        h["log_reconstruction"] = None if question_reconstructor is None else float(out["log_reconstruction"][r])
                        h["log_prior"] = None if program_prior is None else float(out["log_prior"][r])
                    best = int(out["best_row"][i])
                    records[-1]["map_program"] = token_strings(programs[best]) if best >= 0 else []
                    records[-1]["map_answer"] = vocabulary.get_token_from_index(
                        int(out["hypothesis_predictions"][best]) if best >= 0 else nmn._unknown_answer, namespace="answers")

        def finish(batch, queued):
            if marginalise:
                return finish_marginal(batch, queued)
            programs, copied, image = queued
            if copied is not None:
                copied.synchronize()
            extra = None
            if beam_size is not None:
                programs, ranks, valid = choose(programs)
                extra = (programs.tolist(), ranks, valid)
            elif constrained_sampling:
                host = programs.cpu()
                extra = (host.tolist(), None, [c.valid for c in nmn.engine.compiler.compile_batch(host.numpy())])
            out = nmn(image, programs, return_attention=True) if explain else nmn(image, programs)
            answers = out["predictions"].cpu().tolist()
            if explain:
                rows = extra[0] if extra is not None else programs.cpu().tolist()
                mask = out["attention_mask"].cpu().numpy()
                maps = out["attention"].cpu().numpy()
                overlays, where = None, {}
                if "pixels" in batch:
                    overlays, at = attention_overlay(out["attention"], out["attention_mask"], batch["pixels"], overlay_strength, colormap)
                    overlays = overlays.cpu().numpy()
                    where = {(int(i), int(p)): m for m, (i, p) in enumerate(at.cpu().tolist())}
            index = batch["question_index"].cpu().tolist() if "question_index" in batch else range(len(records), len(records) + len(answers))
            for i, (qi, a) in enumerate(zip(index, answers)):
                record = {"question_index": int(qi), "answer": vocabulary.get_token_from_index(int(a), namespace="answers")}
                if extra is not None:
                    record["program"] = [vocabulary.get_token_from_index(int(t), namespace="programs") for t in extra[0][i] if t != pad]
                    if extra[1] is not None:
                        record["beam_rank"] = int(extra[1][i])
                    record["program_valid"] = bool(extra[2][i])
                if explain:
                    tokens = [vocabulary.get_token_from_index(int(t), namespace="programs") for t in rows[i]]
                    record.setdefault("program", [tok for tok, t in zip(tokens, rows[i]) if t != pad])
                    record["steps"] = []
                    for p in reversed(mask[i].nonzero()[0].tolist()):  # execution order: right to left
                        step = {"position": p, "token": tokens[p], "attention": maps[i, p]}
                        if overlays is not None:
                            step["overlay"] = overlays[where[(i, p)]]
                        record["steps"].append(step)
                records.append(record)

        pending = None
        for iteration, batch in enumerate(batches):
            queued = queue(batch, iteration)
            if pending is not None:
                finish(*pending)
            pending = (batch, queued)
        if pending is not None:
            finish(*pending)
        return records
    finally:
        program_generator.train(was_training[0])
        nmn.train(was_training[1])


@torch.no_grad()
def evaluate_marginal_answer_accuracy(program_generator, nmn, batches: Iterable[Dict[str, torch.Tensor]], vocabulary=None,
                                      beam_size: Optional[int] = None, num_programs: Optional[int] = None,
                                      constrained: bool = False, constrained_sampling: bool = False,
                                      num_batches: Optional[int] = None, rerank: bool = False, question_reconstructor=None,
                                      program_prior=None, rerank_weights=(1.0, 1.0, 0.0), without_replacement: bool = False,
                                      sample_weights: str = "probability") -> Dict[str, float]:
    """Answer accuracy of the MARGINAL answer over several programs per question -- the ``beam_size`` hypotheses of a beam
    search (``constrained``: under the validity rule), weighted by their probabilities, or ``num_programs`` sampled ones
    (``constrained_sampling``), uniformly weighted -- on batches with ``"answer"``; free-running decodes, unlike
    ``answering_evaluator``'s teacher-forced greedy pass, which stays what it is.  Returns ``"answer_accuracy"``,
    ``"single_answer_accuracy"`` (each question answered by its FIRST valid hypothesis alone -- the best beam, the first
    draw --, from the same pass), ``"average_support"`` (distinct valid hypotheses per question) and
    ``"average_rows_per_question"`` (NMN rows run per question).  ``vocabulary`` is not needed and only kept for symmetry
    with ``predict_answers``; ``num_batches`` stops the loop as ``Evaluator.evaluate`` does.

    ``rerank``, ``question_reconstructor``, ``program_prior``, ``rerank_weights``: as for ``predict_answers`` -- the hypotheses
    are weighted by their posterior under the generative model -- and the result also holds ``"map_answer_accuracy"``: each
    question answered by its MAP hypothesis alone.

    ``without_replacement``, ``sample_weights``: as for ``predict_answers`` -- the ``num_programs`` hypotheses are one
    stochastic beam search's, a sample without replacement."""
    draw = _without_replacement_options(without_replacement, sample_weights, beam_size, num_programs)
    if beam_size is None and num_programs is None:
        raise ValueError("give the hypotheses: beam_size (a beam search) or num_programs (samples)")
    coefficients = _rerank_options(rerank, beam_size, num_programs, False, question_reconstructor, program_prior, rerank_weights)
    _marginal_options(beam_size, beam_size is not None, num_programs, False)
    if constrained and beam_size is None:
        raise ValueError("constrained=True constrains the beam search: give a beam_size")
    if constrained_sampling and beam_size is not None:
        raise ValueError("constrained_sampling=True samples the programs; with beam_size they are searched (constrained=True)")
    was_training = (program_generator.training, nmn.training)
    program_generator.eval()
    nmn.eval()
    constraint = None
    if constrained or constrained_sampling:
        exclude = [getattr(program_generator, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
        constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)
    copies = _HostCopies()
    totals = {"questions": 0, "correct": 0, "single": 0, "support": 0, "rows": 0, "map": 0}

    def finish(batch, queued):
        reranked = None if coefficients is None else (question_reconstructor, program_prior, coefficients, batch["question"])
        out, programs, start = _finish_hypotheses(nmn, batch["image"], queued, reranked)
        answers = batch["answer"].cpu().numpy()
        has = start[1:] > start[:-1]
        single = np.full(answers.shape[0], nmn._unknown_answer, np.int64)
        single[has] = out["hypothesis_predictions"][start[:-1][has]]
        totals["questions"] += answers.shape[0]
        totals["correct"] += int((out["predictions"] == answers).sum())
        totals["single"] += int((single == answers).sum())
        totals["support"] += int(out["support"].sum())
        totals["rows"] += int(programs.shape[0])
        if reranked is not None:
            best = out["best_row"]
            by_map = np.full(answers.shape[0], nmn._unknown_answer, np.int64)
            by_map[best >= 0] = out["hypothesis_predictions"][best[best >= 0]]
            totals["map"] += int((by_map == answers).sum())

    try:
        pending = None
        for iteration, batch in enumerate(batches):
            queued = _queue_hypotheses(program_generator, batch, iteration, copies, beam_size, num_programs, constraint,
                                       constrained_sampling, {}, batch["image"].is_cuda, draw)
            if pending is not None:
                finish(*pending)
            pending = (batch, queued)
            if num_batches is not None and iteration > num_batches:
                break
        if pending is not None:
            finish(*pending)
    finally:
        program_generator.train(was_training[0])
        nmn.train(was_training[1])
    n = max(totals["questions"], 1)
    result = {"answer_accuracy": totals["correct"] / n, "single_answer_accuracy": totals["single"] / n,
              "average_support": totals["support"] / n, "average_rows_per_question": totals["rows"] / n}
    if coefficients is not None:
        result["map_answer_accuracy"] = totals["map"] / n
    return result


def _program_inference_options(beam_size, num_programs, constrained, constrained_sampling, without_replacement, sample_weights,
                               answer_weight, rerank, question_reconstructor, program_prior, rerank_weights):
    """The argument rules of ``infer_programs`` and what is built on it, checked before any model is touched: (the weights a
    without-replacement sample hands on or None, the rerank coefficients or None, ``answer_weight`` as a finite float)."""
    import math

    _marginal_options(beam_size, beam_size is not None, num_programs, False)
    draw = _without_replacement_options(without_replacement, sample_weights, beam_size, num_programs)
    coefficients = _rerank_options(rerank, beam_size, num_programs, False, question_reconstructor, program_prior, rerank_weights)
    if beam_size is None and num_programs is None:
        raise ValueError("give the hypotheses: beam_size (a beam search) or num_programs (samples)")
    if constrained and beam_size is None:
        raise ValueError("constrained=True constrains the beam search: give a beam_size")
    if constrained_sampling and beam_size is not None:
        raise ValueError("constrained_sampling=True samples the programs; with beam_size they are searched (constrained=True)")
    try:
        w_a = float(answer_weight)
    except (TypeError, ValueError):
        raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
    if isinstance(answer_weight, bool) or not math.isfinite(w_a):
        raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
    return draw, coefficients, w_a


# the options of ``infer_programs`` and their defaults (what ``mine_supervision`` hands on)
_INFERENCE_OPTIONS = dict(beam_size=None, num_programs=None, constrained=False, constrained_sampling=False, without_replacement=False,
                          sample_weights="probability", answer_weight=1.0, rerank=False, question_reconstructor=None,
                          program_prior=None, rerank_weights=(1.0, 1.0, 0.0))


def _group_log_softmax(values, group_of, n_groups):
    """Host numpy, no loop over the groups: ``values`` [R] float64 normalised over the finite entries of each group
    (``group_of`` [R], non-decreasing, in 0 .. n_groups - 1) -- -inf for an entry that is not finite -- and per group the
    index of its first largest finite entry (-1 for a group without one)."""
    values = np.asarray(values, dtype=np.float64)
    ok = np.isfinite(values)
    kept = np.where(ok, values, -np.inf)
    top = np.full(n_groups, -np.inf)
    np.maximum.at(top, group_of, kept)
    with np.errstate(invalid="ignore", divide="ignore"):
        shifted = np.where(ok, kept - top[group_of], -np.inf)
        log_norm = np.log(np.bincount(group_of, weights=np.exp(shifted), minlength=n_groups))
        out = np.where(ok, shifted - log_norm[group_of], -np.inf)
    first = np.full(n_groups, values.size, np.int64)
    leads = np.nonzero(ok & (kept == top[group_of]))[0]
    np.minimum.at(first, group_of[leads], leads)
    return out, np.where(first < values.size, first, -1)


def _inferred_batches(program_generator, nmn, batches, beam_size, num_programs, constrained, constrained_sampling, draw,
                      coefficients, w_a, question_reconstructor, program_prior, num_batches=None):
    """The loop under ``infer_programs``, ``evaluate_program_inference`` and ``mine_supervision``: a generator of (batch, out,
    programs [R, T], group_start [B + 1]) per input batch, pipelined as ``predict_answers`` is -- batch i + 1's generator pass
    is queued before batch i's hypotheses are awaited.  ``out``: ``NeuralModuleNetwork.answer_posterior``'s dict as host numpy,
    and ``"log_prior_weight"`` [R] (the weight of a row before the answer, normalised over its question's rows),
    ``"prior_best_row"`` [B] (the MAP row without the answer term, -1 where there is none), ``"answers"`` [B] and, reranked,
    ``hypothesis_posterior``'s ``"log_reconstruction"`` and ``"log_prior"``.  The generator and the NMN are in ``eval()`` while
    the loop runs and get their state back when it ends, is closed or raises."""
    was_training = (program_generator.training, nmn.training)
    program_generator.eval()
    nmn.eval()
    try:
        constraint = None
        if constrained or constrained_sampling:
            exclude = [getattr(program_generator, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
            constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)
        copies = _HostCopies()

        def finish(batch, queued):
            reranked = None if coefficients is None else (question_reconstructor, program_prior, coefficients, batch["question"])
            B, programs, question_rows, base, _, scored = _awaited_hypotheses(nmn, queued, reranked)
            out = nmn.answer_posterior(batch["image"], torch.from_numpy(programs), question_rows, batch["answer"], base, w_a)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            start = hypothesis_rows.group_start(question_rows, B)
            if reranked is not None:  # (hypothesis_posterior's log_posterior is normalised over the question's rows already)
                out.update({k: scored[k].cpu().numpy() for k in ("log_reconstruction", "log_prior")})
                out["log_prior_weight"] = base.cpu().numpy().astype(np.float64)
                out["prior_best_row"] = scored["best_row"].cpu().numpy().astype(np.int64)
            else:
                out["log_prior_weight"], out["prior_best_row"] = _group_log_softmax(base, question_rows, B)
            out["answers"] = batch["answer"].cpu().numpy()
            return batch, out, programs, start

        pending = None
        for iteration, batch in enumerate(batches):
            queued = _queue_hypotheses(program_generator, batch, iteration, copies, beam_size, num_programs, constraint,
                                       constrained_sampling, {}, batch["image"].is_cuda, draw)
            if pending is not None:
                yield finish(*pending)
            pending = (batch, queued)
            if num_batches is not None and iteration > num_batches:
                break
        if pending is not None:
            yield finish(*pending)
    finally:
        program_generator.train(was_training[0])
        nmn.train(was_training[1])


@torch.no_grad()
def infer_programs(program_generator, nmn, batches: Iterable[Dict[str, torch.Tensor]], vocabulary, beam_size: Optional[int] = None,
                   num_programs: Optional[int] = None, constrained: bool = False, constrained_sampling: bool = False,
                   without_replacement: bool = False, sample_weights: str = "probability", answer_weight: float = 1.0,
                   rerank: bool = False, question_reconstructor=None, program_prior=None,
                   rerank_weights=(1.0, 1.0, 0.0)) -> List[Dict[str, Any]]:
    """Which program explains a question AND its known answer (not in the reference, which uses p(a | z, image) only to answer):
    the posterior over each question's program hypotheses given the answer, p(z | x, a, image) ~ w(z) p(a | z, image)^answer_weight,
    on batches with ``"question"``, ``"image"`` and ``"answer"``, one record per question.

    The hypotheses are those of ``predict_answers`` with the same options and rules: the ``beam_size`` hypotheses of a beam
    search (``constrained``: under the validity rule) or ``num_programs`` sampled ones (``constrained_sampling``;
    ``without_replacement`` / ``sample_weights``: one stochastic beam search's), invalid ones dropped and identical ones merged
    (``group_hypotheses``); one of the two is required.  The weight w(z) of a hypothesis before the answer is seen is its merged
    generator weight; with ``rerank`` (``question_reconstructor``, ``program_prior``, ``rerank_weights``: as for
    ``predict_answers``) it is ``hypothesis_posterior``'s, so that the default coefficients give the posterior under the whole
    generative model, p(x | z) p(z) p(a | z, image)^answer_weight normalised over the candidates.  ``answer_weight`` is a finite
    number; 0 leaves the answer out.  A wrong combination is a ``ValueError`` before any model is touched.

    A record holds ``"question_index"``, ``"answer"`` (the GIVEN one, as a string), ``"support"`` (hypotheses that count),
    ``"log_answer_evidence"`` (log of the summed scores: with ``answer_weight`` 1, log p(a | x, image) on the candidate set; -inf
    without support), ``"consistent_count"`` (counting hypotheses whose own answer is the given one), ``"map_program"`` and
    ``"map_answer"`` (the hypothesis with the largest posterior and its own answer; ``[]`` and ``@@UNKNOWN@@`` when there is
    none), ``"map_consistent"``, ``"first_consistent_rank"`` (position of the first consistent hypothesis among the question's
    hypotheses, None when there is none) and the ``"hypotheses"`` in group order: ``{"program", "prior_weight"`` (its share
    before the answer) ``, "weight"`` (its posterior share) ``, "log_answer_likelihood", "answer"`` (its own) ``, "consistent"}``;
    reranked, each also names its ``"log_reconstruction"`` and ``"log_prior"`` (None for a model that was not given).  The
    models are left in the ``train()`` / ``eval()`` state they were in."""
    draw, coefficients, w_a = _program_inference_options(beam_size, num_programs, constrained, constrained_sampling,
                                                         without_replacement, sample_weights, answer_weight, rerank,
                                                         question_reconstructor, program_prior, rerank_weights)
    pad = getattr(program_generator, "_pad_index", 0)
    records: List[Dict[str, Any]] = []

    def token_strings(row):
        return [vocabulary.get_token_from_index(int(t), namespace="programs") for t in row if t != pad]

    def answer_string(a):
        return vocabulary.get_token_from_index(int(a), namespace="answers")

    for batch, out, programs, start in _inferred_batches(program_generator, nmn, batches, beam_size, num_programs, constrained,
                                                         constrained_sampling, draw, coefficients, w_a, question_reconstructor,
                                                         program_prior):
        B = len(start) - 1
        index = batch["question_index"].cpu().tolist() if "question_index" in batch else range(len(records), len(records) + B)
        for i, qi in enumerate(index):
            given, best, first = int(out["answers"][i]), int(out["best_row"][i]), int(out["first_consistent_row"][i])
            hypotheses = []
            for r in range(start[i], start[i + 1]):
                own, counts = int(out["hypothesis_predictions"][r]), bool(np.isfinite(out["log_posterior"][r]))
                h = {"program": token_strings(programs[r]), "prior_weight": float(np.exp(out["log_prior_weight"][r])),
                     "weight": float(np.exp(out["log_posterior"][r])),
                     "log_answer_likelihood": float(out["log_answer_likelihood"][r]), "answer": answer_string(own),
                     "consistent": counts and own == given}
                if coefficients is not None:
                    h["log_reconstruction"] = None if question_reconstructor is None else float(out["log_reconstruction"][r])
                    h["log_prior"] = None if program_prior is None else float(out["log_prior"][r])
                hypotheses.append(h)
            map_answer = int(out["hypothesis_predictions"][best]) if best >= 0 else nmn._unknown_answer
            records.append({
                "question_index": int(qi), "answer": answer_string(given), "support": int(out["support"][i]),
                "log_answer_evidence": float(out["log_evidence"][i]), "consistent_count": int(out["consistent_count"][i]),
                "map_program": token_strings(programs[best]) if best >= 0 else [], "map_answer": answer_string(map_answer),
                "map_consistent": best >= 0 and map_answer == given,
                "first_consistent_rank": first - int(start[i]) if first >= 0 else None, "hypotheses": hypotheses})
    return records


@torch.no_grad()
def evaluate_program_inference(program_generator, nmn, batches: Iterable[Dict[str, torch.Tensor]], vocabulary=None,
                               beam_size: Optional[int] = None, num_programs: Optional[int] = None, constrained: bool = False,
                               constrained_sampling: bool = False, without_replacement: bool = False,
                               sample_weights: str = "probability", answer_weight: float = 1.0, rerank: bool = False,
                               question_reconstructor=None, program_prior=None, rerank_weights=(1.0, 1.0, 0.0),
                               num_batches: Optional[int] = None) -> Dict[str, float]:
    """Was a program that answers correctly among the hypotheses, and does the answer posterior find it?  The options are
    ``infer_programs``'; ``vocabulary`` is not needed and only kept for symmetry; ``num_batches`` stops the loop as
    ``Evaluator.evaluate`` does.  Returns, as fractions of the questions, ``"answer_recall"`` (at least one counting hypothesis
    whose own answer is the given one), ``"map_consistency"`` (the MAP hypothesis under the answer posterior answers correctly)
    and ``"proposal_consistency"`` (the question's FIRST hypothesis does: ``evaluate_marginal_answer_accuracy``'s
    ``"single_answer_accuracy"``); and ``"average_support"``, ``"average_consistent"`` and ``"average_rows_per_question"`` (NMN
    rows run per question).  Where batches carry ``"program"``, also ``"program_accuracy_with_answer"`` and
    ``"program_accuracy_without_answer"``: the fraction of those questions whose MAP program -- with the answer term, and by the
    weights before it -- is the annotated one, token for token, padding, @start@ and @end@ left out."""
    draw, coefficients, w_a = _program_inference_options(beam_size, num_programs, constrained, constrained_sampling,
                                                         without_replacement, sample_weights, answer_weight, rerank,
                                                         question_reconstructor, program_prior, rerank_weights)
    skip = [getattr(program_generator, name, default) for name, default in (("_pad_index", 0), ("_start_index", 2), ("_end_index", 3))]
    totals = {"questions": 0, "recall": 0, "map": 0, "proposal": 0, "support": 0, "consistent": 0, "rows": 0, "annotated": 0,
              "with": 0, "without": 0}

    def same_program(row, annotated):
        return [t for t in row.tolist() if t not in skip] == [t for t in annotated.tolist() if t not in skip]

    for batch, out, programs, start in _inferred_batches(program_generator, nmn, batches, beam_size, num_programs, constrained,
                                                         constrained_sampling, draw, coefficients, w_a, question_reconstructor,
                                                         program_prior, num_batches):
        answers, best, own = out["answers"], out["best_row"], out["hypothesis_predictions"]
        has = start[1:] > start[:-1]
        by_map = np.full(answers.shape[0], nmn._unknown_answer, np.int64)
        by_map[best >= 0] = own[best[best >= 0]]
        proposal = np.full(answers.shape[0], nmn._unknown_answer, np.int64)
        proposal[has] = own[start[:-1][has]]
        totals["questions"] += answers.shape[0]
        totals["recall"] += int((out["consistent_count"] > 0).sum())
        totals["map"] += int(((by_map == answers) & (best >= 0)).sum())
        totals["proposal"] += int((proposal == answers).sum())
        totals["support"] += int(out["support"].sum())
        totals["consistent"] += int(out["consistent_count"].sum())
        totals["rows"] += int(programs.shape[0])
        if "program" in batch:
            annotated = batch["program"].cpu().numpy()
            totals["annotated"] += annotated.shape[0]
            for i in range(annotated.shape[0]):
                totals["with"] += int(best[i] >= 0 and same_program(programs[best[i]], annotated[i]))
                before = int(out["prior_best_row"][i])
                totals["without"] += int(before >= 0 and same_program(programs[before], annotated[i]))
    n = max(totals["questions"], 1)
    result = {"answer_recall": totals["recall"] / n, "map_consistency": totals["map"] / n,
              "proposal_consistency": totals["proposal"] / n, "average_support": totals["support"] / n,
              "average_consistent": totals["consistent"] / n, "average_rows_per_question": totals["rows"] / n}
    if totals["annotated"]:
        result["program_accuracy_with_answer"] = totals["with"] / totals["annotated"]
        result["program_accuracy_without_answer"] = totals["without"] / totals["annotated"]
    return result


def mine_supervision(program_generator, nmn, batches: Iterable[Dict[str, torch.Tensor]], vocabulary=None, min_posterior: float = 0.9,
                     require_consistent: bool = True, **options):
    """Pseudo-supervision for the questions without a program annotation: programs that explain the question and answer it
    correctly.  A generator over ``batches`` (``"question"``, ``"image"``, ``"answer"``; ``"program"`` [B, T] and
    ``"supervision"`` [B] where some rows are annotated); ``options`` are ``infer_programs``' own, checked here -- before any
    model is touched and before the first batch is asked for.  Each batch is yielded as a shallow copy whose ``"program"`` and
    ``"supervision"`` also cover the mined rows, plus ``"mined"`` (bool [B], beside ``"supervision"``):
      * a row that is already supervised keeps its program bit for bit and is not mined;
      * an unsupervised row gets its MAP program under the answer posterior when that program's posterior share is at least
        ``min_posterior`` and -- with ``require_consistent`` -- its own answer is the given one: in the layout of the
        annotated programs (no @start@, no @end@, padding behind), padded to ``batch["program"].size(1)``; a longer one is not
        mined.  A batch without ``"program"`` gets one as wide as the decoded hypotheses; without ``"supervision"`` none of
        its rows counts as supervised.
    The input tensors are not written.  The generator and the NMN are in ``eval()`` while a batch is worked on and in the state
    they were in whenever the caller holds a batch and when the loop ends; batch i + 1's generator pass is queued before batch i
    is yielded.  ``vocabulary`` is not needed and only kept for symmetry."""
    unknown = sorted(set(options) - set(_INFERENCE_OPTIONS))
    if unknown:
        raise TypeError("mine_supervision() got options that infer_programs does not take: %s" % ", ".join(unknown))
    o = dict(_INFERENCE_OPTIONS, **options)
    draw, coefficients, w_a = _program_inference_options(
        o["beam_size"], o["num_programs"], o["constrained"], o["constrained_sampling"], o["without_replacement"], o["sample_weights"],
        o["answer_weight"], o["rerank"], o["question_reconstructor"], o["program_prior"], o["rerank_weights"])
    pad = getattr(program_generator, "_pad_index", 0)
    skip = (pad, getattr(program_generator, "_start_index", 2), getattr(program_generator, "_end_index", 3))

    @torch.no_grad()
    def mined_batches():
        was_training = (program_generator.training, nmn.training)
        for batch, out, programs, start in _inferred_batches(program_generator, nmn, batches, o["beam_size"], o["num_programs"],
                                                             o["constrained"], o["constrained_sampling"], draw, coefficients, w_a,
                                                             o["question_reconstructor"], o["program_prior"]):
            B = len(start) - 1
            if "program" in batch:
                program = batch["program"].clone()
            else:
                program = torch.full((B, programs.shape[1]), pad, dtype=torch.long, device=batch["question"].device)
            if "supervision" in batch:
                supervision = batch["supervision"].clone()
            else:
                supervision = torch.zeros(B, dtype=torch.long, device=batch["question"].device)
            supervised = supervision.cpu().numpy() != 0
            width = int(program.size(1))
            at, rows = [], []
            for i in np.nonzero(~supervised)[0].tolist():
                best = int(out["best_row"][i])
                if best < 0 or not float(np.exp(out["log_posterior"][best])) >= min_posterior:
                    continue
                if require_consistent and int(out["hypothesis_predictions"][best]) != int(out["answers"][i]):
                    continue
                tokens = [t for t in programs[best].tolist() if t not in skip]
                if len(tokens) <= width:
                    at.append(i)
                    rows.append(tokens + [pad] * (width - len(tokens)))
            mined = torch.zeros(B, dtype=torch.bool)
            if at:
                where = torch.tensor(at, dtype=torch.long)
                mined[where] = True
                program[where.to(program.device)] = torch.tensor(rows, dtype=program.dtype).to(program.device)
                supervision[where.to(supervision.device)] = 1
            result = dict(batch)
            result.update(program=program, supervision=supervision, mined=mined.to(supervision.device))
            program_generator.train(was_training[0]), nmn.train(was_training[1])
            yield result
            program_generator.eval(), nmn.eval()

    return mined_batches()


@torch.no_grad()
def sample_programs(program_prior, vocabulary, num_samples: int, max_sequence_length: int = 28, seed: Optional[int] = None,
                    temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, greedy: bool = False,
                    constrained: bool = False, compiler=None) -> List[Dict[str, Any]]:
    """Programs drawn from the prior p(z) with no question (``ProgramPrior.sample``: one persistent HIP launch), one record
    per sample, most likely first: ``"program"`` (token strings without padding, the closing @end@ included),
    ``"log_probability"`` (log p(z) of the kept tokens as ``ProgramPrior.forward`` scores them) and, with ``compiler`` (a
    ``ProgramCompiler``), whether it is a ``"program_valid"`` one.  ``seed`` makes the draw reproducible; ``temperature``,
    ``top_k``, ``top_p`` and ``greedy`` are those of ``sample``.  ``constrained`` (needs ``compiler``): the samples are
    drawn under the compiler's validity rule (``compiler.decoding_automaton``, built as ``predict_answers`` builds it), so
    every record is valid."""
    if constrained and compiler is None:
        raise ValueError("constrained=True draws under the program compiler's validity rule: give a compiler")
    sampling_filter(temperature, top_k, top_p)
    constraint = None
    if constrained:
        exclude = [getattr(program_prior, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
        constraint = compiler.decoding_automaton(exclude=exclude)
    out = program_prior.sample(num_samples, max_sequence_length, seed=seed, temperature=temperature, top_k=top_k, top_p=top_p,
                               constraint=constraint, greedy=greedy)
    programs = out["predictions"].cpu()
    log_probability = out["log_probability"].cpu().tolist()
    valid = None if compiler is None else [c.valid for c in compiler.compile_batch(programs.numpy())]
    pad = program_prior._pad_index
    records: List[Dict[str, Any]] = []
    for i, row in enumerate(programs.tolist()):
        record = {"program": [vocabulary.get_token_from_index(int(t), namespace="programs") for t in row if t != pad],
                  "log_probability": float(log_probability[i])}
        if valid is not None:
            record["program_valid"] = bool(valid[i])
        records.append(record)
    return records


@torch.no_grad()
def evaluate_question_evidence(program_generator, question_reconstructor, program_prior, batches: Iterable[Dict[str, torch.Tensor]],
                               num_samples: int = 8, constraint=None) -> Dict[str, Any]:
    """A lower bound on log p(x) of every question under the generative model p(x | z) p(z), importance sampled with the
    generator (not in the reference, which has no figure that compares checkpoints' evidence):
        bound_g = logsumexp_k(log w_k) - log K,   log w_k = log p(x_g | z_k) + log p(z_k) - log q(z_k | x_g),   z_k ~ q(. | x_g)
    with every term a true SUM over tokens (``probnmn.modules.importance_weighted``, beta = 1): E[bound_g] <= log p(x_g), it
    tightens as ``num_samples`` = K (1 .. 64) grows, and K = 1 is the ELBO.

    Per batch (``"question"`` on the device): ONE sampling decode of the generator over the questions replicated K-fold,
    question-major (``"sampling"``; with ``constraint``, a token automaton, ``"constrained_sampling"``, scored under the
    grammar-normalised q_c it draws from), the three scoring passes (``teacher_forced_logits``) and one plain
    ``pnmn_importance_bound`` launch.  No gradient; the models run in ``eval()`` mode and come back in the mode they were in;
    no metric of any model moves.  The draw takes its seed from the torch CPU generator (``torch.manual_seed`` makes the
    call reproducible).

    Returns ``"log_evidence_bound"`` (the mean bound over the questions that count: all K rows with a finite weight),
    ``"elbo"`` (the mean log w over the same samples: the K = 1 bound), ``"effective_sample_size"`` (mean 1 / sum share^2),
    ``"questions"`` (how many were evaluated), ``"unsupported"`` (how many of them do not count), ``"bound"`` (fp32, one
    entry per question in batch order; -inf for a question that does not count) and ``"log_weight"`` (fp32 [questions, K]:
    log w of every sample)."""
    from probnmn.modules.importance_weighted import check_samples, importance_weighted_bound
    from probnmn.trainers.joint_training import check_constraint
    from probnmn.trainers.marginal_training import candidate_targets

    K = check_samples(num_samples)
    constraint = check_constraint(constraint)
    pg, qr, prior = program_generator, question_reconstructor, program_prior
    models = (pg, qr, prior)
    was_training = [m.training for m in models]
    for m in models:
        m.eval()
    bounds, weights, sums = [], [], None
    try:
        for batch in batches:
            question = batch["question"]
            if question.device.type != "cuda":
                raise _hip.HipLibraryError("evaluate_question_evidence runs on the ROCm device the questions are on (got %s); "
                                           "there is no CPU path" % question.device)
            questions = question.repeat_interleave(K, 0) if K > 1 else question
            if constraint is None:
                programs = pg(questions, decoding_strategy="sampling")["predictions"]
            else:
                programs = pg(questions, decoding_strategy="constrained_sampling", constraint=constraint)["predictions"]
            targets = candidate_targets(programs, pg)
            q_logits, q_targets = pg.teacher_forced_logits(questions, targets, constraint=constraint)
            x_logits, x_targets = qr.teacher_forced_logits(targets, questions)
            p_logits, p_targets = prior.teacher_forced_logits(targets)
            loss, stats = importance_weighted_bound((x_logits, x_targets, qr._pad_index), (q_logits, q_targets, pg._pad_index),
                                                    (p_logits, p_targets, prior._pad_index), samples=K, beta=1.0)
            counts = stats["support"] == K
            bound = torch.where(counts, -loss, torch.full_like(loss, -float("inf")))
            bounds.append(bound)
            weights.append(stats["log_weight"].view(-1, K))
            zero = torch.zeros_like(loss)
            log_w = torch.where(counts.repeat_interleave(K), stats["log_weight"], torch.zeros_like(stats["log_weight"]))
            part = torch.stack((torch.where(counts, bound, zero).sum().double(), log_w.sum().double() / K,
                                stats["ess"].sum().double(), counts.sum().double()))
            sums = part if sums is None else sums + part
    finally:
        for m, training in zip(models, was_training):
            m.train(training)
    if sums is None:
        nan = float("nan")
        return {"log_evidence_bound": nan, "elbo": nan, "effective_sample_size": nan, "questions": 0, "unsupported": 0,
                "bound": torch.zeros(0), "log_weight": torch.zeros(0, K)}
    total, elbo, ess, n = sums.tolist()
    bound = torch.cat(bounds)
    n = int(n)
    div = lambda v: v / n if n else float("nan")  # noqa: E731
    return {"log_evidence_bound": div(total), "elbo": div(elbo), "effective_sample_size": div(ess),
            "questions": int(bound.numel()), "unsupported": int(bound.numel()) - n, "bound": bound,
            "log_weight": torch.cat(weights)}


@torch.no_grad()
def evaluate_joint_evidence(program_generator, question_reconstructor, program_prior, nmn, batches: Iterable[Dict[str, torch.Tensor]],
                            vocabulary=None, num_samples: int = 8, constraint=None, answer_weight: float = 1.0) -> Dict[str, Any]:
    """A lower bound on log p(x, a | image) of every question and its answer under the generative model
    p(x | z) p(a | z, image) p(z), importance sampled with the generator, and the answers of that model's POSTERIOR over
    programs (not in the reference, which answers from the proposal: one program of the generator per question):
        bound_g = logsumexp_k(log w_k) - log K,   z_k ~ q(. | x_g),
        log w_k = log p(x_g | z_k) + answer_weight log p(a_g | z_k, image_g) + log p(z_k) - log q(z_k | x_g)
    with every sequence term a true SUM over tokens (``probnmn.modules.importance_weighted``, beta = 1; an invalid program
    answers uniformly: log p(a | z) = -log A).  With ``answer_weight`` 1, E[bound_g] <= log p(x_g, a_g | image_g), and it
    tightens as ``num_samples`` = K (1 .. 64) grows.

    Per batch (``"question"``, ``"answer"`` and ``"image"`` -- feature maps or a ``ResidentRows`` batch -- on the device): ONE
    sampling decode of the generator over the questions replicated K-fold, question-major (``"sampling"``; with
    ``constraint``, a token automaton, ``"constrained_sampling"``, scored under the grammar-normalised q_c it draws from),
    the three scoring passes, ONE module-network pass over the K n sampled rows (``nmn.hypothesis_answer_logits``: each row
    reads its question's feature map in place), two plain ``pnmn_importance_bound_joint`` launches -- the joint weights, and
    with the answer's weight 0 the question-only ones, log w^x_k -- and two ``pnmn_answer_marginal`` launches over each
    question's rows: with log w^x as the row weights, the self-normalised importance-sampling estimate of the generative
    model's answer  p(a | x, image) ~= sum_k share^x_k p(a | z_k, image), and with uniform weights the proposal's (invalid
    programs are left out of both sums).  No gradient; the models run in ``eval()`` mode and come back in the mode they were
    in; no metric of any model moves.  The draw takes its seed from the torch CPU generator.  ``vocabulary`` is not needed
    and only kept for symmetry with ``predict_answers``.

    Returns ``"log_joint_evidence_bound"`` (the mean bound on log p(x, a | image) over the questions whose K rows all have a
    finite joint weight), ``"log_evidence_bound"`` (the mean bound on log p(x) from the same samples, over the same
    questions), ``"log_answer_given_question"`` (their difference: an ESTIMATE of log p(a | x, image), the difference of two
    lower bounds, not itself a bound), ``"effective_sample_size"`` (of the joint weights), ``"posterior_answer_accuracy"``
    (the arg-max of sum_k share^x_k p(. | z_k, image) against the answer), ``"proposal_answer_accuracy"`` (the same with
    uniform weights) -- both over ALL the questions asked, those that do not count included, where the three figures before
    them are means over the questions that count --, ``"questions"``, ``"unsupported"`` (questions that do not count), ``"bound"`` (fp32, one entry per
    question in batch order; -inf for one that does not count) and ``"log_weight"`` (fp32 [questions, K]: the joint log w of
    every sample)."""
    from probnmn.modules.importance_weighted import check_answer_weight, check_samples, joint_importance_weighted_bound
    from probnmn.trainers.joint_training import check_constraint
    from probnmn.trainers.marginal_training import candidate_targets

    K = check_samples(num_samples)
    constraint = check_constraint(constraint)
    gamma = check_answer_weight(answer_weight)
    pg, qr, prior = program_generator, question_reconstructor, program_prior
    models = (pg, qr, prior, nmn)
    was_training = [m.training for m in models]
    for m in models:
        m.eval()
    bounds, weights, sums = [], [], None
    try:
        for batch in batches:
            question = batch["question"]
            if question.device.type != "cuda":
                raise _hip.HipLibraryError("evaluate_joint_evidence runs on the ROCm device the questions are on (got %s); "
                                           "there is no CPU path" % question.device)
            dev, n = question.device, int(question.size(0))
            questions = question.repeat_interleave(K, 0) if K > 1 else question
            if constraint is None:
                programs = pg(questions, decoding_strategy="sampling")["predictions"]
            else:
                programs = pg(questions, decoding_strategy="constrained_sampling", constraint=constraint)["predictions"]
            targets = candidate_targets(programs, pg)
            q_logits, q_targets = pg.teacher_forced_logits(questions, targets, constraint=constraint)
            x_logits, x_targets = qr.teacher_forced_logits(targets, questions)
            p_logits, p_targets = prior.teacher_forced_logits(targets)
            qrows = np.repeat(np.arange(n, dtype=np.int64), K)
            answered = nmn.hypothesis_answer_logits(batch["image"], programs, qrows)
            logits, valid = answered["answer_logits"].contiguous(), answered["valid"]
            answers = batch["answer"].to(device=dev, dtype=torch.long)
            terms = ((x_logits, x_targets, qr._pad_index), (q_logits, q_targets, pg._pad_index), (p_logits, p_targets, prior._pad_index))
            loss, stats = joint_importance_weighted_bound(*terms, answer=(logits, answers, valid), samples=K, beta=1.0,
                                                          answer_weight=gamma, unknown_index=int(nmn._unknown_answer))
            x_loss, x_stats = joint_importance_weighted_bound(*terms, answer=(logits, answers, valid), samples=K, beta=1.0,
                                                              answer_weight=0.0, unknown_index=int(nmn._unknown_answer))
            # the answers of the posterior (rows weighed by the question-only log w) and of the proposal (uniform weights)
            A = int(logits.size(1))
            group_start = hypothesis_rows.group_start_on_device(qrows, n, dev)
            answered_by = {}
            for name, row_weights in (("posterior", x_stats["log_weight"]), ("proposal", None)):
                m_out = {"predictions": torch.empty(n, dtype=torch.long, device=dev),
                         "log_probabilities": torch.empty(n, A, dtype=torch.float32, device=dev),
                         "hypothesis_predictions": torch.empty(n * K, dtype=torch.long, device=dev),
                         "hypothesis_weights": torch.empty(n * K, dtype=torch.float32, device=dev),
                         "support": torch.empty(n, dtype=torch.int32, device=dev)}
                _hip.check(_hip.lib().pnmn_answer_marginal(
                    logits.data_ptr(), valid.data_ptr(), 0 if row_weights is None else row_weights.data_ptr(), group_start.data_ptr(),
                    m_out["log_probabilities"].data_ptr(), m_out["predictions"].data_ptr(), m_out["hypothesis_predictions"].data_ptr(),
                    m_out["hypothesis_weights"].data_ptr(), m_out["support"].data_ptr(), n, n * K, A, nmn._unknown_answer,
                    _hip.stream_ptr(dev)), "answer_marginal")
                answered_by[name] = (m_out["predictions"] == answers).sum().double()
            counts = stats["support"] == K
            bound = torch.where(counts, -loss, torch.full_like(loss, -float("inf")))
            bounds.append(bound)
            weights.append(stats["log_weight"].view(-1, K))
            zero = torch.zeros_like(loss)
            # (a question whose joint weights are finite has finite question-only weights: the same terms, one fewer)
            part = torch.stack((torch.where(counts, bound, zero).sum().double(), torch.where(counts, -x_loss, zero).sum().double(),
                                stats["ess"].sum().double(), counts.sum().double(), answered_by["posterior"],
                                answered_by["proposal"]))
            sums = part if sums is None else sums + part
    finally:
        for m, training in zip(models, was_training):
            m.train(training)
    if sums is None:
        nan = float("nan")
        return {"log_joint_evidence_bound": nan, "log_evidence_bound": nan, "log_answer_given_question": nan,
                "effective_sample_size": nan, "posterior_answer_accuracy": nan, "proposal_answer_accuracy": nan, "questions": 0,
                "unsupported": 0, "bound": torch.zeros(0), "log_weight": torch.zeros(0, K)}
    joint, evidence, ess, n, posterior, proposal = sums.tolist()
    bound = torch.cat(bounds)
    n, asked = int(n), int(bound.numel())
    div = lambda v: v / n if n else float("nan")  # noqa: E731
    return {"log_joint_evidence_bound": div(joint), "log_evidence_bound": div(evidence),
            "log_answer_given_question": div(joint) - div(evidence), "effective_sample_size": div(ess),
            "posterior_answer_accuracy": posterior / max(asked, 1), "proposal_answer_accuracy": proposal / max(asked, 1),
            "questions": asked, "unsupported": asked - n, "bound": bound, "log_weight": torch.cat(weights)}
