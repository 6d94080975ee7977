"""One module-training iteration on one GPU (reference: probnmn/trainers/_trainer.py:135-151 and
module_training_trainer.py:88-98): zero_grad -> NMN forward on the given programs -> mean loss ->
backward -> clamp to [-5, 5] -> Adam.  Programs come from the batch (ground-truth or pre-sampled)
or, when a frozen ``program_generator`` is supplied, are sampled from it as the reference does.

``objective="marginal"`` (not in the reference): the frozen generator proposes SEVERAL programs per question and the modules
are trained on the marginal likelihood of the answer over them (``NeuralModuleNetwork.marginal_answer_loss``)."""
import math
from typing import Any, Dict, Optional

import torch

from probnmn import hypothesis_rows, parallel
from probnmn.modules.seq2seq_base import Seq2SeqBase
from probnmn.optim import ClampAdam
from ._base import StepBase

OBJECTIVES = ("sampled", "marginal")


def module_objective_options(objective, has_generator, beam_size, num_programs, constrained, answer_weight) -> float:
    """The argument rules of ``ModuleTrainingStep(objective=...)``; touches no device.  Returns ``answer_weight`` as a
    float; ``ValueError`` otherwise.  ``"sampled"`` takes none of the hypothesis options.  ``"marginal"`` needs the generator
    and exactly one of ``beam_size`` (``Seq2SeqBase.BEAM_SIZES``: 1 .. 16) and ``num_programs`` (2 .. 64), under the rules of
    ``predict_answers``: ``constrained`` constrains the beam search, so it needs ``beam_size``."""
    if objective not in OBJECTIVES:
        raise ValueError("objective must be one of %s, got %r" % (OBJECTIVES, objective))
    try:
        w_a = float(answer_weight)
    except (TypeError, ValueError):
        raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
    if not math.isfinite(w_a):
        raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
    if objective == "sampled":
        if beam_size is not None or num_programs is not None or constrained or w_a != 1.0:
            raise ValueError("beam_size, num_programs, constrained and answer_weight belong to objective=\"marginal\"; the "
                             "sampled objective trains on one program per question")
        return w_a
    if not has_generator:
        raise ValueError("objective=\"marginal\" trains on the program_generator's hypotheses: give the program_generator")
    if (beam_size is None) == (num_programs is None):
        raise ValueError("objective=\"marginal\" takes exactly one of beam_size (the hypotheses are searched) and num_programs "
                         "(they are sampled); got beam_size=%r, num_programs=%r" % (beam_size, num_programs))
    if beam_size is not None and (isinstance(beam_size, bool) or not isinstance(beam_size, int)
                                  or beam_size not in Seq2SeqBase.BEAM_SIZES):
        raise ValueError("beam_size must be one of %s, got %r" % (Seq2SeqBase.BEAM_SIZES, beam_size))
    if num_programs is not None and (isinstance(num_programs, bool) or not isinstance(num_programs, int)
                                     or not 2 <= num_programs <= 64):
        raise ValueError("num_programs must be an int in 2 .. 64, got %r" % (num_programs,))
    if constrained and beam_size is None:
        raise ValueError("constrained=True constrains the beam search: give a beam_size")
    return w_a


class ModuleTrainingStep(StepBase):
    """``objective="sampled"`` (the default): the reference's iteration.  ``objective="marginal"``: every question's
    hypotheses come from ONE decode of the frozen ``program_generator`` under ``no_grad`` -- a beam search of ``beam_size``
    (``constrained``: under the program compiler's validity rule), weighted by the beam's log-probabilities, or
    ``num_programs`` independent samples, weighted uniformly; invalid programs are dropped and identical ones merged
    (``hypothesis_rows.group_hypotheses``) --, the loss is the mean over the batch's questions of
    ``NeuralModuleNetwork.marginal_answer_loss`` (``answer_weight``: its exponent on p(a | z, image)), and backward, the
    gradient all-reduce, the clamp and Adam are the sampled iteration's.  The step then also reports ``"support"`` (the mean
    number of hypotheses that count per question) and ``"rows"`` (R, the hypothesis rows the NMN ran over); ``"metrics"`` is
    None: the marginal loss moves no metric."""

    def __init__(self, nmn, lr: float = 1e-4, weight_decay: float = 0.0, program_generator=None,
                 report_metrics: bool = False, lr_gamma: float = 0.5, lr_patience: int = 1000000, objective: str = "sampled",
                 beam_size: Optional[int] = None, num_programs: Optional[int] = None, constrained: bool = False,
                 answer_weight: float = 1.0):
        self.answer_weight = module_objective_options(objective, program_generator is not None, beam_size, num_programs,
                                                      constrained, answer_weight)
        self.objective, self.beam_size, self.num_programs, self.constrained = objective, beam_size, num_programs, bool(constrained)
        self._constraint = None
        self._copies = hypothesis_rows.HostCopies()
        self.nmn = nmn
        self.program_generator = program_generator
        self.report_metrics = report_metrics
        arena = nmn.engine.ensure_arena()
        nmn.engine.direct_grads = True  # gradients stay in the arena; the optimizer reads them there
        # this iteration has the chip to itself: no CU budget left over from a joint step that ran the same network's
        # trunk beside its seq2seq passes (bench.py's r03c record: 12.7 -> 14.1 ms with a stale budget of 192)
        nmn.engine.conv_cus = nmn.engine.wgrad_cus = 0
        self.optimizer = ClampAdam(nmn.parameters(), arenas=[arena], lr=lr, weight_decay=weight_decay, clamp=5.0)
        # data parallel: the big loose FC gradient starts its all-reduce while the trunk is still in backward
        big = [p for p in self.optimizer.loose if p.numel() >= (1 << 20)]
        self._early = parallel.early_reducer_for(big, [nmn.engine])
        self.models = {"nmn": nmn}  # (the frozen program generator is not checkpointed by this phase)
        self._init_schedule(lr_gamma, lr_patience)
        self.iteration = 0

    def _hypotheses(self, batch):
        """One decode of the frozen generator under ``no_grad``: (programs [R, T], question_rows [R], log-weights [R]), the
        valid hypotheses of the batch's questions, merged."""
        pg = self.program_generator
        if self.constrained and self._constraint is None:  # built once (and cached on the compiler), as predict_answers does
            exclude = [getattr(pg, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
            self._constraint = self.nmn.engine.compiler.decoding_automaton(exclude=exclude)
        was_training = pg.training
        pg.eval()  # (a frozen proposal: no dropout in the decode)
        try:
            with torch.no_grad():
                queued = hypothesis_rows.queue_hypotheses(pg, batch, self.iteration, self._copies, self.beam_size,
                                                          self.num_programs, self._constraint, False, {},
                                                          batch["image"].is_cuda)
        finally:
            pg.train(was_training)
        _, programs, question_rows, log_weights, _, _ = hypothesis_rows.awaited_hypotheses(self.nmn, queued)
        return torch.from_numpy(programs), question_rows, log_weights

    def _marginal_step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        self.optimizer.zero_grad()
        programs, question_rows, log_weights = self._hypotheses(batch)
        if not self.nmn.training:
            self.nmn.train()
        out = self.nmn.marginal_answer_loss(batch["image"], programs, question_rows, batch["answer"], log_weights,
                                            answer_weight=self.answer_weight)
        loss = out["loss"].mean()
        if self._early is not None:
            self._early.arm()
        weighted = loss * parallel.mean_weight(out["loss"].numel(), out["loss"].device)
        if weighted.requires_grad:
            weighted.backward()
            parallel.all_reduce_gradients(self.optimizer.arenas, self.optimizer.loose, early=self._early)
            self.optimizer.step()
        elif parallel.world() > 1:
            # (no hypothesis row anywhere on this rank: no backward ran, so the arena still holds the last step's gradients)
            raise RuntimeError("no question of this rank's batch has a valid hypothesis, so the rank has no gradient to "
                               "all-reduce: decode with constrained=True, which returns valid programs only")
        # (a single process whose batch has no valid hypothesis: every loss is the constant, the parameters stay)
        self.iteration += 1
        return {"loss": loss.detach(), "metrics": None, "support": out["support"].float().mean(), "rows": int(programs.size(0))}

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        if self.objective == "marginal":
            return self._marginal_step(batch)
        self.optimizer.zero_grad()
        if self.program_generator is not None:
            with torch.no_grad():
                programs = self.program_generator(batch["question"], decoding_strategy="sampling")["predictions"]
        else:
            programs = batch["program"]
        if not self.nmn.training:  # (Module.train() walks every submodule: 0.5 ms per step)
            self.nmn.train()
        self.nmn.report_batch_metrics = self.report_metrics
        out = self.nmn(batch["image"], programs, batch["answer"])
        loss = out["loss"].mean()
        # data parallel: the reference's loss is the mean over the whole batch (module_training_trainer.py:91);
        # weighting the local mean by n_local * world / n_global keeps that exact for unequal shards
        if self._early is not None:
            self._early.arm()
        (loss * parallel.mean_weight(out["loss"].numel(), out["loss"].device)).backward()
        parallel.all_reduce_gradients(self.optimizer.arenas, self.optimizer.loose, early=self._early)
        self.optimizer.step()
        self.iteration += 1
        return {"loss": loss.detach(), "metrics": out.get("metrics")}


class ProgramPriorStep(StepBase):
    """One program-prior iteration (reference: probnmn/trainers/program_prior_trainer.py:79-90 and
    _trainer.py:135-151): mean over the batch of the per-sequence cross entropy of the LSTM language model,
    backward, clamp to [-5, 5], Adam.  ``after_validation`` takes 1 / perplexity (higher is better), as
    program_prior_trainer.py:112 does."""

    def __init__(self, program_prior, lr: float = 1e-2, weight_decay: float = 0.0, lr_gamma: float = 0.5,
                 lr_patience: int = 3):
        self.prior = program_prior
        self.optimizer = ClampAdam(program_prior.parameters(), lr=lr, weight_decay=weight_decay, clamp=5.0)
        self.models = {"program_prior": program_prior}
        self._init_schedule(lr_gamma, lr_patience)
        self.iteration = 0

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        self.optimizer.zero_grad()
        if not self.prior.training:
            self.prior.train()
        loss_rows = self.prior(batch["program"], need_predictions=False)["loss"]
        loss = loss_rows.mean()
        (loss * parallel.mean_weight(loss_rows.numel(), loss_rows.device)).backward()
        parallel.all_reduce_gradients([], self.optimizer.loose)
        self.optimizer.step()
        self.iteration += 1
        return {"loss": loss.detach()}
