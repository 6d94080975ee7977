"""Joint training of the program generator and the modules on the marginal likelihood of the answer over the generator's
own candidate programs (the maximum marginal likelihood objective of weakly supervised semantic parsing, with the generator
as the parser; not in the reference, which trains the generator by REINFORCE on one sampled program per question:
probnmn/trainers/joint_training_trainer.py, modules/elbo.py):

    L_g = -log sum_{r in S_g} q(z_r | x_g) p(a_g | z_r, image_g)^answer_weight

S_g: the distinct valid programs ONE decode of the generator proposes for question g.  q(z_r | x): the generator's
teacher-forced sequence probability, NOT renormalised over the candidates -- mass moved onto the candidate set is rewarded,
and with ``answer_weight`` 1 L_g is an upper bound on -log p(a | x, image).  d L_g / d log q(z_r | x) = -p(z_r | x, a, image)
and d L_g / d log p(a | z_r, image) = -answer_weight p(z_r | x, a, image): a program that explains the answer is made more
likely and its modules are trained, the others are left alone."""
import math
from typing import Any, Dict

import torch

from probnmn import hypothesis_rows, parallel
from probnmn.modules.marginal_likelihood import sequence_marginal_loss
from probnmn.modules.seq2seq_base import Seq2SeqBase
from .joint_training import _TrainerBase


def marginal_joint_options(beam_size, constrained, without_replacement, answer_weight, train_modules,
                           grammar_normalised=False) -> float:
    """The argument rules of ``MarginalJointStep``; touches no device and no model.  Returns ``answer_weight`` as a float;
    ``ValueError`` otherwise.  ``beam_size``: one of ``Seq2SeqBase.BEAM_SIZES``; ``constrained``, ``without_replacement``,
    ``train_modules`` and ``grammar_normalised``: booleans; ``answer_weight``: a finite number.  ``grammar_normalised``
    scores the candidates under the automaton the search ran under: it needs ``constrained``."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or beam_size not in Seq2SeqBase.BEAM_SIZES:
        raise ValueError("beam_size must be one of %s, got %r" % (Seq2SeqBase.BEAM_SIZES, beam_size))
    for name, flag in (("constrained", constrained), ("without_replacement", without_replacement), ("train_modules", train_modules),
                       ("grammar_normalised", grammar_normalised)):
        if not isinstance(flag, bool):
            raise ValueError("%s must be True or False, got %r" % (name, flag))
    if grammar_normalised and not constrained:
        raise ValueError("grammar_normalised=True scores the candidates under the validity rule: it needs constrained=True")
    try:
        w_a = float(answer_weight)
    except (TypeError, ValueError):
        raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
    if isinstance(answer_weight, bool) or not math.isfinite(w_a):
        raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
    return w_a


def candidate_targets(programs: torch.Tensor, program_generator) -> torch.Tensor:
    """Rows a decoder returned (each kept up to and including its first @end@) as teacher-forcing targets of the same model:
    the @end@ is taken off, because teacher forcing appends the boundary @end@ itself.  A row's teacher-forced sequence score
    is then the one its decode gave it (``beam_log_probabilities``), its @end@ scored once; a row that ran out of steps
    without one pays for the @end@ it never emitted."""
    return programs.masked_fill(programs == program_generator._end_index, program_generator._pad_index)


class MarginalJointStep(_TrainerBase):
    """One iteration:

    1. candidates -- ONE decode of the generator under ``no_grad`` in ``eval()`` mode: a beam of ``beam_size``
       (``without_replacement``: a stochastic beam search, so the candidate set explores; ``constrained``: under the program
       compiler's validity rule); invalid programs are dropped and identical ones merged
       (``hypothesis_rows.queue_hypotheses`` / ``awaited_hypotheses``).  The decode's own weights are not used;
    2. ``program_generator.teacher_forced_logits(question[rows], programs, differentiable=True)``: logits [R, T, V] with a
       graph (``candidate_targets``: the programs without the @end@ their decode left on them);
    3. ``nmn.answer_log_likelihood``: log p(a | z_r, image) [R] -- with a graph, or under ``no_grad`` and constant when
       ``train_modules`` is False;
    4. ``sequence_marginal_loss(x=(logits, targets, pad), log_q=log_answer, weights=(1, 0, answer_weight))``: L_g, its
       posterior over the candidates and d L_g / d logits in one launch; the loss is the mean over the batch's questions (a
       question without a valid candidate pays ``INVALID_PROGRAM_LOSS``, without a gradient);
    5. backward, the data-parallel gradient all-reduce, the clamp to [-5, 5] and Adam over both models (the generator alone
       without ``train_modules``), as ``ModuleTrainingStep`` runs them.

    ``grammar_normalised`` (needs ``constrained``): step 2 passes the search's automaton to ``teacher_forced_logits``, so
    q above is q_c, the generator's distribution renormalised over the valid programs (``probnmn.modules.grammar``), and L_g
    sums q_c over the candidates: mass the generator puts on invalid programs no longer counts against the candidate set.

    ``step`` reports ``"loss"``, ``"support"`` (the mean number of candidates that count per question), ``"rows"`` (R) and
    ``"posterior_on_map"`` (the mean over the supported questions of the largest posterior share: how peaked the answer
    makes the candidates; NaN without a supported question).  Candidates are searched, never sampled with replacement:
    merged samples would be weighted by their counts, which is not q."""

    def __init__(self, program_generator, nmn, beam_size: int = 4, constrained: bool = False, without_replacement: bool = False,
                 answer_weight: float = 1.0, train_modules: bool = True, lr: float = 1e-4, weight_decay: float = 0.0,
                 lr_gamma: float = 0.5, lr_patience: int = 1000000, grammar_normalised: bool = False):
        self.answer_weight = marginal_joint_options(beam_size, constrained, without_replacement, answer_weight, train_modules,
                                                    grammar_normalised)
        self.beam_size, self.constrained, self.without_replacement = beam_size, constrained, without_replacement
        self.grammar_normalised = grammar_normalised
        self.train_modules = train_modules
        self._constraint = None
        self._copies = hypothesis_rows.HostCopies()
        self.pg, self.nmn = program_generator, nmn
        # this iteration has the chip to itself: no CU budget left over from a joint step that ran the same network's trunk
        # beside its seq2seq passes
        nmn.engine.conv_cus = nmn.engine.wgrad_cus = 0
        self.optimizer = self._make_optimizer([program_generator, nmn] if train_modules else [program_generator], lr, weight_decay)
        self.models = {"program_generator": program_generator}
        if train_modules:
            self.models["nmn"] = nmn
        self._init_schedule(lr_gamma, lr_patience)
        self.iteration = 0

    def _candidates(self, batch):
        """One decode of the generator under ``no_grad`` in ``eval()`` mode: (programs [R, T] on the host, question_rows [R]),
        the distinct valid programs of the batch's questions."""
        pg = self.pg
        if self.constrained and self._constraint is None:  # built once (and cached on the compiler), as predict_answers does
            exclude = [getattr(pg, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
            self._constraint = self.nmn.engine.compiler.decoding_automaton(exclude=exclude)
        was_training = pg.training
        pg.eval()  # (a proposal: no dropout in the decode)
        try:
            with torch.no_grad():
                if self.without_replacement:
                    queued = hypothesis_rows.queue_hypotheses(pg, batch, self.iteration, self._copies, None, self.beam_size,
                                                              self._constraint, False, {}, batch["image"].is_cuda,
                                                              without_replacement="probability")
                else:
                    queued = hypothesis_rows.queue_hypotheses(pg, batch, self.iteration, self._copies, self.beam_size, None,
                                                              self._constraint, False, {}, batch["image"].is_cuda)
        finally:
            pg.train(was_training)
        _, programs, question_rows, _, _, _ = hypothesis_rows.awaited_hypotheses(self.nmn, queued)
        return torch.from_numpy(programs), question_rows

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        from probnmn import _hip
        from probnmn.models.nmn import INVALID_PROGRAM_LOSS

        self.optimizer.zero_grad()
        programs, question_rows = self._candidates(batch)
        question = batch["question"]
        dev, G, R = question.device, int(question.size(0)), int(programs.size(0))
        if not self.pg.training:
            self.pg.train()
        if self.train_modules and not self.nmn.training:
            self.nmn.train()
        if R == 0:
            # (no valid candidate anywhere: every question pays the constant, nothing has a gradient)
            if parallel.world() > 1:
                raise RuntimeError("no question of this rank's batch has a valid candidate program, so the rank has no gradient "
                                   "to all-reduce: decode with constrained=True, which returns valid programs only")
            self.iteration += 1
            return {"loss": torch.full((), INVALID_PROGRAM_LOSS, dtype=torch.float32, device=dev),
                    "support": torch.zeros((), dtype=torch.float32, device=dev), "rows": 0,
                    "posterior_on_map": torch.full((), float("nan"), dtype=torch.float32, device=dev)}
        rows_dev = _hip.to_device(question_rows, dev).view(torch.long)
        logits, targets = self.pg.teacher_forced_logits(question.index_select(0, rows_dev),
                                                        candidate_targets(programs.to(dev), self.pg), differentiable=True,
                                                        constraint=self._constraint if self.grammar_normalised else None)
        with torch.set_grad_enabled(self.train_modules):
            log_answer = self.nmn.answer_log_likelihood(batch["image"], programs, question_rows, batch["answer"])["log_answer"]
        group_start = hypothesis_rows.group_start_on_device(question_rows, G, dev)
        loss_rows, log_posterior, support = sequence_marginal_loss(
            x=(logits, targets, self.pg._pad_index), log_q=log_answer, group_start=group_start,
            weights=(1.0, 0.0, self.answer_weight))
        loss = loss_rows.mean()
        if self._early is not None:
            self._early.arm()
        # data parallel: the mean over the whole batch, exact for unequal shards (ModuleTrainingStep)
        (loss * parallel.mean_weight(loss_rows.numel(), dev)).backward()
        parallel.all_reduce_gradients(self.optimizer.arenas, self.optimizer.loose, early=self._early)
        self.optimizer.step()
        self.iteration += 1
        # the largest posterior share of every supported question (exp(-inf) = 0 for a row that does not count)
        top = torch.zeros(G, dtype=torch.float32, device=dev).scatter_reduce_(0, rows_dev, torch.exp(log_posterior), "amax")
        supported = (support > 0).float()
        return {"loss": loss.detach(), "support": support.float().mean(), "rows": R,
                "posterior_on_map": (top * supported).sum() / supported.sum()}
