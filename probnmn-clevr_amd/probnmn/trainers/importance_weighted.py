"""Question coding on the importance-weighted bound (not in the reference, whose question-coding trainer takes one sampled
program per question through a single-sample ELBO of per-token mean losses: probnmn/trainers/question_coding_trainer.py,
modules/elbo.py):

    L_g = -(logsumexp_k log w_k - log K),   log w_k = log p(x_g | z_k) + beta (log p(z_k) - log q(z_k | x_g)),   z_k ~ q(. | x_g)

over K programs per unsupervised question, every term a true sum over tokens: with beta = 1, -L_g is a lower bound on
log p(x_g) in expectation that tightens as K grows.  The reconstructor gets the exact gradient of L_g; the generator the VIMCO
estimate (Mnih & Rezende 2016): each sample's score-function gradient weighted by the bound minus a baseline built from the
question's OTHER samples, minus beta times the sample's share of the weight (``probnmn.modules.importance_weighted``).  The
supervised rows add the question-coding step's own alpha-weighted teacher-forced cross entropies."""
from typing import Any, Dict

import torch

from probnmn import parallel
from probnmn.modules.importance_weighted import check_beta, check_samples, importance_weighted_bound
from .joint_training import _TrainerBase, _dp_weight, _index_to_device, _replicate, _split_supervision, check_constraint
from .marginal_training import candidate_targets


def importance_weighted_options(num_samples, beta, constraint):
    """The argument rules of ``ImportanceWeightedCodingStep``; touches no device and no model.  Returns (K, beta as a float,
    constraint); ``ValueError`` otherwise.  ``num_samples``: an integer in 2 .. 64 (one sample has no other sample to take a
    baseline from: ``evaluate_question_evidence`` covers K = 1); ``beta``: finite and not negative; ``constraint``: None or a
    token automaton."""
    return check_samples(num_samples, least=2), check_beta(beta), check_constraint(constraint)


def refuse_generator_dropout(program_generator) -> None:
    """Samples and scores must come from the same q: a generator whose encoder LSTM drops activations would sample under one
    mask and be scored under another, which is not one distribution.  ``ValueError`` for dropout p > 0."""
    p = float(program_generator._encoder._module.dropout)
    if p > 0.0:
        raise ValueError("the program generator's encoder has LSTM dropout %g: the importance weights divide by the q the "
                         "programs were drawn from, and a mask while sampling and another while scoring is not one "
                         "distribution -- build the generator with dropout 0" % p)


class ImportanceWeightedCodingStep(_TrainerBase):
    """One iteration:

    1. supervised rows -- the question-coding step's own passes (``_seq2seq_passes(supervised=True, sampled=False)``):
       ``w_sup * alpha * (program generation + question reconstruction)`` cross entropies;
    2. unsupervised rows, replicated K-fold question-major -- ONE sampling decode of the generator under ``no_grad``
       (``"sampling"``; with ``constraint`` ``"constrained_sampling"``, and the scores below are then under the
       grammar-normalised q_c the draw came from); the predictions become targets (``candidate_targets``) and are scored by
       ``program_generator.teacher_forced_logits(..., differentiable=True, constraint=)``,
       ``question_reconstructor.teacher_forced_logits(targets, questions, differentiable=True)`` and, under ``no_grad``,
       ``program_prior.teacher_forced_logits(targets)``; ``importance_weighted_bound`` turns the three into L_g and the
       gradients of all logits in one launch; the loss is the mean over the questions (a question with a row whose weight
       is not finite pays ``INVALID_PROGRAM_LOSS``, without a gradient);
    3. backward, the data-parallel gradient all-reduce, the clamp to [-5, 5] and Adam over the generator and the
       reconstructor.  The prior stays in ``eval()`` mode and gets no gradient.

    ``step`` reports ``"objective"``, ``"bound"`` (the mean bound of the questions that count; NaN without one),
    ``"effective_sample_size"`` (their mean 1 / sum share^2, between 1 and K), ``"signal_variance"`` (the variance of the
    generator's learning signal over their rows), ``"unsupported"`` (questions that do not count), ``"programs"`` (the
    sampled rows), ``"samples_per_question"`` and the supervised ``"loss"`` dict.  Eager passes: there is no ``Seq2SeqPlan``
    for this iteration.  Samples are drawn with replacement; alpha's scale against a bound in nats per question is the
    question-coding default, not tuned."""

    use_plan = False

    def __init__(self, program_generator, question_reconstructor, program_prior, num_samples: int = 4, beta: float = 1.0,
                 alpha: float = 100.0, constraint=None, lr: float = 1e-3, weight_decay: float = 0.0, lr_gamma: float = 0.5,
                 lr_patience: int = 3):
        self.num_samples, self.beta, self.constraint = importance_weighted_options(num_samples, beta, constraint)
        refuse_generator_dropout(program_generator)
        self.pg, self.qr, self.prior = program_generator, question_reconstructor, program_prior
        self.alpha = alpha
        self.prior.eval()
        self.models = {"program_generator": self.pg, "question_reconstructor": self.qr}
        self.optimizer = self._make_optimizer([self.pg, self.qr], lr, weight_decay)
        self._init_schedule(lr_gamma, lr_patience)
        self.iteration = 0

    def _sample(self, questions: torch.Tensor) -> torch.Tensor:
        """One program per row of ``questions`` from the generator as it is (``train()`` mode, no dropout to differ by), no
        graph: the rows are trimmed behind their first @end@."""
        with torch.no_grad():
            if self.constraint is None:
                return self.pg(questions, decoding_strategy="sampling")["predictions"]
            return self.pg(questions, decoding_strategy="constrained_sampling", constraint=self.constraint)["predictions"]

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        self.optimizer.zero_grad()
        for m in (self.pg, self.qr):
            if not m.training:
                m.train()
        K = self.num_samples
        dev = batch["question"].device
        sup, nosup = _split_supervision(batch["supervision"])
        n_questions = int(nosup.numel())
        sup_d, nosup_d = _index_to_device(sup, dev), _index_to_device(_replicate(nosup, K), dev)
        # data parallel: both weights on every rank, whatever its shard holds (the same collectives in the same order)
        w_sup, w_nosup = _dp_weight(sup.numel(), dev), parallel.mean_weight(n_questions, dev)
        out: Dict[str, Any] = {"samples_per_question": K}
        loss = torch.zeros((), device=dev)

        p = self._seq2seq_passes(batch, sup_d, nosup_d, supervised=True, sampled=False, prior=False)
        self._split_means(p)
        if "pg_sup" in p:
            loss = loss + w_sup * self.alpha * (p["pg_sup"] + p["qr_sup"])
            out["loss"] = {"program_generation_gt": p["pg_sup"].detach(), "question_reconstruction_gt": p["qr_sup"].detach()}
        if "grammar" in p:
            out["grammar"] = p["grammar"]

        if n_questions:
            questions = batch["question"].index_select(0, nosup_d)
            programs = self._sample(questions)
            targets = candidate_targets(programs, self.pg)
            q_logits, q_targets = self.pg.teacher_forced_logits(questions, targets, differentiable=True, constraint=self.constraint)
            x_logits, x_targets = self.qr.teacher_forced_logits(targets, questions, differentiable=True)
            with torch.no_grad():  # frozen model
                p_logits, p_targets = self.prior.teacher_forced_logits(targets)
            loss_rows, stats = importance_weighted_bound(
                (x_logits, x_targets, self.qr._pad_index), (q_logits, q_targets, self.pg._pad_index),
                (p_logits, p_targets, self.prior._pad_index), samples=K, beta=self.beta)
            loss = loss + loss_rows.mean() * w_nosup
            counts = stats["support"] == K
            n = counts.sum()
            rows = counts.repeat_interleave(K)
            n_rows = (n * K).clamp(min=1)
            signal = torch.where(rows, stats["signal"], torch.zeros_like(stats["signal"]))
            mean_signal = signal.sum() / n_rows
            out.update({
                "bound": torch.where(counts, -loss_rows.detach(), torch.zeros_like(loss_rows)).sum() / n,
                "effective_sample_size": stats["ess"].sum() / n,  # (0 for a question that does not count)
                "signal_variance": torch.where(rows, (signal - mean_signal) ** 2, torch.zeros_like(signal)).sum() / n_rows,
                "unsupported": n_questions - n, "programs": programs})
        self._finish(loss)
        out["objective"] = loss.detach()
        return out


def importance_weighted_joint_options(num_samples, beta, answer_weight, constraint, train_modules):
    """The argument rules of ``ImportanceWeightedJointStep``; touches no device and no model.  Returns (K, beta, answer_weight
    as floats, constraint, train_modules); ``ValueError`` otherwise.  ``num_samples``, ``beta``, ``constraint``: as for
    ``ImportanceWeightedCodingStep``; ``answer_weight``: finite and not negative; ``train_modules``: a bool."""
    from probnmn.modules.importance_weighted import check_answer_weight

    K, beta, constraint = importance_weighted_options(num_samples, beta, constraint)
    if not isinstance(train_modules, bool):
        raise ValueError("train_modules must be True or False, got %r" % (train_modules,))
    return K, beta, check_answer_weight(answer_weight), constraint, train_modules


class ImportanceWeightedJointStep(_TrainerBase):
    """Joint training on the importance-weighted bound on log p(x, a | image) (not in the reference, whose joint trainer adds
    the answer's cross entropy of one sampled program to a single-sample ELBO of per-token mean losses:
    probnmn/trainers/joint_training_trainer.py, modules/elbo.py):

        L_g = -(logsumexp_k log w_k - log K),
        log w_k = log p(x_g | z_k) + answer_weight log p(a_g | z_k, image_g) + beta (log p(z_k) - log q(z_k | x_g)),  z_k ~ q(. | x_g)

    One iteration:

    1. supervised rows -- as in ``ImportanceWeightedCodingStep``: ``w_sup * alpha * (program generation + question
       reconstruction)`` cross entropies;
    2. unsupervised rows, replicated K-fold question-major -- ONE sampling decode of the generator under ``no_grad`` (under
       ``constraint`` when one is given, and then scored under the grammar-normalised q_c the draw came from); the three
       scoring passes of ``ImportanceWeightedCodingStep``; ``nmn.hypothesis_answer_logits`` over the sampled rows, each
       reading its question's feature map in place, under ``set_grad_enabled(train_modules)``;
       ``joint_importance_weighted_bound`` turns the four logits tensors into L_g and all their gradients in one launch
       (an invalid program answers uniformly: log p(a | z) = -log A); the loss is the mean over the questions (a question
       with a row whose weight is not finite pays ``INVALID_PROGRAM_LOSS``, without a gradient);
    3. backward, the data-parallel gradient all-reduce, the clamp to [-5, 5] and Adam over the generator, the reconstructor
       and, with ``train_modules``, the module network.  The reconstructor and the modules get the exact gradient of L_g, the
       generator the VIMCO estimate -- whose signal now holds the answer, so the generator learns from answers.  The prior
       stays in ``eval()`` mode and gets no gradient.

    ``step`` reports the coding step's keys -- ``"objective"``, ``"bound"``, ``"effective_sample_size"``,
    ``"signal_variance"``, ``"unsupported"``, ``"programs"``, ``"samples_per_question"``, the supervised ``"loss"`` dict --
    plus ``"answer_accuracy"`` (the mean over the sampled rows of the row's own answer being the question's),
    ``"posterior_answer_accuracy"`` (the same weighted by share, over the questions that count; NaN without one) and
    ``"invalid_rows"`` (sampled rows whose program is invalid).  Eager passes: there is no ``Seq2SeqPlan`` for this
    iteration, and the stem runs once per sampled row.  Samples are drawn with replacement; alpha's scale against a bound in
    nats per question is the question-coding default, not tuned."""

    use_plan = False

    def __init__(self, program_generator, question_reconstructor, program_prior, nmn, num_samples: int = 4, beta: float = 1.0,
                 answer_weight: float = 1.0, alpha: float = 100.0, constraint=None, train_modules: bool = True,
                 lr: float = 1e-3, weight_decay: float = 0.0, lr_gamma: float = 0.5, lr_patience: int = 3):
        self.num_samples, self.beta, self.answer_weight, self.constraint, self.train_modules = importance_weighted_joint_options(
            num_samples, beta, answer_weight, constraint, train_modules)
        refuse_generator_dropout(program_generator)
        self.pg, self.qr, self.prior, self.nmn = program_generator, question_reconstructor, program_prior, nmn
        self.alpha = alpha
        self.prior.eval()
        self.models = {"program_generator": self.pg, "question_reconstructor": self.qr}
        trained = [self.pg, self.qr]
        if self.train_modules:
            self.models["nmn"] = self.nmn
            trained.append(self.nmn)
        self.optimizer = self._make_optimizer(trained, lr, weight_decay)
        self._init_schedule(lr_gamma, lr_patience)
        self.iteration = 0

    _sample = ImportanceWeightedCodingStep._sample

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, Any]:
        from probnmn.modules.importance_weighted import joint_importance_weighted_bound

        self.optimizer.zero_grad()
        for m in (self.pg, self.qr) + ((self.nmn,) if self.train_modules else ()):
            if not m.training:
                m.train()
        K = self.num_samples
        dev = batch["question"].device
        sup, nosup = _split_supervision(batch["supervision"])
        n_questions = int(nosup.numel())
        rows_host = _replicate(nosup, K)
        sup_d, nosup_d = _index_to_device(sup, dev), _index_to_device(rows_host, dev)
        # data parallel: both weights on every rank, whatever its shard holds (the same collectives in the same order)
        w_sup, w_nosup = _dp_weight(sup.numel(), dev), parallel.mean_weight(n_questions, dev)
        out: Dict[str, Any] = {"samples_per_question": K}
        loss = torch.zeros((), device=dev)

        p = self._seq2seq_passes(batch, sup_d, nosup_d, supervised=True, sampled=False, prior=False)
        self._split_means(p)
        if "pg_sup" in p:
            loss = loss + w_sup * self.alpha * (p["pg_sup"] + p["qr_sup"])
            out["loss"] = {"program_generation_gt": p["pg_sup"].detach(), "question_reconstruction_gt": p["qr_sup"].detach()}
        if "grammar" in p:
            out["grammar"] = p["grammar"]

        if n_questions:
            questions = batch["question"].index_select(0, nosup_d)
            programs = self._sample(questions)
            targets = candidate_targets(programs, self.pg)
            q_logits, q_targets = self.pg.teacher_forced_logits(questions, targets, differentiable=True, constraint=self.constraint)
            x_logits, x_targets = self.qr.teacher_forced_logits(targets, questions, differentiable=True)
            with torch.no_grad():  # frozen model
                p_logits, p_targets = self.prior.teacher_forced_logits(targets)
            with torch.set_grad_enabled(self.train_modules):
                # (the batch's feature maps, read in place: row r belongs to example rows_host[r], K rows per question)
                answered = self.nmn.hypothesis_answer_logits(batch["image"], programs, rows_host)
            answers = batch["answer"].index_select(0, _index_to_device(nosup, dev)).to(torch.long)
            loss_rows, stats = joint_importance_weighted_bound(
                (x_logits, x_targets, self.qr._pad_index), (q_logits, q_targets, self.pg._pad_index),
                (p_logits, p_targets, self.prior._pad_index), answer=(answered["answer_logits"], answers, answered["valid"]),
                samples=K, beta=self.beta, answer_weight=self.answer_weight, unknown_index=int(self.nmn._unknown_answer))
            loss = loss + loss_rows.mean() * w_nosup
            counts = stats["support"] == K
            n = counts.sum()
            rows = counts.repeat_interleave(K)
            n_rows = (n * K).clamp(min=1)
            signal = torch.where(rows, stats["signal"], torch.zeros_like(stats["signal"]))
            mean_signal = signal.sum() / n_rows
            right = (stats["row_predictions"] == answers.repeat_interleave(K)).to(torch.float32)
            out.update({
                "bound": torch.where(counts, -loss_rows.detach(), torch.zeros_like(loss_rows)).sum() / n,
                "effective_sample_size": stats["ess"].sum() / n,  # (0 for a question that does not count)
                "signal_variance": torch.where(rows, (signal - mean_signal) ** 2, torch.zeros_like(signal)).sum() / n_rows,
                "unsupported": n_questions - n, "programs": programs,
                "answer_accuracy": right.mean(),
                "posterior_answer_accuracy": (stats["share"] * right).sum() / n,  # (share is 0 where a question does not count)
                "invalid_rows": (answered["valid"] == 0).sum()})
        elif self.train_modules:
            for a in self.optimizer.arenas:  # no NMN backward on this rank, which is what zeroes them
                a.grad.zero_()
        self._finish(loss)
        out["objective"] = loss.detach()
        return out
