"""REINFORCE estimator and the two evidence lower bounds -- class surface of the reference's
``probnmn.modules.elbo`` (reference: probnmn/modules/elbo.py:12-280).

Arithmetic is the reference's, including what looks odd: the "moving average" baseline is
``b += decay * mean(R - b)`` (not an EMA), the surrogate is ``logq * (R - b) - beta * logq``.
Two things differ in mechanics: the baseline lives on the device (the reference's
``.mean().item()`` costs a host sync per step), and under data parallelism the batch mean that
updates it is the GLOBAL mean (sum and count are all-reduced), so every rank keeps the same
baseline -- SURVEY.md 8(e).

Multi-sample estimator (``num_samples=K``, ``baseline="leave_one_out"``): K programs are drawn per question, the rows are
question-major (row q * K + k), and a sample's reward is centred by the mean reward of the question's other K - 1 samples
(Kool et al. 2019) instead of the moving scalar: c_i = R_i - (S_q - R_i) / (K - 1).  The baseline is independent of the
sample it centres, so the gradient stays an unbiased estimate of the same objective; it needs no state and no collective.
Everything else of the arithmetic is unchanged.  ``baseline="moving"`` with K > 1 is the old estimator over K times the rows.
"""
from typing import Dict

import torch
from torch import nn

from probnmn import parallel


class Reinforce(nn.Module):
    def __init__(self, baseline_decay: float = 0.99):
        super().__init__()
        self._baseline = None  # 0-dim tensor on the reward's device; not part of state_dict (as in the reference)
        self._baseline_decay = baseline_decay

    @property
    def _reinforce_baseline(self) -> float:
        return 0.0 if self._baseline is None else float(self._baseline)

    def forward(self, inputs: torch.Tensor, reward: torch.Tensor) -> torch.Tensor:
        reward = reward.detach()
        if self._baseline is None or self._baseline.device != reward.device:
            value = 0.0 if self._baseline is None else float(self._baseline)
            self._baseline = torch.full((), value, dtype=reward.dtype, device=reward.device)
        centered = reward - self._baseline
        stats = torch.stack((centered.sum(), torch.full_like(self._baseline, float(centered.numel()))))
        stats = parallel.all_reduce_scalars(stats)
        # (a rank whose shard holds no sampled rows still takes part in the collective -- see `idle`;
        # with no rows anywhere the baseline stays where it is)
        self._baseline = self._baseline + self._baseline_decay * stats[0] / stats[1].clamp(min=1.0)
        return inputs * centered

    def idle(self, device, dtype=torch.float32) -> None:
        """Data parallel: this rank has no sampled rows in this iteration.  Takes part in the baseline's
        all-reduce with an empty contribution, so that every rank issues the same collectives and ends
        the iteration with the same baseline."""
        empty = torch.zeros(0, dtype=dtype, device=device)
        self.forward(empty, empty)


class _FusedElbo(torch.autograd.Function):
    """``pnmn_elbo_rows``: reward, centring, KL surrogate, ELBO and the five batch sums in one launch; the
    backward is analytic (d sum(elbo) / d pg_loss[n] = (R[n] - b) - beta, d / d qr_loss[n] = -1, the reward
    itself is a constant of the estimator -- reference elbo.py:28-34,76-82)."""

    @staticmethod
    def forward(ctx, pg_loss, qr_loss, prior_loss, nmn_loss, baseline, beta, gamma):
        n = pg_loss.numel()
        dev = pg_loss.device
        # (zeros, not empty: with no sampled rows the kernel returns without writing, and the means and the
        # baseline update below must then see zeros, not whatever the allocator handed out)
        sums = torch.zeros(6, dtype=torch.float32, device=dev)
        dpg = torch.empty(n, dtype=torch.float32, device=dev)
        from probnmn import _hip

        keep = [t.detach().contiguous() if t is not None else None for t in (pg_loss, qr_loss, prior_loss, nmn_loss)]
        _hip.check(_hip.lib().pnmn_elbo_rows(*[0 if t is None else t.data_ptr() for t in keep], baseline.data_ptr(),
                                             float(beta), float(gamma), n, sums.data_ptr(), dpg.data_ptr(),
                                             _hip.stream_ptr(dev)), "elbo_rows")
        ctx.save_for_backward(dpg)
        ctx.has_nmn = nmn_loss is not None
        return sums

    @staticmethod
    def backward(ctx, dsums):
        (dpg,) = ctx.saved_tensors
        # sums = [sum rec, sum kl, sum elbo, sum R, sum nmn, sum c]; with rec = -qr, kl = -pg c + beta pg, elbo = rec - kl:
        #   d/d pg[n] = -dsums[1] (c - beta) + dsums[2] (c - beta);  d/d qr[n] = -dsums[0] - dsums[2];  d/d nmn[n] = dsums[4]
        d_pg = (dsums[2] - dsums[1]) * dpg
        d_qr = -(dsums[0] + dsums[2]).expand_as(dpg)
        d_nmn = dsums[4].expand_as(dpg) if ctx.has_nmn else None
        return d_pg, d_qr, None, d_nmn, None, None, None


def _launch_joint_objective(rows, weights, baseline_ptr, alpha, beta, gamma, decay, flag, n, m, n_stats, dev):
    """The ONE call of ``pnmn_joint_objective``: the per-row losses ``rows`` = (pg, qr, prior, nmn, pg_sup) and the
    ``weights`` = (w_u, w_s) packed into one launch.  ``baseline_ptr`` and ``flag`` are the entry point's ``baseline`` /
    ``update_baseline``: a device scalar and 0 / 1 for the moving baseline, or no pointer (0) and the samples per question
    for the leave-one-out kernel, which reports ``n_stats`` = 11 statistics where the moving one reports 10.  Returns
    (out = the statistics followed by J, the per-row derivatives d_pg | d_qr | d_nmn | d_pg_sup in one tensor, their sizes)."""
    from probnmn import _hip

    keep = [None if t is None else t.detach().contiguous() for t in rows + weights]
    out = torch.zeros(n_stats + 1, dtype=torch.float32, device=dev)
    sizes = (n, n + m, n if rows[3] is not None else 0, m)
    grads = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    ptrs, at = [], 0
    for k in sizes:
        ptrs.append(grads.data_ptr() + 4 * at if k else 0)
        at += k
    p = [0 if t is None or t.numel() == 0 else t.data_ptr() for t in keep]  # (no rows: no pointer, like their derivatives)
    _hip.check(_hip.lib().pnmn_joint_objective(
        p[0], p[1], p[2], p[3], p[4], baseline_ptr, p[5], p[6], float(alpha), float(beta), float(gamma),
        float(decay), int(flag), n, m, out.data_ptr(), out.data_ptr() + 4 * n_stats, ptrs[0], ptrs[1], ptrs[2],
        ptrs[3], _hip.stream_ptr(dev)), "joint_objective")
    return out, grads, sizes


def _joint_objective_forward(ctx, rows, weights, baseline_ptr, alpha, beta, gamma, decay, flag, n, m, n_stats, dev):
    """What ``_Objective`` and ``_ObjectiveLoo`` share: the launch, the derivatives kept for backward; (J, detached stats)."""
    out, grads, sizes = _launch_joint_objective(rows, weights, baseline_ptr, alpha, beta, gamma, decay, flag, n, m, n_stats, dev)
    ctx.save_for_backward(grads)
    ctx.sizes = sizes
    ctx.present = (rows[0] is not None, rows[1] is not None, rows[3] is not None, rows[4] is not None)
    stats, objective = out[:n_stats], out[n_stats]
    ctx.mark_non_differentiable(stats)
    return objective, stats


def _joint_objective_backward(ctx, d_objective):
    """ONE multiply of the stored derivatives by the incoming dJ: the gradients of (pg, qr, prior, nmn, pg_sup)."""
    (grads,) = ctx.saved_tensors
    grads = grads * d_objective
    d_pg, d_qr, d_nmn, d_pgs = grads.split(ctx.sizes)
    has_pg, has_qr, has_nmn, has_pgs = ctx.present
    return (d_pg if has_pg else None, d_qr if has_qr else None, None, d_nmn if has_nmn else None, d_pgs if has_pgs else None)


class _Objective(torch.autograd.Function):
    """``pnmn_joint_objective``: the ELBO combination over the sampled rows, the supervised rows' mean cross entropies,
    the objective J = w_u (gamma mean(nmn) - mean(elbo)) + w_s alpha (mean(pg_sup) + mean(qr_sup)) and every per-row
    derivative in one launch; backward is ONE multiply of the stored derivatives by the incoming dJ.  Replaces the
    ~30 scalar torch ops (and their autograd nodes) between the models' per-row losses and ``backward()`` of a
    question-coding / joint-training iteration (reference question_coding_trainer.py:128-165,
    joint_training_trainer.py:150-191) -- at 128 questions per GPU that chain alone was 0.5 ms of host time."""

    @staticmethod
    def forward(ctx, pg, qr, prior, nmn, pg_sup, baseline, w_u, w_s, alpha, beta, gamma, decay, update_baseline, n, m):
        return _joint_objective_forward(ctx, (pg, qr, prior, nmn, pg_sup), (w_u, w_s), baseline.data_ptr(), alpha, beta, gamma,
                                        decay, update_baseline, n, m, 10, baseline.device)

    @staticmethod
    def backward(ctx, d_objective, _):
        return _joint_objective_backward(ctx, d_objective) + (None,) * 10


class _ObjectiveLoo(torch.autograd.Function):
    """``_Objective`` over n_questions x samples question-major sampled rows with the leave-one-out baseline: the same
    launch without a baseline tensor, the same backward.  stats[11]: the ten of ``_Objective`` and the reward variance."""

    @staticmethod
    def forward(ctx, pg, qr, prior, nmn, pg_sup, w_u, w_s, alpha, beta, gamma, n_questions, samples, m, dev):
        return _joint_objective_forward(ctx, (pg, qr, prior, nmn, pg_sup), (w_u, w_s), 0, alpha, beta, gamma, 0.0, samples,
                                        n_questions * samples, m, 11, dev)

    @staticmethod
    def backward(ctx, d_objective, _):
        return _joint_objective_backward(ctx, d_objective) + (None,) * 9


class _FusedElboLoo(torch.autograd.Function):
    """``combine`` under the leave-one-out baseline on the device: the same kernel with w_u = 1 and no supervised rows.  Its
    derivatives are those of J = gamma mean(nmn) - mean(elbo), so d mean(elbo) / d pg = -d_pg, d mean(elbo) / d qr = -d_qr
    (= -1 / N), d mean(nmn) / d nmn = 1 / N; the means of rec and kl get theirs from the same rows, as in ``_FusedElbo``."""

    @staticmethod
    def forward(ctx, pg_loss, qr_loss, prior_loss, nmn_loss, beta, gamma, samples):
        n = pg_loss.numel()
        if n % samples:
            raise ValueError("%d sampled rows are no whole number of groups of %d" % (n, samples))
        out, grads, ctx.sizes = _launch_joint_objective((pg_loss, qr_loss, prior_loss, nmn_loss, None), (None, None), 0, 0.0,
                                                        beta, gamma, 0.0, samples, n, 0, 11, pg_loss.device)
        ctx.save_for_backward(grads)
        ctx.has_nmn = nmn_loss is not None
        return out[:11]

    @staticmethod
    def backward(ctx, d):
        (grads,) = ctx.saved_tensors
        d_pg, d_qr, d_nmn, _ = grads.split(ctx.sizes)  # (by sizes: an empty batch still gives its pieces)
        # stats = [mean rec, mean kl, mean elbo, mean R, mean nmn, ...] with rec = -qr, kl = -pg c + beta pg, elbo = rec - kl
        g_pg = (d[1] - d[2]) * d_pg
        g_qr = -(d[0] + d[2]) * d_qr
        g_nmn = d[4] * d_qr if ctx.has_nmn else None
        return g_pg, g_qr, None, g_nmn, None, None, None


BASELINES = ("moving", "leave_one_out")


def check_estimator(num_samples, baseline: str) -> int:
    """The one rule for (samples per question, baseline), for the ELBO modules and the trainers alike: 1 .. 64 samples (what
    the kernel's groups hold; the same bound under either baseline), and another sample to take the leave-one-out baseline
    from.  Returns the sample count as an int; anything else is a ``ValueError``."""
    if baseline not in BASELINES:
        raise ValueError("baseline must be one of %s, got %r" % (BASELINES, baseline))
    if isinstance(num_samples, bool) or int(num_samples) != num_samples or not 1 <= num_samples <= 64:
        raise ValueError("num_samples must be an integer from 1 to 64, got %r" % (num_samples,))
    if baseline == "leave_one_out" and num_samples < 2:
        raise ValueError("the leave-one-out baseline centres a sample by the question's OTHER samples: num_samples must be "
                         "2 .. 64, got %d" % num_samples)
    return int(num_samples)


def leave_one_out_rows(logprobs_generation, logprobs_reconstruction, reinforce_reward, beta: float, samples: int):
    """The host statement of the multi-sample estimator with torch ops: per-row (kl, elbo, c) and the reward variance of
    question-major rows (row q * samples + k).  The reward is a constant of the estimator."""
    R = reinforce_reward.detach().reshape(-1, samples)
    S = R[:, 0].clone()
    for k in range(1, samples):  # (the kernel's order of additions)
        S = S + R[:, k]
    S = S.unsqueeze(1)
    centered = (R - (S - R) / (samples - 1)).reshape(-1)
    variance = ((R - S / samples) ** 2).sum(1) / (samples - 1)
    kl_divergence = logprobs_generation * centered - beta * logprobs_generation
    return kl_divergence, logprobs_reconstruction - kl_divergence, centered, variance.mean() if variance.numel() else variance.sum()


class _ElboWithReinforce(nn.Module):
    def __init__(self, beta: float = 0.1, baseline_decay: float = 0.99, num_samples: int = 1, baseline: str = "moving"):
        super().__init__()
        num_samples = check_estimator(num_samples, baseline)
        self._reinforce = Reinforce(baseline_decay=baseline_decay)
        self._beta = beta
        self._num_samples = int(num_samples)
        self._baseline_kind = baseline

    @property
    def leave_one_out(self) -> bool:
        return self._baseline_kind == "leave_one_out"

    def _forward_loo(self, inference_likelihood, reconstruction_likelihood, reinforce_reward) -> Dict[str, torch.Tensor]:
        """``_forward`` under the leave-one-out baseline (CPU tensors: the host statement); ``Reinforce`` is not involved."""
        if inference_likelihood.numel() % self._num_samples:
            raise ValueError("%d sampled rows are no whole number of groups of %d" % (inference_likelihood.numel(), self._num_samples))
        kl_divergence, elbo, _, variance = leave_one_out_rows(inference_likelihood, reconstruction_likelihood, reinforce_reward,
                                                              self._beta, self._num_samples)
        return {
            "reconstruction_likelihood": reconstruction_likelihood.mean(),
            "kl_divergence": kl_divergence.mean(),
            "elbo": elbo.mean(),
            "reinforce_reward": reinforce_reward.mean(),
            "reward_variance": variance,
        }

    def _fused_loo(self, generation_loss, reconstruction_loss, prior_loss, nmn_loss, gamma: float) -> Dict[str, torch.Tensor]:
        stats = _FusedElboLoo.apply(generation_loss, reconstruction_loss, prior_loss, nmn_loss, self._beta, gamma, self._num_samples)
        out = {"reconstruction_likelihood": stats[0], "kl_divergence": stats[1], "elbo": stats[2], "reinforce_reward": stats[3],
               "reward_variance": stats[10].detach()}
        if nmn_loss is not None:
            out["nmn_loss"] = stats[4]
        return out

    def _forward(self, inference_likelihood, reconstruction_likelihood, reinforce_reward) -> Dict[str, torch.Tensor]:
        kl_divergence = self._reinforce(inference_likelihood, reinforce_reward) - self._beta * inference_likelihood
        fully_monte_carlo_elbo = reconstruction_likelihood - kl_divergence
        return {
            "reconstruction_likelihood": reconstruction_likelihood.mean(),
            "kl_divergence": kl_divergence.mean(),
            "elbo": fully_monte_carlo_elbo.mean(),
            "reinforce_reward": reinforce_reward.mean(),
        }

    def objective(self, generation_loss, reconstruction_rows, prior_loss, nmn_loss, supervised_generation_loss,
                  w_unsup, w_sup, alpha: float, gamma: float, n: int, m: int):
        """The "ours" objective of an iteration from the models' per-row losses, on the device in one launch (see
        ``_Objective``).  ``reconstruction_rows``: the n sampled rows' reconstruction losses followed by the m supervised
        ones.  Returns (J, dict of the detached batch statistics the trainers report).  The REINFORCE baseline is
        updated here (in the kernel in a single process; from the all-reduced sum under data parallelism).

        Under the leave-one-out baseline the n sampled rows are n / num_samples question-major groups, the kernel is
        the leave-one-out one (``pnmn_joint_objective`` without a baseline pointer), the moving baseline is neither read nor written and no rank issues a collective; the
        statistics gain ``reward_variance``."""
        if self.leave_one_out:
            if n % self._num_samples:
                raise ValueError("%d sampled rows are no whole number of groups of %d" % (n, self._num_samples))
            w_u = w_unsup if isinstance(w_unsup, torch.Tensor) else None
            w_s = w_sup if isinstance(w_sup, torch.Tensor) else None
            J, stats = _ObjectiveLoo.apply(generation_loss, reconstruction_rows, prior_loss, nmn_loss, supervised_generation_loss,
                                           w_u, w_s, alpha, self._beta, gamma, n // self._num_samples, self._num_samples, m,
                                           reconstruction_rows.device)
            return J, {"reconstruction_likelihood": stats[0], "kl_divergence": stats[1], "elbo": stats[2], "reinforce_reward": stats[3],
                       "nmn_loss": stats[4], "program_generation_gt": stats[6], "question_reconstruction_gt": stats[7],
                       "reward_variance": stats[10]}
        r = self._reinforce
        dev = reconstruction_rows.device
        if r._baseline is None or r._baseline.device != dev:
            value = 0.0 if r._baseline is None else float(r._baseline)
            r._baseline = torch.full((), value, dtype=torch.float32, device=dev)
        single = parallel.world() == 1
        w_u = w_unsup if isinstance(w_unsup, torch.Tensor) else None
        w_s = w_sup if isinstance(w_sup, torch.Tensor) else None
        J, stats = _Objective.apply(generation_loss, reconstruction_rows, prior_loss, nmn_loss, supervised_generation_loss,
                                    r._baseline, w_u, w_s, alpha, self._beta, gamma, r._baseline_decay, single, n, m)
        if not single:
            with torch.no_grad():
                total = parallel.all_reduce_scalars(torch.stack((stats[5], stats[9])))
                r._baseline = r._baseline + r._baseline_decay * total[0] / total[1].clamp(min=1.0)
        out = {"reconstruction_likelihood": stats[0], "kl_divergence": stats[1], "elbo": stats[2], "reinforce_reward": stats[3],
               "nmn_loss": stats[4], "program_generation_gt": stats[6], "question_reconstruction_gt": stats[7]}
        return J, out

    def _fused(self, generation_loss, reconstruction_loss, prior_loss, nmn_loss, gamma: float) -> Dict[str, torch.Tensor]:
        """The "ours" objectives on the device in one launch (same arithmetic as ``combine`` -> ``_forward``
        -> ``Reinforce.forward``; the baseline update and its data-parallel all-reduce stay here)."""
        r = self._reinforce
        if r._baseline is None or r._baseline.device != generation_loss.device:
            value = 0.0 if r._baseline is None else float(r._baseline)
            r._baseline = torch.full((), value, dtype=torch.float32, device=generation_loss.device)
        n = generation_loss.numel()
        sums = _FusedElbo.apply(generation_loss, reconstruction_loss, prior_loss, nmn_loss, r._baseline, self._beta, gamma)
        with torch.no_grad():
            stats = torch.stack((sums[5], torch.full_like(sums[5], float(n))))
            stats = parallel.all_reduce_scalars(stats)
            r._baseline = r._baseline + r._baseline_decay * stats[0] / stats[1].clamp(min=1.0)
        means = sums / max(n, 1)
        out = {"reconstruction_likelihood": means[0], "kl_divergence": means[1], "elbo": means[2],
               "reinforce_reward": means[3]}
        if nmn_loss is not None:
            out["nmn_loss"] = means[4]
        return out


class QuestionCodingElbo(_ElboWithReinforce):
    def __init__(self, program_generator, question_reconstructor, program_prior, beta: float = 0.1,
                 baseline_decay: float = 0.99, num_samples: int = 1, baseline: str = "moving"):
        super().__init__(beta, baseline_decay, num_samples, baseline)
        self._program_generator = program_generator
        self._question_reconstructor = question_reconstructor
        self._program_prior = program_prior

    def forward(self, question_tokens: torch.LongTensor):
        if self._num_samples > 1:  # K programs per question, question-major (the decoders draw per row position)
            question_tokens = question_tokens.repeat_interleave(self._num_samples, 0)
        pg_out = self._program_generator(question_tokens, decoding_strategy="sampling")
        sampled_programs = pg_out["predictions"]
        with torch.no_grad():  # frozen model whose output only enters the detached reward
            prior_out = self._program_prior(sampled_programs)
        qr_out = self._question_reconstructor(sampled_programs, question_tokens, decoding_strategy="sampling")
        return self.combine(pg_out["loss"], qr_out["loss"], prior_out["loss"])

    def combine(self, generation_loss, reconstruction_loss, prior_loss) -> Dict[str, torch.Tensor]:
        """The objective from the three per-example negative log-likelihoods of the SAMPLED programs
        (reference elbo.py:130-161); trainers that batch the model passes themselves call this."""
        if generation_loss.is_cuda:
            fused = self._fused_loo if self.leave_one_out else self._fused
            return fused(generation_loss, reconstruction_loss, prior_loss, None, 0.0)
        logprobs_reconstruction = -reconstruction_loss
        logprobs_generation = -generation_loss
        logprobs_prior = -prior_loss
        reinforce_reward = logprobs_reconstruction + self._beta * (logprobs_prior - logprobs_generation)
        if self.leave_one_out:
            return self._forward_loo(logprobs_generation, logprobs_reconstruction, reinforce_reward)
        return super()._forward(logprobs_generation, logprobs_reconstruction, reinforce_reward)


class JointTrainingElbo(_ElboWithReinforce):
    def __init__(self, program_generator, question_reconstructor, program_prior, nmn, beta: float = 0.1,
                 gamma: float = 10, baseline_decay: float = 0.99, objective: str = "ours", num_samples: int = 1,
                 baseline: str = "moving"):
        super().__init__(beta, baseline_decay, num_samples, baseline)
        if objective == "baseline" and (num_samples > 1 or baseline != "moving"):
            raise ValueError("the reference's joint 'baseline' objective draws one program per question and centres it "
                             "with the moving baseline")
        self._program_generator = program_generator
        self._question_reconstructor = question_reconstructor
        self._program_prior = program_prior
        self._nmn = nmn
        self._gamma = gamma
        self._objective = objective

    def forward(self, question_tokens, image_features, answer_tokens):
        if self._num_samples > 1:
            # K programs per question, question-major; the images are replicated by index (a resident batch through its
            # row indices: no map is copied)
            K = self._num_samples
            replicas = torch.arange(question_tokens.size(0), device=question_tokens.device).repeat_interleave(K)
            question_tokens = question_tokens.repeat_interleave(K, 0)
            answer_tokens = answer_tokens.repeat_interleave(K, 0)
            if isinstance(image_features, torch.Tensor):
                image_features = image_features.index_select(0, replicas.to(image_features.device))  # (same device: no copy)
            else:
                image_features = image_features.subset(replicas)  # (host indices: what a resident batch is named by)
        pg_out = self._program_generator(question_tokens, decoding_strategy="sampling")
        sampled_programs = pg_out["predictions"]
        # (one stream: the recurrent kernels and the library GEMMs of these passes must not share the chip
        # with each other -- DESIGN.md 6; the batched joint step in probnmn.trainers overlaps the NMN trunk)
        qr_loss = self._question_reconstructor(sampled_programs, question_tokens, decoding_strategy="sampling")["loss"]
        prior_loss = None
        if self._objective != "baseline":
            with torch.no_grad():  # frozen model whose output only enters the detached reward
                prior_loss = self._program_prior(sampled_programs)["loss"]
        nmn_out = self._nmn(image_features, sampled_programs, answer_tokens)
        return self.combine(pg_out["loss"], qr_loss, prior_loss, nmn_out)

    def combine(self, generation_loss, reconstruction_loss, prior_loss, nmn_out) -> Dict[str, torch.Tensor]:
        """The objective from the per-example losses of the SAMPLED programs (reference
        elbo.py:220-280); trainers that batch the model passes themselves call this."""
        if self._objective == "baseline":
            reinforce_reward = -nmn_out["loss"]
            output_dict = {
                "elbo": self._reinforce(generation_loss, reinforce_reward).mean(),
                "reinforce_reward": reinforce_reward.mean(),
            }
        elif generation_loss.is_cuda:
            fused = self._fused_loo if self.leave_one_out else self._fused
            return fused(generation_loss, reconstruction_loss, prior_loss, nmn_out["loss"], self._gamma)
        else:
            logprobs_reconstruction = -reconstruction_loss
            logprobs_generation = -generation_loss
            logprobs_prior = -prior_loss
            logprobs_answering = -nmn_out["loss"]
            reinforce_reward = (logprobs_reconstruction + self._beta * logprobs_prior
                                - self._beta * logprobs_generation + self._gamma * logprobs_answering)
            forward = self._forward_loo if self.leave_one_out else super()._forward
            output_dict = forward(logprobs_generation, logprobs_reconstruction, reinforce_reward)
        output_dict["nmn_loss"] = nmn_out["loss"].mean()
        return output_dict
