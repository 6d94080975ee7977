"""Marginal-likelihood module training without a device: the fp64 reference of ``pnmn_answer_posterior``'s gradient mode
(tests/helpers/marginal_loss_reference.py) against torch's fp64 autograd of the loss written out, what the entry point
answers in gradient mode before it would launch anything, and the option rules of ``ModuleTrainingStep(objective=...)``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from answer_posterior_cases import ANSWERS, SEEDS, ragged_inputs  # noqa: E402
from marginal_loss_reference import marginal_loss_reference  # noqa: E402


def _autograd(logits, valid, log_weight, answers, start, w_a, usable):
    """(loss fp64 [G] -- NaN without support --, d sum(loss) / d logits fp64 [R, A]) of
    loss[g] = -(logsumexp over usable rows of (lw + w_a log_softmax[a]) - logsumexp over base-usable rows of lw)."""
    z = torch.from_numpy(np.asarray(logits, np.float64)).requires_grad_(True)
    lw = torch.zeros(len(logits), dtype=torch.float64) if log_weight is None else torch.from_numpy(np.asarray(log_weight, np.float64))
    base = (np.asarray(valid) != 0) & np.isfinite(lw.numpy())
    log_softmax = torch.log_softmax(z, 1)
    losses, total = np.full(len(start) - 1, np.nan), None
    for g in range(len(start) - 1):
        rows = np.arange(start[g], start[g + 1])
        use = torch.from_numpy(rows[usable[rows]])
        if not len(use):
            continue
        base_rows = torch.from_numpy(rows[base[rows]])
        loss = -(torch.logsumexp(lw[use] + w_a * log_softmax[use, int(answers[g])], 0) - torch.logsumexp(lw[base_rows], 0))
        losses[g] = float(loss.detach())
        total = loss if total is None else total + loss
    total.backward()
    return losses, z.grad.numpy()


@pytest.mark.parametrize("A", ANSWERS)
def test_reference_gradient_against_fp64_autograd(A):
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    for w_a in (1.0, 0.5):
        ref = marginal_loss_reference(logits, valid, log_weight, answers, start, w_a, A)
        supported = ref["support"] > 0
        assert supported.sum() >= 28 and ref["covered"].all() and not np.isnan(ref["d_logits"]).any()
        losses, grad = _autograd(logits, valid, log_weight, answers, start, w_a, ref["usable"])
        worst = np.abs(ref["d_logits"] - grad).max()
        print("A = %d, w_a %s: %d supported groups, largest |d_logits - autograd| %.3g" % (A, w_a, int(supported.sum()), worst))
        assert worst <= 1e-12
        np.testing.assert_allclose(-ref["log_evidence"][supported], losses[supported], rtol=0, atol=1e-12)
        # what the device test holds exactly: rows that do not count are zeros; the answer's column pulls down, the others up
        assert (ref["d_logits"][~ref["usable"]] == 0).all() and ref["usable"].sum() > 100
        for g in np.nonzero(supported)[0]:
            rows = np.arange(start[g], start[g + 1])
            rows = rows[ref["usable"][rows]]
            others = np.delete(ref["d_logits"][rows], int(answers[g]), axis=1)
            assert (ref["d_logits"][rows, int(answers[g])] <= 0).all() and (others >= 0).all()
            assert np.abs(ref["d_logits"][rows].sum(1)).max() <= 1e-12
    zero = marginal_loss_reference(logits, valid, log_weight, answers, start, 0.0, A)
    assert (zero["d_logits"] == 0).all() and (zero["support"] > 0).sum() >= 28


def test_gradient_mode_checks_its_arguments_without_a_device():
    from probnmn import _hip

    assert _hip.ABI_VERSION == 14 and len(_hip.SIGNATURES) == 103 and len(_hip.SIGNATURES["pnmn_answer_posterior"]) == 19
    fn = _hip.lib().pnmn_answer_posterior
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)

    def call(logits=p, answers=p, group_start=p, w_a=1.0, d_logits=p, log_posterior=p, log_evidence=p, n_groups=1, n_rows=2, A=4):
        # gradient mode: no best_row, and d_logits in log_answer's place
        return fn(logits, 0, 0, answers, group_start, w_a, d_logits, 0, log_posterior, log_evidence, 0, 0, 0, 0, n_groups, n_rows, A, 0, 0)

    for missing in ("log_posterior", "log_evidence", "answers", "group_start", "logits"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(d_logits=0) == _hip.EINVAL  # (neither best_row nor d_logits: the call that was always refused)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(w_a=bad) == _hip.EINVAL, bad
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL and call(A=0) == _hip.EINVAL
    assert call(A=1025) == _hip.ESHAPE and call(A=1025, w_a=float("nan")) == _hip.EINVAL  # (the pointers and w_a, then the shape)
    assert call(n_groups=0) == 0 and call(n_groups=0, logits=0, answers=0, group_start=0, log_posterior=0, log_evidence=0) == 0


def test_trainer_option_rules():
    from probnmn.trainers.module_training import ModuleTrainingStep, module_objective_options

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the options are checked before any model is touched (%s)" % name)

    nmn, pg = Untouchable(), Untouchable()
    bad = [dict(objective="marginal", beam_size=4, program_generator=None),             # no generator
           dict(objective="marginal", beam_size=4, num_programs=4),                      # both
           dict(objective="marginal"),                                                   # neither
           dict(objective="marginal", beam_size=0), dict(objective="marginal", beam_size=32), dict(objective="marginal", beam_size=3),
           dict(objective="marginal", beam_size=True), dict(objective="marginal", beam_size=4.0),
           dict(objective="marginal", num_programs=1), dict(objective="marginal", num_programs=65),
           dict(objective="marginal", num_programs=True), dict(objective="marginal", num_programs=8.0),
           dict(objective="marginal", num_programs=4, constrained=True),                 # (constrained constrains the beam search)
           dict(objective="marginal", beam_size=4, answer_weight=float("nan")), dict(objective="marginal", beam_size=4, answer_weight=None),
           dict(objective="mml", beam_size=4), dict(objective=None),                     # unknown objectives
           dict(beam_size=4), dict(num_programs=4), dict(constrained=True), dict(answer_weight=0.5)]  # options of the other objective
    for options in bad:
        kwargs = dict(program_generator=pg)
        kwargs.update(options)
        with pytest.raises(ValueError):
            ModuleTrainingStep(nmn, **kwargs)
    for beam_size in (1, 2, 4, 8, 16):
        assert module_objective_options("marginal", True, beam_size, None, True, 1.0) == 1.0
    for num_programs in (2, 4, 64):
        assert module_objective_options("marginal", True, None, num_programs, False, 0.5) == 0.5
    assert module_objective_options("sampled", False, None, None, False, 1.0) == 1.0
