"""Joint marginal-likelihood training without a device: the fp64 reference of ``pnmn_hypothesis_posterior``'s gradient mode
(tests/helpers/sequence_marginal_reference.py) against torch's fp64 autograd of the loss written out, what the entry point
answers in gradient mode before it would launch anything, and the option rules of ``MarginalJointStep``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from sequence_marginal_cases import HOST_CASES, SEEDS, WEIGHTS, ragged_inputs, requirements, satisfies  # noqa: E402
from sequence_marginal_reference import sequence_marginal_reference  # noqa: E402


def _autograd(x, z, log_q, start, weights, usable):
    """(loss fp64 [G] -- NaN without support --, d sum(loss) / d x logits, d z logits, d log_q) of
    loss[g] = -logsumexp over the usable rows of g of (w_x lp_x + w_z lp_z + w_q log_q), lp = the sum over the steps that are
    not padding of log_softmax(logits)[token]; a term whose coefficient is 0 is left out."""
    w_x, w_z, w_q = weights
    leaves, score = [], torch.zeros(len(log_q), dtype=torch.float64)
    for (logits, tokens, pad), w in ((x, w_x), (z, w_z)):
        leaf = torch.from_numpy(np.asarray(logits, np.float64)).requires_grad_(True)
        leaves.append(leaf)
        if w == 0.0:
            continue
        V = logits.shape[2]
        tok = torch.from_numpy(tokens)
        scored = (tok != pad) & (tok >= 0) & (tok < V)  # (a usable row has no other token that is not padding)
        lp = torch.log_softmax(leaf, -1).gather(2, tok.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
        score = score + w * torch.where(scored, lp, torch.zeros_like(lp)).sum(1)
    q = torch.from_numpy(np.asarray(log_q, np.float64)).requires_grad_(True)
    if w_q != 0.0:
        score = score + w_q * q
    losses, total = np.full(len(start) - 1, np.nan), None
    for g in range(len(start) - 1):
        rows = np.arange(start[g], start[g + 1])
        use = torch.from_numpy(rows[usable[rows]])
        if not len(use):
            continue
        loss = -torch.logsumexp(score[use], 0)
        losses[g] = float(loss.detach())
        total = loss if total is None else total + loss
    total.backward()
    grads = [leaf.grad.numpy() if leaf.grad is not None else np.zeros(leaf.shape) for leaf in leaves]
    return losses, grads[0], grads[1], q.grad.numpy() if q.grad is not None else np.zeros(len(log_q))


@pytest.mark.parametrize("case", HOST_CASES)
def test_reference_gradient_against_fp64_autograd(case):
    Vx, Vz, Tx = case
    x, z, log_q, start = ragged_inputs(Vx, Vz, SEEDS[case], Tx=Tx)
    assert len(start) - 1 == 37
    requirements(x, z, log_q, start)
    for weights in WEIGHTS:
        ref = sequence_marginal_reference(x, z, log_q, start, weights)
        assert satisfies(ref) and ref["covered"].all()
        usable, supported = ref["usable"], ref["support"] > 0
        losses, g_x, g_z, g_q = _autograd(x, z, log_q, start, weights, usable)
        worst = max(np.abs(ref["d_x_logits"] - g_x).max(), np.abs(ref["d_z_logits"] - g_z).max(), np.abs(ref["d_log_q"] - g_q).max())
        print("V = %s, weights %s: %d supported groups, %d usable rows, largest |gradient - autograd| %.3g"
              % ((Vx, Vz), weights, int(supported.sum()), int(usable.sum()), worst))
        assert worst <= 1e-12
        np.testing.assert_allclose(-ref["log_evidence"][supported], losses[supported], rtol=0, atol=1e-12)
        # what the device test holds exactly: rows that do not count and padding steps are zeros; the target's column pulls
        # down, the others up; a scored step of a usable row sums to 0
        for (logits, tokens, pad), d, w in ((x, ref["d_x_logits"], weights[0]), (z, ref["d_z_logits"], weights[1])):
            assert not np.isnan(d).any() and (d[~usable] == 0).all() and (d[tokens == pad] == 0).all()
            if w == 0.0:
                assert (d == 0).all()
                continue
            scored = usable[:, None] & (tokens != pad)
            target = np.zeros(d.shape, bool)
            r, t = np.nonzero(scored)
            target[r, t, tokens[r, t]] = True
            assert (d[target] <= 0).all() and (d[scored][~target[scored]] >= 0).all() and (d[scored] != 0).any()
            assert np.abs(d[scored].sum(-1)).max() <= 1e-12
            assert (d[np.isneginf(logits)] == 0).all()
        assert (ref["d_log_q"] <= 0).all() and (ref["d_log_q"][~usable] == 0).all()
        for g in np.nonzero(supported)[0]:  # the shares of a supported group sum to 1
            assert abs(ref["d_log_q"][start[g]:start[g + 1]].sum() + weights[2]) <= 1e-12


def test_gradient_mode_checks_its_arguments_without_a_device():
    from probnmn import _hip

    assert _hip.ABI_VERSION == 14 and len(_hip.SIGNATURES) == 103 and len(_hip.SIGNATURES["pnmn_hypothesis_posterior"]) == 26
    fn = _hip.lib().pnmn_hypothesis_posterior
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)

    def call(x_logits=p, x_tokens=p, z_logits=p, z_tokens=p, log_q=p, group_start=p, w=(1.0, 1.0, 0.0), d_x=p, d_z=0,
             log_posterior=p, log_evidence=p, n_groups=1, n_rows=2, Tx=3, Vx=4, Tz=3, Vz=4):
        # gradient mode: no best_row, and d_x_logits / d_z_logits in log_px's / log_pz's place
        return fn(x_logits, x_tokens, Tx, z_logits, z_tokens, Tz, log_q, group_start, *w, 0, 0, d_x, d_z, log_posterior,
                  log_evidence, 0, 0, n_groups, n_rows, Tx, Vx, Tz, Vz, 0)

    # the call that was refused with EINVAL until this mode existed now gets as far as the shape
    assert call(Vx=1025) == _hip.ESHAPE
    assert call(d_x=0, d_z=p, Vz=1025) == _hip.ESHAPE and call(d_z=p, Vx=1025) == _hip.ESHAPE
    assert call(d_x=0, d_z=0) == _hip.EINVAL and call(d_x=0, d_z=0, Vx=1025) == _hip.EINVAL  # (neither best_row nor a slot)
    # a slot needs its logits
    assert call(x_logits=0) == _hip.EINVAL and call(x_logits=0, x_tokens=0) == _hip.EINVAL
    assert call(d_x=0, d_z=p, z_logits=0) == _hip.EINVAL and call(d_z=p, z_logits=0, z_tokens=0) == _hip.EINVAL
    for missing in ("log_posterior", "log_evidence", "group_start", "x_tokens", "z_tokens"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL
    for name in ("Tx", "Vx", "Tz", "Vz"):
        assert call(**{name: 0}) == _hip.EINVAL, name
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            w = [1.0, 1.0, 1.0]
            w[k] = bad
            assert call(w=w) == _hip.EINVAL, (bad, k)
            assert call(w=w, Vx=1025) == _hip.EINVAL  # (the pointers and the coefficients, then the shape)
    # without a group there is nothing to do, whatever else is given
    assert call(n_groups=0) == 0
    assert call(n_groups=0, n_rows=0, x_logits=0, z_logits=0, log_q=0, group_start=0, log_posterior=0, log_evidence=0, Vx=4000) == 0
    assert call(n_groups=0, w=(float("nan"), 1.0, 1.0)) == 0


def test_sequence_marginal_loss_checks_its_arguments_before_a_launch():
    from probnmn.modules.marginal_likelihood import sequence_marginal_loss

    start = torch.zeros(3, dtype=torch.int32)
    logits, tokens = torch.zeros(4, 5, 6), torch.zeros(4, 5, dtype=torch.long)
    for kwargs in (dict(), dict(x=(logits, tokens, 0), weights=(1.0, 0.0)), dict(x=(logits, tokens, 0), weights=(1.0, 0.0, float("nan"))),
                   dict(x=(logits, tokens, 0), weights=None), dict(x=(logits.double(), tokens, 0)), dict(x=(logits, tokens.int(), 0)),
                   dict(x=(logits, tokens[:, :4], 0)), dict(x=(logits, tokens, 0), log_q=torch.zeros(3)),
                   dict(x=(logits, tokens, 0), z=(logits[:3], tokens[:3], 0)), dict(log_q=torch.zeros(4, 1))):
        with pytest.raises(ValueError):
            sequence_marginal_loss(group_start=start, **kwargs)
    with pytest.raises(ValueError):
        sequence_marginal_loss(x=(logits, tokens, 0), group_start=start.long())


def test_trainer_option_rules():
    from probnmn import trainers
    from probnmn.trainers.marginal_training import MarginalJointStep, marginal_joint_options

    assert trainers.MarginalJointStep is MarginalJointStep

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the options are checked before any model is touched (%s)" % name)

    pg, nmn = Untouchable(), Untouchable()
    bad = [dict(beam_size=0), dict(beam_size=3), dict(beam_size=32), dict(beam_size=True), dict(beam_size=4.0), dict(beam_size=None),
           dict(answer_weight=float("nan")), dict(answer_weight=float("inf")), dict(answer_weight=None), dict(answer_weight="heavy"),
           dict(constrained=1), dict(constrained=None), dict(without_replacement="probability"), dict(without_replacement=0),
           dict(train_modules=None), dict(train_modules=1)]
    for options in bad:
        with pytest.raises(ValueError):
            MarginalJointStep(pg, nmn, **options)
    with pytest.raises(TypeError):
        MarginalJointStep(pg, nmn, num_programs=4)  # (not offered: merged samples are weighted by counts, which is not q)
    for beam_size in (1, 2, 4, 8, 16):
        assert marginal_joint_options(beam_size, True, False, 1.0, True) == 1.0
    assert marginal_joint_options(4, False, True, 0.5, False) == 0.5 and marginal_joint_options(4, False, False, 0, True) == 0.0
