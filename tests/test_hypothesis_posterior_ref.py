"""Posterior reranking without a device: the fp64 reference of ``pnmn_hypothesis_posterior`` (tests/helpers/
hypothesis_posterior_reference.py) against torch, the argument rules of ``rerank`` in ``predict_answers`` /
``evaluate_marginal_answer_accuracy`` and what the entry point answers before it would launch anything."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from hypothesis_posterior_reference import (hypothesis_posterior_reference, sequence_log_likelihood,  # noqa: E402
                                            top_two_score_margin)


def _dense(seed=3, G=7, K=5, Tx=6, Vx=11, Tz=4, Vz=9):
    rng = np.random.default_rng(seed)
    R = G * K
    x_logits, z_logits = rng.standard_normal((R, Tx, Vx)) * 3, rng.standard_normal((R, Tz, Vz)) * 3
    x_tokens, z_tokens = rng.integers(0, Vx, (R, Tx)), rng.integers(0, Vz, (R, Tz))  # (0 is the padding)
    log_q = rng.standard_normal(R) * 4 - 20
    return (x_logits, x_tokens, 0), (z_logits, z_tokens, 0), log_q, np.arange(G + 1) * K


def _torch_lp(logits, tokens, pad):
    logits, tokens = torch.from_numpy(logits), torch.from_numpy(tokens)
    lp = torch.log_softmax(logits, -1).gather(2, tokens.unsqueeze(-1)).squeeze(-1)
    return (lp * (tokens != pad)).sum(1)


def test_reference_equals_the_torch_composition_on_a_dense_case():
    """G groups of K rows: log_softmax, gather, mask, sum per term; the weighted sum; log_softmax / logsumexp / argmax over
    the hypotheses of a group."""
    x, z, log_q, start = _dense()
    G, K = len(start) - 1, int(start[1])
    weights = (1.0, 0.5, 0.25)
    ref = hypothesis_posterior_reference(x, z, log_q, start, weights)
    lp_x, lp_z = _torch_lp(*x), _torch_lp(*z)
    np.testing.assert_allclose(ref["log_px"], lp_x.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["log_pz"], lp_z.numpy(), rtol=1e-12, atol=1e-12)
    score = (weights[0] * lp_x + weights[1] * lp_z + weights[2] * torch.from_numpy(log_q)).view(G, K)
    np.testing.assert_allclose(ref["score"], score.reshape(-1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["log_posterior"], torch.log_softmax(score, 1).reshape(-1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["log_evidence"], torch.logsumexp(score, 1).numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(ref["best_row"], (score.argmax(1) + torch.arange(G) * K).numpy())
    assert ref["support"].tolist() == [K] * G and ref["usable"].all() and ref["covered"].all()
    np.testing.assert_allclose(np.exp(ref["log_posterior"]).reshape(G, K).sum(1), 1.0, rtol=1e-12)
    top = np.sort(score.numpy(), 1)
    np.testing.assert_allclose(top_two_score_margin(ref["score"], ref["usable"], start), top[:, -1] - top[:, -2], rtol=1e-12)
    np.testing.assert_allclose(ref["max_abs_score"], np.abs(score.numpy()).max(1), rtol=1e-12)
    # with n scored tokens, -lp / n is the per-token mean the sequence losses report
    n = (x[1] != 0).sum(1)
    mean = -(torch.log_softmax(torch.from_numpy(x[0]), -1).gather(2, torch.from_numpy(x[1]).unsqueeze(-1)).squeeze(-1)
             * torch.from_numpy(x[1] != 0)).sum(1) / torch.from_numpy(n)
    np.testing.assert_allclose(-ref["log_px"][n > 0] / n[n > 0], mean.numpy()[n > 0], rtol=1e-12)


def test_reference_rows_that_do_not_count():
    x, z, log_q, start = _dense(seed=5)
    x[1][0] = 0                      # row 0: all padding -> lp_x = 0, still usable
    x[1][1, 2] = 11                  # row 1: a token beyond the vocabulary
    x[1][2, 0] = -3                  # row 2: a negative token
    z[1][3, 1] = 4                   # row 3: -inf at a scored target
    z[0][3, 1, 4] = -np.inf
    log_q[4] = -np.inf               # row 4: the generator rules it out
    ref = hypothesis_posterior_reference(x, z, log_q, start, (1.0, 1.0, 1.0))
    assert ref["log_px"][0] == 0.0 and ref["usable"][0]
    assert np.isneginf(ref["log_px"][[1, 2]]).all() and np.isneginf(ref["log_pz"][3])
    assert not ref["usable"][:5][1:].any() and ref["support"][0] == 1 and ref["best_row"][0] == 0
    assert ref["log_posterior"][0] == 0.0 and np.isneginf(ref["log_posterior"][1:5]).all()
    assert ref["log_evidence"][0] == ref["score"][0]
    assert np.isinf(top_two_score_margin(ref["score"], ref["usable"], start)[0])
    assert sequence_log_likelihood(np.zeros((2, 3, 1)), np.zeros((2, 3), np.int64), 7).tolist() == [0.0, 0.0]  # one token: log 1


def test_reference_clamps_group_bounds():
    x, z, log_q, _ = _dense(G=2, K=3)
    ref = hypothesis_posterior_reference(x, z, log_q, [-4, 2, 1, 9], (1.0, 1.0, 0.0))  # rows [0, 2), nothing, [1, 6)
    assert ref["support"].tolist() == [2, 0, 5] and ref["covered"].all()
    assert ref["best_row"][1] == -1 and np.isneginf(ref["log_evidence"][1])
    assert 0 <= ref["best_row"][0] < 2 and 1 <= ref["best_row"][2] < 6
    ref = hypothesis_posterior_reference(x, z, log_q, [3, 3, 5], (1.0, 1.0, 0.0))
    assert ref["covered"].tolist() == [False, False, False, True, True, False] and np.isneginf(ref["log_posterior"][~ref["covered"]]).all()


def test_reference_a_zero_coefficient_drops_its_term():
    x, z, log_q, start = _dense(seed=7)
    x[1][3, 1] = 99                  # unusable by index in the x term ...
    log_q[6] = -np.inf               # ... and ruled out by the generator
    full = hypothesis_posterior_reference(x, z, log_q, start, (1.0, 1.0, 1.0))
    assert not full["usable"][3] and not full["usable"][6]
    for weights, null, back in (((0.0, 1.0, 1.0), (None, z, log_q), 3), ((1.0, 1.0, 0.0), (x, z, None), 6)):
        zero = hypothesis_posterior_reference(x, z, log_q, start, weights)
        gone = hypothesis_posterior_reference(*null, start, weights, n_rows=len(log_q))
        assert zero["usable"][back] and np.isfinite(zero["score"]).sum() == np.isfinite(full["score"]).sum() + 1
        for name in ("score", "log_posterior", "log_evidence", "best_row", "support"):
            assert np.array_equal(zero[name], gone[name]), name          # no 0 * -inf: the term is simply not there
    only_q = hypothesis_posterior_reference(x, z, log_q, start, (0.0, 0.0, 1.0))
    lq = torch.from_numpy(log_q).view(len(start) - 1, -1)
    np.testing.assert_allclose(only_q["log_posterior"], torch.log_softmax(lq, 1).reshape(-1).numpy(), rtol=1e-12, atol=1e-12)
    assert np.isneginf(only_q["log_px"][3])  # (the term is still reported)


def test_reference_a_group_without_a_usable_row():
    x, z, log_q, start = _dense(seed=9)
    log_q[start[2]:start[3]] = -np.inf
    x[1][start[4]:start[5], 0] = -1
    ref = hypothesis_posterior_reference(x, z, log_q, start, (1.0, 1.0, 1.0))
    for g in (2, 4):
        assert ref["support"][g] == 0 and ref["best_row"][g] == -1 and np.isneginf(ref["log_evidence"][g])
        assert np.isneginf(ref["log_posterior"][start[g]:start[g + 1]]).all() and ref["max_abs_score"][g] == 0.0
    assert (ref["support"][[0, 1, 3, 5, 6]] == 5).all()
    empty = hypothesis_posterior_reference(x, z, log_q, [0, 0, 0], (1.0, 1.0, 1.0))
    assert empty["support"].tolist() == [0, 0] and empty["best_row"].tolist() == [-1, -1] and not empty["covered"].any()


@pytest.mark.parametrize("options", [
    dict(rerank=True),                                                              # no hypotheses to rerank
    dict(rerank=True, marginal=True),
    dict(rerank=True, beam_size=4),                                                 # default coefficients, no models
    dict(rerank=True, num_programs=4, question_reconstructor=object()),             # w_z = 1 without the prior
    dict(rerank=True, beam_size=4, program_prior=object()),                         # w_x = 1 without the reconstructor
    dict(rerank=True, beam_size=4, rerank_weights=(0.0, 0.5, 1.0)),
    dict(rerank=True, beam_size=4, rerank_weights=(0.5, 0.0, 1.0)),
    dict(rerank=True, beam_size=4, explain=True, question_reconstructor=object(), program_prior=object()),
    dict(rerank=True, num_programs=4, explain=True, rerank_weights=(0.0, 0.0, 1.0)),
    dict(rerank=True, num_programs=4, beam_size=4, rerank_weights=(0.0, 0.0, 1.0)),  # samples and a search
    dict(rerank=True, num_programs=1, rerank_weights=(0.0, 0.0, 1.0)),
    dict(rerank=True, beam_size=4, rerank_weights=(0.0, 0.0)),
    dict(rerank=True, beam_size=4, rerank_weights=(0.0, 0.0, float("nan"))),
    dict(rerank=True, beam_size=4, rerank_weights=(0.0, float("inf"), 1.0)),
    dict(rerank=True, beam_size=4, rerank_weights="110"[:2]),
    dict(rerank=True, beam_size=4, rerank_weights=None),
])
def test_rerank_is_refused_before_a_model_is_touched(options):
    from probnmn.evaluators import evaluate_marginal_answer_accuracy, predict_answers

    with pytest.raises(ValueError):
        predict_answers(None, None, [], None, **options)
    if "marginal" not in options and "explain" not in options:  # (the accuracy loop has neither keyword)
        with pytest.raises(ValueError):
            evaluate_marginal_answer_accuracy(None, None, [], None, **options)


def test_hypothesis_posterior_checks_its_arguments_before_a_model_is_touched():
    from probnmn.evaluators import hypothesis_posterior

    q, p, rows = torch.zeros(2, 3, dtype=torch.long), torch.zeros(4, 5, dtype=torch.long), np.array([0, 0, 1, 1])
    for kwargs in (dict(), dict(weights=(1.0, 0.0, 0.0)), dict(weights=(0.0, 1.0, 0.0)), dict(weights=(0.0, 0.0, 1.0)),
                   dict(weights=(0.0, 0.0, 0.0)), dict(weights=(0.0, 0.0, float("nan")), log_q=np.zeros(4)),
                   dict(weights=(0.0, 0.0, 1.0), log_q=np.zeros(4), max_rows=0)):
        with pytest.raises(ValueError):
            hypothesis_posterior(None, None, q, p, rows, **kwargs)


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device():
    from probnmn import _hip

    assert len(_hip.SIGNATURES["pnmn_hypothesis_posterior"]) == 26
    fn = _hip.lib().pnmn_hypothesis_posterior
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)

    def call(x_logits=p, x_tokens=p, z_logits=p, z_tokens=p, log_q=p, group_start=p, w=(1.0, 1.0, 0.0), log_posterior=p,
             log_evidence=p, best_row=p, n_groups=1, n_rows=2, Tx=3, Vx=4, Tz=3, Vz=4):
        return fn(x_logits, x_tokens, Tx, z_logits, z_tokens, Tz, log_q, group_start, *w, 0, 0, 0, 0, log_posterior,
                  log_evidence, best_row, 0, n_groups, n_rows, Tx, Vx, Tz, Vz, 0)

    for missing in ("group_start", "log_posterior", "log_evidence", "best_row", "x_tokens", "z_tokens"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(x_logits=0, z_logits=0, log_q=0) == _hip.EINVAL           # nothing to score with
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL
    for name in ("Tx", "Vx", "Tz", "Vz"):
        assert call(**{name: 0}) == _hip.EINVAL and call(**{name: -2}) == _hip.EINVAL, name
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            w = [1.0, 1.0, 1.0]
            w[k] = bad
            assert call(w=w) == _hip.EINVAL, (bad, k)
    assert call(Vx=1025) == _hip.ESHAPE and call(Vz=1025) == _hip.ESHAPE
    # the sizes of a term that is not given do not matter ...
    assert call(x_logits=0, x_tokens=0, Tx=0, Vx=0, Vz=1025) == _hip.ESHAPE
    assert call(z_logits=0, z_tokens=0, Tz=-1, Vz=4000, n_groups=-1) == _hip.EINVAL
    # ... and without a group there is nothing to do, whatever else is given
    assert call(n_groups=0) == 0 and call(n_groups=0, n_rows=0, x_logits=0, z_logits=0, log_q=0, group_start=0) == 0
