"""Marginal answering without a device: the fp64 reference of ``pnmn_answer_marginal`` (tests/helpers/
answer_marginal_reference.py) against torch, ``group_hypotheses``, the argument rules of ``predict_answers`` and what the
entry point answers before it would launch anything."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from answer_marginal_reference import answer_marginal_reference, top_two_margin  # noqa: E402


def test_reference_equals_the_torch_composition_on_a_dense_case():
    """G groups of K rows each: log_softmax over the answers, the normalised log-weights added, logsumexp over the
    hypotheses -- with invalid rows and rows of weight -inf masked out."""
    rng = np.random.default_rng(3)
    G, K, A, unknown = 9, 5, 28, 28
    logits = rng.standard_normal((G * K, A)) * 3
    valid = (rng.random(G * K) < 0.7).astype(np.int32)
    log_weight = rng.standard_normal(G * K) * 4 - 20
    log_weight[rng.random(G * K) < 0.1] = -np.inf
    valid[2 * K:3 * K] = 0  # a whole group invalid
    ref = answer_marginal_reference(logits, valid, log_weight, np.arange(G + 1) * K, unknown)

    lw = torch.from_numpy(log_weight).view(G, K).masked_fill(torch.from_numpy(valid).view(G, K) == 0, -float("inf"))
    log_w = lw - torch.logsumexp(lw, 1, keepdim=True)
    want = torch.logsumexp(log_w[:, :, None] + torch.log_softmax(torch.from_numpy(logits).view(G, K, A), -1), 1).numpy()
    supported = np.isfinite(lw.numpy()).any(1)
    assert not supported[2] and supported.sum() >= G // 2 and np.array_equal(ref["support"] > 0, supported)
    assert np.array_equal(ref["support"], np.isfinite(lw.numpy()).sum(1))
    np.testing.assert_allclose(ref["log_marginal"][supported], want[supported], rtol=1e-12, atol=1e-12)
    assert np.isneginf(ref["log_marginal"][~supported]).all() and (ref["predictions"][~supported] == unknown).all()
    assert np.array_equal(ref["predictions"][supported], want[supported].argmax(1))
    np.testing.assert_allclose(ref["row_weight"], torch.nan_to_num(log_w.exp(), nan=0.0).reshape(-1).numpy(), rtol=1e-12, atol=0)
    assert np.array_equal(ref["row_predictions"], np.where(valid != 0, logits.argmax(1), unknown))
    np.testing.assert_allclose(np.exp(ref["log_marginal"][supported]).sum(1), 1.0, rtol=1e-12)
    assert top_two_margin(ref["log_marginal"], ref["support"]) > 0
    # uniform weights are what a null log_weight means
    a = answer_marginal_reference(logits, valid, None, np.arange(G + 1) * K, unknown)
    b = answer_marginal_reference(logits, valid, np.full(G * K, -3.5), np.arange(G + 1) * K, unknown)
    np.testing.assert_allclose(a["log_marginal"], b["log_marginal"], rtol=1e-12, atol=1e-12)


def test_reference_clamps_group_bounds():
    logits = np.random.default_rng(0).standard_normal((6, 3))
    ref = answer_marginal_reference(logits, None, None, [-4, 2, 1, 9], 3)  # rows [0, 2), nothing, [1, 6)
    assert ref["support"].tolist() == [2, 0, 5] and ref["covered"].all()
    assert ref["predictions"][1] == 3 and np.isneginf(ref["log_marginal"][1]).all()


def test_group_hypotheses_merges_duplicates_in_first_occurrence_order():
    from probnmn.evaluators import group_hypotheses

    tokens = np.array([[[5, 6, 0], [7, 0, 0], [5, 6, 0], [8, 9, 0]],     # slots 0 and 2 are the same program
                       [[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]],     # nothing valid
                       [[4, 4, 0], [3, 0, 0], [3, 0, 0], [4, 4, 0]]])
    valid = np.array([[1, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]])
    programs, rows, weights, first = group_hypotheses(tokens, None, valid)
    assert programs.tolist() == [[5, 6, 0], [7, 0, 0], [4, 4, 0], [3, 0, 0]] and programs.dtype == np.int64
    assert rows.tolist() == [0, 0, 2, 2] and first.tolist() == [0, 1, 0, 1]  # question 1 has an empty group
    np.testing.assert_allclose(weights, np.log([2, 1, 2, 2]), rtol=1e-15)
    assert (np.diff(rows) >= 0).all()

    lw = np.array([[-1.0, -np.inf, -3.0, -0.5], [0.0, 0.0, 0.0, 0.0], [-2.0, np.nan, -4.0, -2.0]])
    programs, rows, weights, first = group_hypotheses(tokens, lw, np.ones((3, 4), np.int32))
    # question 0: slot 1 has weight -inf and goes; slot 3 is valid here.  question 2: the NaN goes, so program [3] first appears in slot 2
    assert programs.tolist() == [[5, 6, 0], [8, 9, 0], [1, 0, 0], [4, 4, 0], [3, 0, 0]]
    assert rows.tolist() == [0, 0, 1, 2, 2] and first.tolist() == [0, 3, 0, 0, 2]
    np.testing.assert_allclose(weights, [np.logaddexp(-1.0, -3.0), -0.5, np.log(4.0), -2.0 + np.log(2.0), -4.0], rtol=1e-15)


def test_group_hypotheses_with_one_slot_and_with_nothing():
    from probnmn.evaluators import group_hypotheses

    tokens = np.array([[[2, 3]], [[4, 0]], [[5, 5]]])
    programs, rows, weights, first = group_hypotheses(tokens, np.array([[-0.25], [-1.0], [-np.inf]]), np.array([[1], [0], [1]]))
    assert programs.tolist() == [[2, 3]] and rows.tolist() == [0] and weights.tolist() == [-0.25] and first.tolist() == [0]
    programs, rows, weights, first = group_hypotheses(tokens, None, np.zeros((3, 1)))
    assert programs.shape == (0, 2) and rows.shape == weights.shape == first.shape == (0,)
    with pytest.raises(ValueError):
        group_hypotheses(tokens[0], None, np.ones((1, 2)))


@pytest.mark.parametrize("options", [
    dict(marginal=True),                                  # marginal without a beam
    dict(num_programs=4, beam_size=4),                    # samples and a search
    dict(num_programs=4, beam_size=4, marginal=True),
    dict(marginal=True, beam_size=4, explain=True),
    dict(num_programs=4, explain=True),
    dict(num_programs=1), dict(num_programs=65), dict(num_programs=0), dict(num_programs=-3),
    dict(num_programs=4.0), dict(num_programs="4"), dict(num_programs=True),
])
def test_predict_answers_refuses_before_it_touches_a_model(options):
    from probnmn.evaluators import predict_answers

    with pytest.raises(ValueError):
        predict_answers(None, None, [], None, **options)


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device():
    from probnmn import _hip

    assert len(_hip.SIGNATURES["pnmn_answer_marginal"]) == 14
    fn = _hip.lib().pnmn_answer_marginal
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)

    def call(logits=p, group_start=p, log_marginal=p, predictions=p, n_groups=1, n_rows=2, num_answers=4):
        return fn(logits, 0, 0, group_start, log_marginal, predictions, 0, 0, 0, n_groups, n_rows, num_answers, 4, 0)

    for missing in ("logits", "group_start", "log_marginal", "predictions"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(num_answers=0) == _hip.EINVAL and call(num_answers=-1) == _hip.EINVAL
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL
    assert call(n_groups=0) == 0 and call(n_groups=0, n_rows=0, logits=0) == 0
    assert call(num_answers=1025) == _hip.ESHAPE
