"""Program inference from question and answer without a device: the fp64 reference of ``pnmn_answer_posterior``
(tests/helpers/answer_posterior_reference.py) against a per-row ``log_softmax`` and against the reference of
``pnmn_answer_marginal``, the conditions the device test's seeds were chosen for, the argument rules of ``infer_programs`` /
``evaluate_program_inference`` / ``mine_supervision`` and what the entry point answers before it would launch anything."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from answer_marginal_reference import answer_marginal_reference  # noqa: E402
from answer_posterior_cases import (ANSWERS, BEYOND_GROUP, DEAD_GROUP, FIXED_SIZES, NEGATIVE_GROUP, SEEDS, ragged_inputs,  # noqa: E402
                                    variants)
from answer_posterior_reference import answer_posterior_reference, top_two_score_margin  # noqa: E402

UNKNOWN = 99


def _brute_force(logits, valid, log_weight, answers, start, w_a):
    """The contract spelled out row by row with torch's ``log_softmax``: (log_answer, log_posterior, log_evidence, best_row,
    support, consistent_count, first_consistent)."""
    R, A = logits.shape
    G = len(start) - 1
    ls = torch.log_softmax(torch.from_numpy(np.asarray(logits, np.float64)), 1).numpy() if R else np.zeros((0, A))
    log_answer, log_posterior = np.full(R, np.nan), np.full(R, -np.inf)
    log_evidence, best_row, support = np.full(G, -np.inf), np.full(G, -1), np.zeros(G, int)
    consistent, first = np.zeros(G, int), np.full(G, -1)
    for g in range(G):
        a = int(answers[g])
        rows = list(range(start[g], start[g + 1]))
        for r in rows:
            log_answer[r] = ls[r, a] if 0 <= a < A else -np.inf
        base = [r for r in rows if (valid is None or valid[r]) and (log_weight is None or np.isfinite(log_weight[r]))]
        if not base:
            continue
        lw = torch.tensor([0.0 if log_weight is None else float(log_weight[r]) for r in base], dtype=torch.float64)
        log_w = torch.log_softmax(lw, 0).numpy()
        score = {r: log_w[i] + (w_a * log_answer[r] if w_a != 0 else 0.0) for i, r in enumerate(base)}
        usable = [r for r in base if np.isfinite(score[r])]
        support[g] = len(usable)
        if not usable:
            continue
        s = torch.tensor([score[r] for r in usable], dtype=torch.float64)
        log_evidence[g] = float(torch.logsumexp(s, 0))
        log_posterior[usable] = torch.log_softmax(s, 0).numpy()
        best_row[g] = usable[int(s.argmax())]
        agree = [r for r in usable if int(np.argmax(logits[r])) == a]
        consistent[g] = len(agree)
        first[g] = agree[0] if agree else -1
    return log_answer, log_posterior, log_evidence, best_row, support, consistent, first


def _hand_made():
    """Six groups over 14 rows of 5 answers: an empty group, an all-invalid one, an out-of-range answer, -inf at the target of
    one row, a weight of -inf, and an ordinary one."""
    rng = np.random.default_rng(7)
    start = np.array([0, 0, 2, 5, 8, 11, 14])
    logits = rng.standard_normal((14, 5)) * 3
    valid = np.ones(14, np.int32)
    valid[0:2] = 0                            # group 1: every program invalid
    answers = np.array([1, 2, 7, 3, 0, 4])    # group 2: the answer is no index
    logits[5, 3] = -np.inf                    # group 3: -inf at the target of its first row
    log_weight = rng.standard_normal(14) * 2 - 5
    log_weight[9] = -np.inf                   # group 4: the generator rules its middle row out
    valid[12] = 0                             # group 5: one invalid row
    return logits, valid, log_weight, answers, start


@pytest.mark.parametrize("w_a", [1.0, 0.5, 0.0, -2.0])
@pytest.mark.parametrize("given", ["both", "neither"])
def test_reference_equals_a_brute_force_log_softmax_on_hand_made_cases(w_a, given):
    logits, valid, log_weight, answers, start = _hand_made()
    v, lw = (valid, log_weight) if given == "both" else (None, None)
    ref = answer_posterior_reference(logits, v, lw, answers, start, w_a, UNKNOWN)
    log_answer, log_posterior, log_evidence, best_row, support, consistent, first = _brute_force(logits, v, lw, answers, start, w_a)
    assert ref["covered"].all()
    np.testing.assert_allclose(ref["log_answer"], log_answer, rtol=1e-12, atol=1e-12)
    assert np.array_equal(np.isneginf(ref["log_posterior"]), np.isneginf(log_posterior))
    fin = np.isfinite(log_posterior)
    np.testing.assert_allclose(ref["log_posterior"][fin], log_posterior[fin], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["log_evidence"], log_evidence, rtol=1e-12, atol=1e-12)
    for name, want in (("best_row", best_row), ("support", support), ("consistent_count", consistent), ("first_consistent", first)):
        assert np.array_equal(ref[name], want), name
    assert np.array_equal(ref["usable"], fin)
    # what the cases are there for
    assert support[0] == 0 and best_row[0] == -1 and first[0] == -1 and np.isneginf(log_evidence[0])          # empty
    assert np.isneginf(ref["log_answer"][2:5]).all() and np.isneginf(ref["log_answer"][5])                      # no index; -inf at the target
    if given == "both":
        assert support[1] == 0 and (ref["row_predictions"][:2] == UNKNOWN).all() and np.isfinite(ref["log_answer"][:2]).all()
        assert not ref["usable"][9] and not ref["usable"][12] and ref["row_predictions"][12] == UNKNOWN
    if w_a != 0.0:
        assert support[2] == 0 and consistent[2] == 0 and not ref["usable"][5]
    else:  # the answer term is left out: no 0 * -inf, the rows count, and none of them can agree with an answer that is no index
        assert support[2] == 3 and consistent[2] == 0 and ref["usable"][5] and np.isneginf(ref["log_answer"][5])
        for g in range(1, 6):
            rows = np.arange(start[g], start[g + 1])[ref["usable"][start[g]:start[g + 1]]]
            if rows.size:
                w = np.zeros(rows.size) if lw is None else lw[rows]
                np.testing.assert_allclose(ref["log_posterior"][rows], torch.log_softmax(torch.from_numpy(w), 0).numpy(), rtol=1e-12, atol=1e-12)
                assert abs(ref["log_evidence"][g]) < 1e-12  # (the normalised weights sum to one)
    shares = np.array([np.exp(ref["log_posterior"][start[g]:start[g + 1]]).sum() for g in range(6)])
    np.testing.assert_allclose(shares[support > 0], 1.0, rtol=1e-12)
    m = top_two_score_margin(ref["score"], ref["usable"], start)
    for g in range(6):
        s = np.sort(ref["score"][start[g]:start[g + 1]][ref["usable"][start[g]:start[g + 1]]])
        assert m[g] == (s[-1] - s[-2] if s.size >= 2 else np.inf)


@pytest.mark.parametrize("A", ANSWERS)
def test_evidence_with_unit_answer_weight_is_the_marginal_of_the_given_answer(A):
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    logits = np.where(np.isneginf(logits), np.float32(-60.0), logits)  # (the marginal's contract is stated for finite logits)
    for v, lw in ((valid, log_weight), (None, None)):
        ref = answer_posterior_reference(logits, v, lw, answers, start, 1.0, A)
        marginal = answer_marginal_reference(logits, v, lw, start, A)
        assert np.array_equal(ref["row_predictions"], marginal["row_predictions"])
        for g in range(len(start) - 1):
            if 0 <= answers[g] < A:
                want = marginal["log_marginal"][g, answers[g]]
                assert ref["support"][g] == marginal["support"][g]
                assert np.isneginf(want) if ref["support"][g] == 0 else abs(ref["log_evidence"][g] - want) <= 1e-10, g
            else:
                assert np.isneginf(ref["log_evidence"][g]) and ref["support"][g] == 0


@pytest.mark.parametrize("A", ANSWERS)
def test_the_seeds_of_the_device_test_hold_on_the_reference(A):
    """No supported group is left out of the ``best_row`` comparison, and at least 28 groups are supported."""
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    assert len(start) - 1 == 37 and (np.diff(start)[:12] == FIXED_SIZES).all()
    assert 0.03 < (valid == 0).mean() < 0.2 and np.isneginf(log_weight).any()
    assert np.isneginf(log_weight[start[DEAD_GROUP]:start[DEAD_GROUP + 1]]).all()
    assert answers[BEYOND_GROUP] == A + 3 and answers[NEGATIVE_GROUP] == -2
    assert (np.abs(logits[np.isfinite(logits).all(1)]).max(1) > 24).any()  # (rows scaled by 8)
    for w_a, lw in variants(A, log_weight):
        ref = answer_posterior_reference(logits, valid, lw, answers, start, w_a, A)
        tolerance = 1e-5 * (1.0 + ref["max_abs_score"])
        margin = top_two_score_margin(ref["score"], ref["usable"], start)
        supported = ref["support"] > 0
        assert (margin[supported] >= 100 * tolerance[supported]).all(), (w_a, lw is None)
        assert supported.sum() >= 28
        assert ref["support"][0] == 0 and ref["support"][10] == 0 and ref["support"][BEYOND_GROUP] == ref["support"][NEGATIVE_GROUP] == 0
        if lw is not None:
            assert ref["support"][DEAD_GROUP] == 0
        if A > 1:
            in_range = np.repeat((answers >= 0) & (answers < A), np.diff(start))
            assert np.isneginf(ref["log_answer"][in_range]).any()          # -inf at some targets
    assert len(variants(A, log_weight)) == (3 if A >= 28 else 2)


def test_reference_clamps_group_bounds():
    logits, valid, log_weight, answers, _ = _hand_made()
    ref = answer_posterior_reference(logits[:6], None, None, [0, 1, 2], [-4, 2, 1, 9], 1.0, UNKNOWN)  # rows [0, 2), nothing, [1, 6)
    assert ref["support"][1] == 0 and ref["best_row"][1] == -1 and ref["covered"].all()
    assert 0 <= ref["best_row"][0] < 2 and 1 <= ref["best_row"][2] < 6
    ref = answer_posterior_reference(logits[:6], None, None, [0, 1], [3, 3, 5], 1.0, UNKNOWN)
    assert ref["covered"].tolist() == [False, False, False, True, True, False]
    assert np.isnan(ref["log_answer"][~ref["covered"]]).all() and np.isneginf(ref["log_posterior"][~ref["covered"]]).all()


@pytest.mark.parametrize("options", [
    dict(),                                                                         # no hypotheses
    dict(beam_size=4, num_programs=4),                                              # samples and a search
    dict(num_programs=1), dict(num_programs=65), dict(num_programs=4.0), dict(num_programs=True),
    dict(constrained=True, num_programs=4), dict(constrained=True),                 # constrains a beam search
    dict(constrained_sampling=True, beam_size=4),
    dict(beam_size=4, without_replacement=True),
    dict(num_programs=3, without_replacement=True),                                 # not a beam size
    dict(num_programs=4, sample_weights="importance"),                              # weighs a sample without replacement
    dict(num_programs=4, without_replacement=True, sample_weights="gumbel"),
    dict(beam_size=4, answer_weight=float("nan")), dict(beam_size=4, answer_weight=float("inf")),
    dict(beam_size=4, answer_weight=None), dict(beam_size=4, answer_weight="much"),
    dict(rerank=True),                                                              # nothing to rerank
    dict(rerank=True, beam_size=4),                                                 # default coefficients, no models
    dict(rerank=True, num_programs=4, question_reconstructor=object()),             # w_z = 1 without the prior
    dict(rerank=True, beam_size=4, program_prior=object()),                         # w_x = 1 without the reconstructor
    dict(rerank=True, beam_size=4, rerank_weights=(0.0, 0.0)),
    dict(rerank=True, beam_size=4, rerank_weights=(0.0, 0.0, float("nan"))),
])
def test_program_inference_is_refused_before_a_model_is_touched(options):
    from probnmn.evaluators import evaluate_program_inference, infer_programs, mine_supervision

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("a model was touched: .%s" % name)

    def batches():
        raise AssertionError("a batch was asked for")
        yield

    for fn in (infer_programs, evaluate_program_inference, mine_supervision):
        with pytest.raises(ValueError):
            fn(Untouchable(), Untouchable(), batches(), None, **options)
    with pytest.raises(TypeError):
        mine_supervision(Untouchable(), Untouchable(), batches(), None, beam_size=4, marginal=True)  # (no option of infer_programs)


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device():
    import ctypes

    from probnmn import _hip

    sig = _hip.SIGNATURES["pnmn_answer_posterior"]
    assert len(sig) == 19 and sig[5] is ctypes.c_float and sig[14:18] == (ctypes.c_int,) * 4
    assert all(t is ctypes.c_void_p for i, t in enumerate(sig) if i != 5 and not 14 <= i < 18)
    assert _hip.ABI_VERSION == 14 and len(_hip.SIGNATURES) == 103
    fn = _hip.lib().pnmn_answer_posterior
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)

    def call(logits=p, answers=p, group_start=p, w_a=1.0, log_posterior=p, log_evidence=p, best_row=p, n_groups=1, n_rows=2, A=4):
        return fn(logits, 0, 0, answers, group_start, w_a, 0, 0, log_posterior, log_evidence, best_row, 0, 0, 0, n_groups, n_rows, A, 0, 0)

    for missing in ("group_start", "answers", "log_posterior", "log_evidence", "best_row", "logits"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL
    assert call(A=0) == _hip.EINVAL and call(A=-3) == _hip.EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(w_a=bad) == _hip.EINVAL, bad
    assert call(A=1025) == _hip.ESHAPE and call(A=1025, w_a=float("nan")) == _hip.EINVAL
    # without a group there is nothing to do, whatever else is given
    assert call(n_groups=0) == 0 and call(n_groups=0, n_rows=0, logits=0, answers=0, group_start=0, log_posterior=0) == 0
