"""``pnmn_answer_posterior`` and what is built on it, on the MI355X: the kernel against the fp64 reference of
tests/helpers/answer_posterior_reference.py over ragged groups, ties, a zero answer weight, the evidence against one
``pnmn_answer_marginal`` launch, bitwise independence of a group from its batch, clamped group bounds, the argument checks;
``NeuralModuleNetwork.answer_posterior`` against the network's own logits; ``infer_programs``, ``evaluate_program_inference``
and ``mine_supervision``.

Tolerances.  ``log_answer``: rtol = atol = 1e-5, the project's bar for log-softmax quantities
(tests/test_hip_kernels.py::test_answer_loss): one term (z[a] - max) - log sum exp, a few fp32 ulps of its own size.
``log_posterior`` / ``log_evidence``: 1e-5 * (1 + the largest |score| among the group's usable rows) -- the posterior is a
DIFFERENCE of scores, so it inherits their absolute error, not their relative one.  ``row_predictions``, ``support``,
``consistent_count``, ``first_consistent`` and usability are compared exactly: the kernel and numpy compare the same fp32
values.  ``best_row`` is compared where the reference's two best scores differ by 100 x the group's tolerance; the seeds of
tests/helpers/answer_posterior_cases.py are those at which, on the reference alone, that leaves out no supported group."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from answer_posterior_cases import (ANSWERS, BEYOND_GROUP, DEAD_GROUP, FIXED_SIZES, NEGATIVE_GROUP, SEEDS, ragged_inputs,  # noqa: E402
                                    variants)
from answer_posterior_reference import answer_posterior_reference, top_two_score_margin  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)
GUARD = 64     # guard words on either side of every output buffer
ROW_OUTPUTS = ("log_answer", "row_predictions", "log_posterior")
GROUP_OUTPUTS = ("log_evidence", "best_row", "support", "consistent_count", "first_consistent")
OPTIONAL = ("log_answer", "row_predictions", "support", "consistent_count", "first_consistent")


def launch(logits, valid, log_weight, answers, group_start, w_a, unknown, optional=True):
    """One ``pnmn_answer_posterior`` launch on numpy inputs; every output lies between GUARD sentinel words, which must come
    back untouched.  Returns the outputs as numpy (rows no group covers keep the sentinel)."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    R, A = logits.shape
    G = len(group_start) - 1
    # (an input without rows is still an allocation: a null pointer means "not given")
    up = lambda a, dt: None if a is None else (torch.from_numpy(np.ascontiguousarray(a)).to(dt) if len(a) else torch.zeros(1, dtype=dt)).to(dev)  # noqa: E731
    d_logits, d_valid, d_lw = up(logits, torch.float32), up(valid, torch.int32), up(log_weight, torch.float32)
    d_answers = up(np.asarray(answers, np.int64), torch.long)
    d_start = up(np.asarray(group_start, np.int64), torch.int32)
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    bufs = {"log_answer": torch.full((R + 2 * GUARD,), -777.0, **f),
            "row_predictions": torch.full((R + 2 * GUARD,), -777, dtype=torch.long, device=dev),
            "log_posterior": torch.full((R + 2 * GUARD,), -777.0, **f), "log_evidence": torch.full((G + 2 * GUARD,), -777.0, **f),
            "best_row": torch.full((G + 2 * GUARD,), -777, **i), "support": torch.full((G + 2 * GUARD,), -777, **i),
            "consistent_count": torch.full((G + 2 * GUARD,), -777, **i), "first_consistent": torch.full((G + 2 * GUARD,), -777, **i)}
    ptr = lambda name: bufs[name][GUARD:].data_ptr()  # noqa: E731
    opt = lambda name: ptr(name) if optional else 0  # noqa: E731
    rc = _hip.lib().pnmn_answer_posterior(
        d_logits.data_ptr(), 0 if d_valid is None else d_valid.data_ptr(), 0 if d_lw is None else d_lw.data_ptr(),
        d_answers.data_ptr(), d_start.data_ptr(), float(w_a), opt("log_answer"), opt("row_predictions"), ptr("log_posterior"),
        ptr("log_evidence"), ptr("best_row"), opt("support"), opt("consistent_count"), opt("first_consistent"), G, R, A, unknown,
        _hip.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == -777).all() and (host[-GUARD:] == -777).all(), name
        out[name] = host[GUARD:-GUARD]
    return out


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def row_tolerance(ref, start):
    """1e-5 * (1 + largest |score| of the group) per group, and the same spread over the group's rows."""
    per_group = 1e-5 * (1.0 + ref["max_abs_score"])
    per_row = np.zeros(ref["score"].size)
    for g in range(len(start) - 1):
        per_row[start[g]:start[g + 1]] = per_group[g]
    return per_group, per_row


def check_against_reference(got, ref, start, best=True):
    """Every row is covered here."""
    per_group, per_row = row_tolerance(ref, start)
    inf = np.isneginf(ref["log_answer"])
    assert np.array_equal(np.isneginf(got["log_answer"]), inf) and not np.isnan(got["log_answer"]).any()
    np.testing.assert_allclose(got["log_answer"][~inf], ref["log_answer"][~inf], **TOL)
    assert np.array_equal(got["row_predictions"], ref["row_predictions"])
    usable = ref["usable"]
    assert np.array_equal(np.isfinite(got["log_posterior"]), usable)  # usability, exactly
    assert np.isneginf(got["log_posterior"][~usable]).all()
    for name in ("support", "consistent_count", "first_consistent"):
        assert np.array_equal(got[name], ref[name]), name
    assert (np.abs(got["log_posterior"][usable] - ref["log_posterior"][usable]) <= per_row[usable]).all()
    supported = ref["support"] > 0
    assert np.isneginf(got["log_evidence"][~supported]).all() and (got["best_row"][~supported] == -1).all()
    assert (got["consistent_count"][~supported] == 0).all() and (got["first_consistent"][~supported] == -1).all()
    assert (np.abs(got["log_evidence"][supported] - ref["log_evidence"][supported]) <= per_group[supported]).all()
    assert (usable[got["best_row"][supported]]).all()
    if best:  # the MAP row is the reference's, the margin being what the caller asserted ...
        assert np.array_equal(got["best_row"], ref["best_row"])
        for g in np.nonzero(supported)[0]:  # ... and the first row with the largest posterior the device itself wrote
            lp = got["log_posterior"][start[g]:start[g + 1]]
            assert got["best_row"][g] == start[g] + int(np.argmax(lp == lp.max())), g


@pytest.mark.parametrize("A", ANSWERS)
def test_kernel_against_fp64_reference(A):
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    assert len(start) - 1 == 37 and (np.diff(start)[:12] == FIXED_SIZES).all()
    # what the inputs are required to hold
    assert (valid == 0).any() and np.isneginf(log_weight).any() and np.isneginf(log_weight[start[DEAD_GROUP]:start[DEAD_GROUP + 1]]).all()
    assert answers[BEYOND_GROUP] == A + 3 and answers[NEGATIVE_GROUP] == -2 and (A == 1 or np.isneginf(logits).any())
    for w_a, lw in variants(A, log_weight):
        ref = answer_posterior_reference(logits, valid, lw, answers, start, w_a, A)
        per_group, per_row = row_tolerance(ref, start)
        margin = top_two_score_margin(ref["score"], ref["usable"], start)
        supported = ref["support"] > 0
        print("A = %d, w_a %s, weights %s: smallest top-two margin / (100 x tolerance) %.3g over %d supported groups"
              % (A, w_a, "given" if lw is not None else "null", (margin / (100 * per_group))[supported].min(), int(supported.sum())))
        # (of the reference alone: no supported group is left out of the best_row comparison below)
        assert (margin[supported] >= 100 * per_group[supported]).all() and supported.sum() >= 28
        assert ref["support"][0] == 0 and (lw is None or ref["support"][DEAD_GROUP] == 0)
        got = launch(logits, valid, lw, answers, start, w_a, A)
        usable = ref["usable"]
        print("    largest |log_posterior - reference| / tolerance: %.3g"
              % (np.abs(got["log_posterior"][usable] - ref["log_posterior"][usable]) / per_row[usable]).max())
        check_against_reference(got, ref, start)
        # the optional outputs left out: the required ones are the same bits
        bare = launch(logits, valid, lw, answers, start, w_a, A, optional=False)
        for name in ("log_posterior", "log_evidence", "best_row"):
            assert np.array_equal(bits(bare[name]), bits(got[name])), name
        for name in OPTIONAL:
            assert (bare[name] == -777).all(), name
    # neither validity nor weights: every row is base-usable
    ref = answer_posterior_reference(logits, None, None, answers, start, 1.0, A)
    check_against_reference(launch(logits, None, None, answers, start, 1.0, A), ref, start, best=False)


def test_exact_ties_take_the_first_row():
    rng = np.random.default_rng(5)
    A = 28
    for size, first, second in ((9, 2, 5), (70, 3, 67), (70, 66, 7), (130, 64, 128)):
        logits = (rng.standard_normal((size, A)) * 2).astype(np.float32)
        lw = (rng.standard_normal(size) - 30).astype(np.float32)
        lo, hi = min(first, second), max(first, second)
        logits[hi] = logits[lo]                       # the same row twice (in different sweeps), on top of the group
        logits[lo, 4] = logits[hi, 4] = logits[lo].max() + 1
        lw[hi] = lw[lo] = 5.0
        got = launch(logits, None, lw, [4], [0, size], 1.0, A)
        lp = got["log_posterior"]
        assert lp[lo] == lp[hi] == lp.max() and got["log_answer"][lo] == got["log_answer"][hi]
        assert got["best_row"][0] == lo and got["support"][0] == size
        assert got["first_consistent"][0] <= lo and got["consistent_count"][0] >= 2
    # one answer and uniform weights: every usable row scores -log(support), so each group's first usable row leads
    logits, valid, _, answers, start = ragged_inputs(1, SEEDS[1])
    ref = answer_posterior_reference(logits, valid, None, answers, start, 1.0, 1)
    assert (ref["log_answer"][np.repeat(answers == 0, np.diff(start))] == 0).all() and (ref["support"] > 1).sum() >= 20
    assert not ref["usable"].all()
    got = launch(logits, valid, None, answers, start, 1.0, 1)
    check_against_reference(got, ref, start)  # (the reference's argmax is the first maximum too)
    for g in np.nonzero(ref["support"] > 0)[0]:
        assert got["best_row"][g] == start[g] + int(np.argmax(ref["usable"][start[g]:start[g + 1]]))
        assert got["first_consistent"][g] == got["best_row"][g] and got["consistent_count"][g] == ref["support"][g]


def test_a_zero_answer_weight_is_the_log_softmax_of_the_weights():
    A = 64
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    full = launch(logits, valid, log_weight, answers, start, 1.0, A)
    none = launch(logits, valid, log_weight, answers, start, 0.0, A)
    assert np.array_equal(bits(none["log_answer"]), bits(full["log_answer"]))  # the term is still reported, the same bits
    assert np.array_equal(none["row_predictions"], full["row_predictions"])
    check_against_reference(none, answer_posterior_reference(logits, valid, log_weight, answers, start, 0.0, A), start, best=False)
    for g in range(37):
        rows = np.arange(start[g], start[g + 1])
        rows = rows[(valid[rows] != 0) & np.isfinite(log_weight[rows])]
        assert none["support"][g] == rows.size  # (-inf at the target, an answer that is no index: the rows count again)
        if rows.size:
            lw = log_weight[rows].astype(np.float64)
            want = lw - lw.max() - np.log(np.exp(lw - lw.max()).sum())
            np.testing.assert_allclose(none["log_posterior"][rows], want, rtol=0, atol=1e-5 * (1 + np.abs(want).max()))
            assert abs(none["log_evidence"][g]) <= 1e-5
    assert none["support"][BEYOND_GROUP] > 0 and none["consistent_count"][BEYOND_GROUP] == 0 and full["support"][BEYOND_GROUP] == 0


@pytest.mark.parametrize("A", [28, 130])
def test_evidence_with_unit_answer_weight_is_the_marginal_of_the_given_answer(A):
    from probnmn import _hip

    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    logits = np.where(np.isneginf(logits), np.float32(-60.0), logits)  # (pnmn_answer_marginal's contract: finite logits)
    ref = answer_posterior_reference(logits, valid, log_weight, answers, start, 1.0, A)
    per_group, _ = row_tolerance(ref, start)
    got = launch(logits, valid, log_weight, answers, start, 1.0, A)
    dev = torch.device("cuda:0")
    G, R = 37, int(start[-1])
    d = [torch.from_numpy(a).to(dev) for a in (logits, valid, log_weight, start)]
    log_marginal = torch.empty(G, A, dtype=torch.float32, device=dev)
    predictions = torch.empty(G, dtype=torch.long, device=dev)
    assert _hip.lib().pnmn_answer_marginal(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), log_marginal.data_ptr(),
                                           predictions.data_ptr(), 0, 0, 0, G, R, A, A, _hip.stream_ptr(dev)) == 0
    log_marginal = log_marginal.cpu().numpy()
    compared = 0
    for g in np.nonzero(ref["support"] > 0)[0]:
        assert abs(got["log_evidence"][g] - log_marginal[g, answers[g]]) <= 2 * per_group[g], g
        compared += 1
    assert compared >= 28


def test_a_group_is_the_same_bits_alone_and_in_a_batch():
    A = 65
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    whole = launch(logits, valid, log_weight, answers, start, 0.5, A)
    again = launch(logits, valid, log_weight, answers, start, 0.5, A)
    for name in whole:
        assert np.array_equal(bits(whole[name]), bits(again[name])), name
    for g in (0, 3, 4, DEAD_GROUP, 6, 7, BEYOND_GROUP, NEGATIVE_GROUP, 20, 36):
        lo, hi = int(start[g]), int(start[g + 1])
        alone = launch(logits[lo:hi], valid[lo:hi], log_weight[lo:hi], answers[g:g + 1], [0, hi - lo], 0.5, A)
        for name in ROW_OUTPUTS:
            assert np.array_equal(bits(alone[name]), bits(whole[name][lo:hi])), (g, name)
        for name in ("log_evidence", "support", "consistent_count"):
            assert bits(alone[name])[0] == bits(whole[name])[g], (g, name)
        for name in ("best_row", "first_consistent"):
            assert alone[name][0] == (whole[name][g] - lo if whole[name][g] >= 0 else -1), (g, name)


def test_group_bounds_are_clamped_into_the_arrays():
    """Correct launches of the kernel with a ``group_start`` that a caller got wrong: every bound is clamped into
    [0, n_rows] with end >= start, so nothing outside the arrays is read or written (``launch`` checks the guard words) and
    the groups that share no row with another give the same bits."""
    A = 28
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    R = int(start[-1])
    base = launch(logits, valid, log_weight, answers, start, 1.0, A)

    # a last entry beyond n_rows and a first one below 0 clamp to what they should have been: nothing changes
    for last in (R + 1000, 2 ** 31 - 1):
        bad = start.astype(np.int64)
        bad[-1], bad[0] = last, -5
        got = launch(logits, valid, log_weight, answers, bad, 1.0, A)
        for name in base:
            assert np.array_equal(bits(got[name]), bits(base[name])), (last, name)

    # every bound out of range on the same side: no group has a row, nothing but the group outputs is written
    for bad in (np.full(38, -9), np.full(38, R + 7)):
        got = launch(logits, valid, log_weight, answers, bad, 1.0, A)
        assert (got["support"] == 0).all() and (got["best_row"] == -1).all() and np.isneginf(got["log_evidence"]).all()
        assert (got["consistent_count"] == 0).all() and (got["first_consistent"] == -1).all()
        assert all((got[name] == -777).all() for name in ROW_OUTPUTS)

    # a decreasing pair: start[4] = 30 > start[5] = 22.  Group 3 becomes rows [3, 30), group 4 is empty; groups 3 and 5 now
    # share rows 22 .. 29, whose row outputs either may write: every OTHER group keeps its bits
    assert start[3] == 3 and start[4] == 6 and start[5] == 22
    bad = start.copy()
    bad[4] = 30
    got = launch(logits, valid, log_weight, answers, bad, 1.0, A)
    others = np.array([g for g in range(37) if g not in (3, 4, 5)])
    for name in GROUP_OUTPUTS:
        assert np.array_equal(bits(got[name])[others], bits(base[name])[others]), name
    assert got["support"][4] == 0 and got["best_row"][4] == -1 and np.isneginf(got["log_evidence"][4])
    outside = np.r_[0:3, int(start[6]):R]
    for name in ROW_OUTPUTS:
        assert np.array_equal(bits(got[name])[outside], bits(base[name])[outside]), name
    assert np.array_equal(got["row_predictions"], base["row_predictions"])  # (a row's own arg-max: whoever writes it)


def test_argument_errors_return_without_a_launch():
    from probnmn import _hip

    dev = torch.device("cuda:0")
    fn = _hip.lib().pnmn_answer_posterior
    out = torch.full((64,), -777.0, device=dev)
    p = out.data_ptr()

    def call(logits=p, answers=p, group_start=p, w_a=1.0, log_posterior=p, log_evidence=p, best_row=p, n_groups=1, n_rows=2, A=4):
        return fn(logits, 0, 0, answers, group_start, w_a, 0, 0, log_posterior, log_evidence, best_row, 0, 0, 0, n_groups, n_rows, A, 0,
                  _hip.stream_ptr(dev))

    for missing in ("group_start", "answers", "log_posterior", "log_evidence", "best_row", "logits"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL and call(A=0) == _hip.EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(w_a=bad) == _hip.EINVAL
    assert call(A=1025) == _hip.ESHAPE and call(n_groups=0) == 0
    torch.cuda.synchronize()
    assert (out == -777).all()  # nothing ran


# ---- the network and the evaluators ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=32).to(dev)
    qr = QuestionReconstructor(vocab).to(dev)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev)
    batch = synthetic_batch(vocab, 8, seed=31)
    return vocab, pg, nmn, qr, prior, batch, dev


def _batches(batch, dev, answers=None, extra=()):
    out = []
    for s in (slice(0, 4), slice(4, 8)):
        b = {k: batch[k][s].to(dev) for k in ("question", "image", "answer") + tuple(extra)}
        if answers is not None:
            b["answer"] = torch.as_tensor(answers[s]).to(dev)
        out.append(b)
    return out


def test_answer_posterior_against_the_networks_own_logits(models):
    vocab, pg, nmn, qr, prior, batch, dev = models
    question_rows = np.array([0, 0, 1, 2, 2, 2, 3, 5, 5, 5, 6, 7])     # (question 4 has no hypothesis)
    programs = batch["program"][[0, 1, 1, 2, 3, 4, 5, 5, 6, 7, 0, 3]]
    image = batch["image"].to(dev)
    log_weights = np.linspace(-3.0, -0.5, 12).astype(np.float32)
    log_weights[4] = -np.inf
    unknown = nmn._unknown_answer
    nmn.eval()
    with torch.no_grad():
        own = nmn(image[torch.from_numpy(question_rows).to(dev)], programs, return_logits=True)
    logits = own["answer_logits"].double().cpu().numpy()
    A = logits.shape[1]
    answers = logits.argmax(1)[[0, 2, 5, 6, 0, 8, 10, 11]].astype(np.int64)  # each question: one of its hypotheses' own answers
    answers[6] = (answers[6] + 1) % A
    metrics = nmn.get_metrics(reset=False)
    nmn.train()

    out = nmn.answer_posterior(image, programs, question_rows, answers, log_weights, answer_weight=0.75)
    in_passes = nmn.answer_posterior(image, programs.to(dev), torch.from_numpy(question_rows).to(dev), torch.from_numpy(answers).to(dev),
                                     torch.from_numpy(log_weights).to(dev), answer_weight=0.75, max_rows=5)
    assert nmn.training and nmn.get_metrics(reset=False) == metrics    # the flag and the metrics are what they were
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert set(got) == {"log_answer_likelihood", "log_posterior", "hypothesis_predictions", "log_evidence", "best_row",
                        "first_consistent_row", "consistent_count", "support"}
    valid = (own["predictions"].cpu().numpy() != unknown).astype(np.int32)
    assert valid.all()
    ls = torch.log_softmax(torch.from_numpy(logits), 1).numpy()        # fp64, per row
    np.testing.assert_allclose(got["log_answer_likelihood"], ls[np.arange(12), answers[question_rows]], **TOL)
    start = np.searchsorted(question_rows, np.arange(9))
    ref = answer_posterior_reference(logits, valid, log_weights, answers, start, 0.75, unknown)
    per_group, per_row = row_tolerance(ref, start)
    usable = ref["usable"]
    assert np.array_equal(np.isfinite(got["log_posterior"]), usable) and not usable[4] and usable.sum() == 11
    assert (np.abs(got["log_posterior"][usable] - ref["log_posterior"][usable]) <= per_row[usable]).all()
    sup = ref["support"] > 0
    assert ref["support"].tolist() == [2, 1, 2, 1, 0, 3, 1, 1] and np.array_equal(got["support"], ref["support"])
    assert (np.abs(got["log_evidence"][sup] - ref["log_evidence"][sup]) <= per_group[sup]).all() and np.isneginf(got["log_evidence"][4])
    margin = top_two_score_margin(ref["score"], ref["usable"], start)
    sure = margin >= 100 * per_group
    assert np.array_equal(got["best_row"][sure], ref["best_row"][sure]) and got["best_row"][4] == -1
    sure_rows = np.sort(logits, 1)[:, -1] - np.sort(logits, 1)[:, -2] >= 1e-3   # rows whose own answer leads clearly
    assert np.array_equal(got["hypothesis_predictions"][sure_rows], ref["row_predictions"][sure_rows])
    # the consistent rows, in the questions whose rows' own answers all lead clearly (not vacuous: most questions are such)
    sure_groups = np.array([sure_rows[start[g]:start[g + 1]].all() for g in range(8)])
    assert sure_groups.sum() >= 6
    assert np.array_equal(got["consistent_count"][sure_groups], ref["consistent_count"][sure_groups])
    assert np.array_equal(got["first_consistent_row"][sure_groups], ref["first_consistent"][sure_groups])
    given_own = np.array([0, 1, 2, 3, 5, 7])  # questions given one of their counting hypotheses' own answers
    assert (ref["consistent_count"][given_own] >= 1).all() and ref["first_consistent"][0] == 0 and ref["consistent_count"][4] == 0
    # passes of five rows stay within the tolerance of one pass, and of the reference
    again = {k: v.cpu().numpy() for k, v in in_passes.items()}
    np.testing.assert_allclose(again["log_answer_likelihood"], got["log_answer_likelihood"], **TOL)
    np.testing.assert_allclose(again["log_answer_likelihood"], ls[np.arange(12), answers[question_rows]], **TOL)
    assert np.array_equal(np.isfinite(again["log_posterior"]), usable) and np.array_equal(again["support"], got["support"])
    for name, other in (("one pass", got), ("the reference", {"log_posterior": ref["log_posterior"], "log_evidence": ref["log_evidence"]})):
        d_row = np.abs(again["log_posterior"][usable] - other["log_posterior"][usable]) / per_row[usable]
        d_group = np.abs(again["log_evidence"][sup] - other["log_evidence"][sup]) / per_group[sup]
        print("passes of 5 rows against %s: largest |difference| / tolerance %.3g (log_posterior), %.3g (log_evidence)"
              % (name, d_row.max(), d_group.max()))
        assert (d_row <= 1).all() and (d_group <= 1).all(), name
    assert np.array_equal(again["best_row"][sure], ref["best_row"][sure])
    assert np.array_equal(again["consistent_count"][sure_groups], ref["consistent_count"][sure_groups])

    # no hypothesis at all; arguments that are wrong
    none = nmn.answer_posterior(image, programs[:0], np.zeros(0, np.int64), answers)
    assert none["support"].tolist() == [0] * 8 and none["best_row"].tolist() == [-1] * 8 and none["first_consistent_row"].tolist() == [-1] * 8
    assert torch.isneginf(none["log_evidence"]).all() and none["log_posterior"].shape == (0,)
    for bad in (dict(question_rows=np.array([1, 0])), dict(question_rows=np.array([0, 8])), dict(answers=answers[:7]),
                dict(answers=answers.astype(np.float32)), dict(answer_weight=float("nan")), dict(answer_weight=None),
                dict(log_weights=np.zeros(3)), dict(max_rows=0)):
        kwargs = dict(question_rows=np.array([0, 1]), answers=answers)
        kwargs.update(bad)
        with pytest.raises(ValueError):
            nmn.answer_posterior(image, programs[:2], kwargs.pop("question_rows"), kwargs.pop("answers"), **kwargs)
    assert nmn.training


RECORD_KEYS = {"question_index", "answer", "support", "log_answer_evidence", "consistent_count", "map_program", "map_answer",
               "map_consistent", "first_consistent_rank", "hypotheses"}
HYPOTHESIS_KEYS = {"program", "prior_weight", "weight", "log_answer_likelihood", "answer", "consistent"}


def _check_records(records, hypothesis_keys=HYPOTHESIS_KEYS):
    assert len(records) == 8 and [r["question_index"] for r in records] == list(range(8))
    for r in records:
        assert set(r) == RECORD_KEYS and len(r["hypotheses"]) == r["support"] >= 1  # (a constrained beam: valid programs only)
        assert all(set(h) == hypothesis_keys for h in r["hypotheses"])
        weights = np.array([h["weight"] for h in r["hypotheses"]])
        assert weights.sum() == pytest.approx(1.0, abs=1e-5) and sum(h["prior_weight"] for h in r["hypotheses"]) == pytest.approx(1.0, abs=1e-5)
        heaviest = [h for h in r["hypotheses"] if h["weight"] == weights.max()]
        assert any(r["map_program"] == h["program"] and r["map_answer"] == h["answer"] for h in heaviest)
        assert r["map_consistent"] == (r["map_answer"] == r["answer"])
        consistent = [k for k, h in enumerate(r["hypotheses"]) if h["consistent"]]
        assert all(h["consistent"] == (h["answer"] == r["answer"]) for h in r["hypotheses"])
        assert r["consistent_count"] == len(consistent) and r["first_consistent_rank"] == (consistent[0] if consistent else None)
        assert np.isfinite(r["log_answer_evidence"]) and r["log_answer_evidence"] <= 1e-5


def test_infer_programs_over_the_constrained_beam(models):
    from probnmn.evaluators import evaluate_program_inference, infer_programs

    vocab, pg, nmn, qr, prior, batch, dev = models
    first = infer_programs(pg, nmn, _batches(batch, dev), vocab, beam_size=4, constrained=True)
    _check_records(first)
    assert all(r["answer"] == vocab.get_token_from_index(int(a), namespace="answers") for r, a in zip(first, batch["answer"].tolist()))
    # every question given the own answer of one of its hypotheses (the last one): the posterior must find it
    stoi = vocab.get_token_to_index_vocabulary("answers")
    picked = [len(r["hypotheses"]) - 1 for r in first]
    answers = np.array([stoi[r["hypotheses"][k]["answer"]] for r, k in zip(first, picked)], np.int64)
    batches = _batches(batch, dev, answers)
    records = infer_programs(pg, nmn, batches, vocab, beam_size=4, constrained=True)
    _check_records(records)
    for r, f, k in zip(records, first, picked):
        assert [h["program"] for h in r["hypotheses"]] == [h["program"] for h in f["hypotheses"]]  # (a deterministic search)
        assert r["consistent_count"] >= 1 and r["hypotheses"][k]["consistent"] and r["first_consistent_rank"] <= k
        assert r["first_consistent_rank"] == [h["answer"] for h in r["hypotheses"]].index(r["answer"])
        # the weights: softmax of log prior share + log p(a | z, image), recomputed on the host
        s = np.log([h["prior_weight"] for h in r["hypotheses"]]) + np.array([h["log_answer_likelihood"] for h in r["hypotheses"]])
        want = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
        np.testing.assert_allclose([h["weight"] for h in r["hypotheses"]], want, rtol=1e-4, atol=1e-5)
    # answer_weight = 0: the weights before the answer
    plain = infer_programs(pg, nmn, batches, vocab, beam_size=4, constrained=True, answer_weight=0.0)
    for r in plain:
        np.testing.assert_allclose([h["weight"] for h in r["hypotheses"]], [h["prior_weight"] for h in r["hypotheses"]], **TOL)

    m = evaluate_program_inference(pg, nmn, batches, vocab, beam_size=4, constrained=True)
    assert set(m) == {"answer_recall", "map_consistency", "proposal_consistency", "average_support", "average_consistent",
                      "average_rows_per_question"}
    assert m["answer_recall"] == sum(r["consistent_count"] > 0 for r in records) / 8 == 1.0
    assert m["map_consistency"] == sum(r["map_consistent"] for r in records) / 8
    assert m["proposal_consistency"] == sum(r["hypotheses"][0]["consistent"] for r in records) / 8
    assert m["average_support"] == m["average_rows_per_question"] == sum(r["support"] for r in records) / 8
    assert m["average_consistent"] == sum(r["consistent_count"] for r in records) / 8
    annotated = evaluate_program_inference(pg, nmn, _batches(batch, dev, answers, extra=("program",)), vocab, beam_size=4, constrained=True)
    assert set(annotated) == set(m) | {"program_accuracy_with_answer", "program_accuracy_without_answer"}
    assert all(annotated[k] == m[k] for k in m)
    truth = [[vocab.get_token_from_index(int(t), namespace="programs") for t in row if t != 0] for row in batch["program"].tolist()]
    strip = lambda p: [t for t in p if t not in ("@start@", "@end@")]  # noqa: E731
    assert annotated["program_accuracy_with_answer"] == sum(strip(r["map_program"]) == t for r, t in zip(records, truth)) / 8
    before = [max(r["hypotheses"], key=lambda h: h["weight"])["program"] for r in plain]
    assert annotated["program_accuracy_without_answer"] == sum(strip(p) == t for p, t in zip(before, truth)) / 8
    assert pg.training and nmn.training


def test_infer_programs_reranked_by_the_generative_model(models):
    from probnmn.evaluators import infer_programs, predict_answers

    vocab, pg, nmn, qr, prior, batch, dev = models
    batches = _batches(batch, dev)
    records = infer_programs(pg, nmn, batches, vocab, beam_size=4, constrained=True, rerank=True, question_reconstructor=qr,
                             program_prior=prior, answer_weight=0.5)
    _check_records(records, HYPOTHESIS_KEYS | {"log_reconstruction", "log_prior"})
    reranked = predict_answers(pg, nmn, batches, vocab, beam_size=4, constrained=True, rerank=True, question_reconstructor=qr,
                               program_prior=prior)
    several = 0
    for r, p in zip(records, reranked):
        assert [h["program"] for h in r["hypotheses"]] == [h["program"] for h in p["hypotheses"]]
        # the share before the answer is hypothesis_posterior's ...
        np.testing.assert_allclose([h["prior_weight"] for h in r["hypotheses"]], [h["weight"] for h in p["hypotheses"]], rtol=1e-4, atol=1e-5)
        # ... and the weights are the softmax of log_posterior + answer_weight * log_answer_likelihood, recomputed on the host
        lp = np.array([h["log_reconstruction"] + h["log_prior"] for h in r["hypotheses"]], np.float64)
        s = (lp - lp.max() - np.log(np.exp(lp - lp.max()).sum())) + 0.5 * np.array([h["log_answer_likelihood"] for h in r["hypotheses"]])
        want = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
        tol = 1e-5 * (1 + np.abs(lp).max())
        assert (np.abs(np.array([h["weight"] for h in r["hypotheses"]]) - want) <= tol).all()
        several += len(r["hypotheses"]) > 1
    assert several >= 4
    assert pg.training and nmn.training and qr.training and prior.training


def test_mine_supervision(models):
    from probnmn.evaluators import infer_programs, mine_supervision

    vocab, pg, nmn, qr, prior, batch, dev = models
    batches = _batches(batch, dev, extra=("program", "supervision"))
    for b in batches:
        b["supervision"] = torch.tensor([1, 0, 0, 1])
    records = infer_programs(pg, nmn, batches, vocab, beam_size=4, constrained=True, rerank=True, question_reconstructor=qr,
                             program_prior=prior)
    options = dict(beam_size=4, constrained=True, rerank=True, question_reconstructor=qr, program_prior=prior)
    stoi = vocab.get_token_to_index_vocabulary("programs")
    k = 0
    for b, m in zip(batches, mine_supervision(pg, nmn, batches, vocab, min_posterior=0.0, require_consistent=False, **options)):
        assert set(m) == set(b) | {"mined"} and m["question"] is b["question"] and m["program"] is not b["program"]
        assert m["mined"].tolist() == [False, True, True, False] and m["supervision"].tolist() == [1, 1, 1, 1]
        assert b["supervision"].tolist() == [1, 0, 0, 1] and m["program"].shape == b["program"].shape
        assert pg.training and nmn.training  # (while the caller holds a batch)
        for i in range(4):
            if not m["mined"][i]:
                assert torch.equal(m["program"][i], b["program"][i])  # supervised rows: bit for bit
            else:
                want = [stoi[t] for t in records[k + i]["map_program"] if t not in ("@start@", "@end@")]
                assert m["program"][i].tolist() == want + [0] * (b["program"].size(1) - len(want)) and len(want) >= 1
        k += 4
    none = list(mine_supervision(pg, nmn, batches, vocab, min_posterior=1.5, require_consistent=False, **options))
    assert len(none) == 2 and not any(m["mined"].any() for m in none)
    assert all(torch.equal(m["program"], b["program"]) and m["supervision"].tolist() == [1, 0, 0, 1] for m, b in zip(none, batches))
    # only programs that answer correctly, at any share
    consistent = list(mine_supervision(pg, nmn, batches, vocab, min_posterior=0.0, **options))
    got = [bool(v) for m in consistent for v in m["mined"].tolist()]
    assert got == [r["map_consistent"] and s == 0 for r, s in zip(records, [1, 0, 0, 1] * 2)]
    # a program wider than the batch's is not mined
    narrow = [dict(b, program=b["program"][:, :1].contiguous()) for b in batches]
    mined = [bool(v) for m in mine_supervision(pg, nmn, narrow, vocab, min_posterior=0.0, require_consistent=False, **options)
             for v in m["mined"].tolist()]
    fits = [len([t for t in r["map_program"] if t != "@end@"]) <= 1 for r in records]
    assert mined == [f and s == 0 for f, s in zip(fits, [1, 0, 0, 1] * 2)] and not all(fits)
    assert pg.training and nmn.training and qr.training and prior.training
