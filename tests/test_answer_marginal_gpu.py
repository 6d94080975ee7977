"""``pnmn_answer_marginal`` and what is built on it, on the MI355X: the kernel against the fp64 reference of
tests/helpers/answer_marginal_reference.py over ragged groups, ties, the identities of a weighted mixture, bitwise
independence of a group from its batch, clamped group bounds; ``NeuralModuleNetwork.marginal_answers`` against the network
run row by row; ``predict_answers(marginal= / num_programs=)`` and ``evaluate_marginal_answer_accuracy``.

Tolerance on log-probabilities and weights: rtol = atol = 1e-5, the project's bar for log-softmax quantities
(tests/test_hip_kernels.py::test_answer_loss).  The kernel rounds every term at its own size -- (z - max) - log sum exp and
(lw - max) - log sum exp, then a running (maximum, sum) over at most 65 rows here -- so its error is a few fp32 ulps of the
value (6e-8 relative each) plus at most 65 * 6e-8 = 4e-6 from the sum: inside the bar."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from answer_marginal_reference import answer_marginal_reference, top_two_margin  # noqa: E402

from fixtures import VALIDITY_CASES, encode_programs  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)
MARGIN = 1e-3  # a prediction is compared only where the reference's best answer leads by this much (100 x the tolerance)
GUARD = 64     # guard words on either side of every output buffer
FIXED_SIZES = [0, 1, 2, 3, 16, 17, 64, 65, 5, 1, 0, 7]
INVALID_GROUP = 5  # (the 17 rows)
# one seed per number of answers at which, on the reference alone, every supported group's best answer leads by MARGIN,
# with valid / log_weight given and with both null (searched on the CPU; most seeds do).  257 and 513 are the first widths
# of the NPER 8 and 16 kernels (one live column in their register 4 and 8), 1024 the full width: of the seeds 0 .. 39, 27, 20
# and 11 hold there (and leave at least 30 groups supported); the first of each is taken
SEEDS = {1: 0, 2: 2, 28: 0, 29: 1, 64: 3, 65: 4, 130: 6, 257: 0, 513: 0, 1024: 1}


def ragged_inputs(A: int, seed: int):
    """37 groups (not a multiple of the four a workgroup takes): FIXED_SIZES and 25 groups of 1 .. 8 rows."""
    rng = np.random.default_rng(1000 * A + seed)
    sizes = np.array(FIXED_SIZES + rng.integers(1, 9, 25).tolist())
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    R = int(start[-1])
    logits = (rng.standard_normal((R, A)) * 3).astype(np.float32)
    logits[rng.random(R) < 0.1] *= 25  # rows far out in the exponent range
    valid = (rng.random(R) < 0.7).astype(np.int32)
    valid[start[INVALID_GROUP]:start[INVALID_GROUP + 1]] = 0
    log_weight = (rng.standard_normal(R) * 4 - 20).astype(np.float32)
    log_weight[rng.random(R) < 0.1] = -np.inf
    return logits, valid, log_weight, start


def launch(logits, valid, log_weight, group_start, unknown, optional=True):
    """One ``pnmn_answer_marginal`` launch on numpy inputs; every output lies between GUARD sentinel words, which must come
    back untouched.  Returns the outputs as numpy (rows no group covers keep the sentinel)."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    R, A = logits.shape
    G = len(group_start) - 1
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)  # noqa: E731
    d_logits, d_valid, d_lw = up(logits, torch.float32), up(valid, torch.int32), up(log_weight, torch.float32)
    d_start = up(np.asarray(group_start, np.int64), torch.int32)
    bufs = {"log_marginal": torch.full((G * A + 2 * GUARD,), -777.0, dtype=torch.float32, device=dev),
            "predictions": torch.full((G + 2 * GUARD,), -777, dtype=torch.long, device=dev),
            "row_predictions": torch.full((R + 2 * GUARD,), -777, dtype=torch.long, device=dev),
            "row_weight": torch.full((R + 2 * GUARD,), -777.0, dtype=torch.float32, device=dev),
            "support": torch.full((G + 2 * GUARD,), -777, dtype=torch.int32, device=dev)}
    ptr = lambda name: bufs[name][GUARD:].data_ptr()  # noqa: E731
    opt = lambda name: ptr(name) if optional else 0  # noqa: E731
    rc = _hip.lib().pnmn_answer_marginal(
        d_logits.data_ptr(), 0 if d_valid is None else d_valid.data_ptr(), 0 if d_lw is None else d_lw.data_ptr(),
        d_start.data_ptr(), ptr("log_marginal"), ptr("predictions"), opt("row_predictions"), opt("row_weight"), opt("support"),
        G, R, A, unknown, _hip.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == -777).all() and (host[-GUARD:] == -777).all(), name
        out[name] = host[GUARD:-GUARD]
    out["log_marginal"] = out["log_marginal"].reshape(G, A)
    return out


def check_against_reference(got, ref, predictions=True):
    finite = np.isfinite(ref["log_marginal"])
    assert np.array_equal(np.isneginf(got["log_marginal"]), ~finite)  # -inf exactly where the reference has it
    np.testing.assert_allclose(got["log_marginal"][finite], ref["log_marginal"][finite], **TOL)
    np.testing.assert_allclose(got["row_weight"], ref["row_weight"], **TOL)
    assert np.array_equal(got["row_weight"] == 0, ref["row_weight"] == 0)
    assert np.array_equal(got["support"], ref["support"])
    assert np.array_equal(got["row_predictions"], ref["row_predictions"])
    # the prediction is the first arg-max of the device's OWN log-marginal ...
    own = np.where(ref["support"] > 0, got["log_marginal"].argmax(1), ref["predictions"])
    assert np.array_equal(got["predictions"], own)
    if predictions:  # ... and the reference's, the margin being what the caller asserted
        assert np.array_equal(got["predictions"], ref["predictions"])


@pytest.mark.parametrize("A", sorted(SEEDS))
def test_kernel_against_fp64_reference(A):
    logits, valid, log_weight, start = ragged_inputs(A, SEEDS[A])
    assert len(start) - 1 == 37 and (np.diff(start)[:12] == FIXED_SIZES).all()
    for v, lw in ((valid, log_weight), (None, None)):
        ref = answer_marginal_reference(logits, v, lw, start, A)
        margin = top_two_margin(ref["log_marginal"], ref["support"])
        print("A = %d, %s: smallest top-two margin %.3g over %d supported groups" % (A, "given" if v is not None else "null", margin, int((ref["support"] > 0).sum())))
        assert margin >= MARGIN  # (of the reference alone: no group is left out of the comparison below)
        if v is not None:
            assert ref["support"][INVALID_GROUP] == 0 and ref["support"][0] == 0 and (ref["support"] > 0).sum() >= 30
        got = launch(logits, v, lw, start, A)
        finite = np.isfinite(ref["log_marginal"])
        delta = np.abs(got["log_marginal"][finite] - ref["log_marginal"][finite])
        print("    largest |log_marginal - reference| / (atol + rtol |reference|): %.3g"
              % (delta / (TOL["atol"] + TOL["rtol"] * np.abs(ref["log_marginal"][finite]))).max())
        check_against_reference(got, ref)
        # the optional outputs left out: the required ones are the same bits
        bare = launch(logits, v, lw, start, A, optional=False)
        assert np.array_equal(bare["log_marginal"].view(np.int32), got["log_marginal"].view(np.int32))
        assert np.array_equal(bare["predictions"], got["predictions"]) and (bare["support"] == -777).all()


def test_exact_ties_take_the_first_answer():
    rng = np.random.default_rng(5)
    for A, first, second in ((28, 3, 17), (130, 2, 129), (130, 70, 7)):
        logits = (rng.standard_normal((9, A)) * 2).astype(np.float32)
        logits[:, second] = logits[:, first] = logits.max(1) + 1  # the same column twice, on top in every row
        lw = rng.standard_normal(9).astype(np.float32)
        got = launch(logits, None, lw, [0, 9], A)
        lm = got["log_marginal"][0]
        assert lm[first] == lm[second] == lm.max()
        assert got["predictions"][0] == min(first, second) and (got["row_predictions"] == min(first, second)).all()


def test_identities_of_a_weighted_mixture():
    rng = np.random.default_rng(11)
    A, R = 28, 12
    logits = (rng.standard_normal((R, A)) * 3).astype(np.float32)
    lw = (rng.standard_normal(R) * 2 - 5).astype(np.float32)
    start = [0, 1, 5, 12]
    base = launch(logits, None, lw, start, A)
    # a group of one row is that row's log-softmax
    z = logits[0].astype(np.float64)
    np.testing.assert_allclose(base["log_marginal"][0], z - z.max() - np.log(np.exp(z - z.max()).sum()), **TOL)
    assert base["row_weight"][0] == 1.0
    # a constant added to a group's log-weights changes nothing
    shifted = lw.copy()
    shifted[1:5] += 7.5
    np.testing.assert_allclose(launch(logits, None, shifted, start, A)["log_marginal"], base["log_marginal"], **TOL)
    # a row split into two copies of weight w / 2 each changes nothing
    split_logits = np.concatenate([logits[:6], logits[5:]])          # row 5 twice
    split_lw = np.concatenate([lw[:6], lw[5:]])
    split_lw[5:7] -= np.float32(np.log(2.0))
    got = launch(split_logits, None, split_lw, [0, 1, 5, 13], A)
    np.testing.assert_allclose(got["log_marginal"], base["log_marginal"], **TOL)
    np.testing.assert_allclose(got["row_weight"][5] + got["row_weight"][6], base["row_weight"][5], **TOL)
    # uniform log-weights are what null log-weights mean
    uniform = launch(logits, None, np.full(R, -3.25, np.float32), start, A)
    null = launch(logits, None, None, start, A)
    np.testing.assert_allclose(uniform["log_marginal"], null["log_marginal"], **TOL)
    np.testing.assert_allclose(uniform["row_weight"], null["row_weight"], **TOL)
    np.testing.assert_allclose(null["row_weight"], np.repeat(1.0 / np.array([1, 4, 7]), [1, 4, 7]), rtol=1e-6, atol=0)


def test_a_group_is_the_same_bits_alone_and_in_a_batch():
    A = 65
    logits, valid, log_weight, start = ragged_inputs(A, SEEDS[A])
    whole = launch(logits, valid, log_weight, start, A)
    again = launch(logits, valid, log_weight, start, A)
    for name in whole:
        assert np.array_equal(whole[name].view(np.int32 if whole[name].dtype == np.float32 else whole[name].dtype),
                              again[name].view(np.int32 if again[name].dtype == np.float32 else again[name].dtype)), name
    for g in (0, 3, 4, INVALID_GROUP, 6, 7, 11, 20, 36):
        lo, hi = int(start[g]), int(start[g + 1])
        alone = launch(logits[lo:hi], valid[lo:hi], log_weight[lo:hi], [0, hi - lo], A)
        assert np.array_equal(alone["log_marginal"][0].view(np.int32), whole["log_marginal"][g].view(np.int32)), g
        assert alone["predictions"][0] == whole["predictions"][g] and alone["support"][0] == whole["support"][g]
        assert np.array_equal(alone["row_weight"].view(np.int32), whole["row_weight"][lo:hi].view(np.int32)), g
        assert np.array_equal(alone["row_predictions"], whole["row_predictions"][lo:hi]), g


def test_group_bounds_are_clamped_into_the_arrays():
    """Correct launches of the kernel with a ``group_start`` that a caller got wrong: every bound is clamped into
    [0, n_rows] with end >= start, so nothing outside the arrays is read or written (``launch`` checks the guard words)
    and the groups whose bounds are right give the same bits."""
    A = 29
    logits, valid, log_weight, start = ragged_inputs(A, SEEDS[A])
    R = int(start[-1])
    base = launch(logits, valid, log_weight, start, A)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a  # noqa: E731

    # a last entry beyond n_rows and a first one below 0 clamp to what they should have been: nothing changes
    for last in (R + 1000, 2 ** 31 - 1):
        bad = start.astype(np.int64)
        bad[-1], bad[0] = last, -5
        got = launch(logits, valid, log_weight, bad, A)
        for name in base:
            assert np.array_equal(bits(got[name]), bits(base[name])), (last, name)

    # a decreasing pair: start[4] = 30 > start[5] = 22.  Group 3 becomes rows [3, 30), group 4 is empty, the others keep
    # their rows (rows 22 .. 29 are group 3's AND group 5's now: both write their row outputs, either may land)
    assert start[3] == 3 and start[4] == 6 and start[5] == 22
    bad = start.copy()
    bad[4] = 30
    ref = answer_marginal_reference(logits, valid, log_weight, bad, A)
    got = launch(logits, valid, log_weight, bad, A)
    others = np.array([g for g in range(37) if g not in (3, 4)])
    for name in ("log_marginal", "predictions", "support"):
        assert np.array_equal(bits(got[name])[others], bits(base[name])[others]), name
    assert got["support"][4] == 0 and got["predictions"][4] == A and np.isneginf(got["log_marginal"][4]).all()
    assert got["support"][3] == ref["support"][3] > 0
    np.testing.assert_allclose(got["log_marginal"][3], ref["log_marginal"][3], **TOL)
    outside = np.r_[0:3, 30:R]
    assert np.array_equal(bits(got["row_weight"])[outside], bits(base["row_weight"])[outside])
    assert np.array_equal(got["row_predictions"], base["row_predictions"])  # (a row's own arg-max: whoever writes it)
    np.testing.assert_allclose(got["row_weight"][3:22], ref["row_weight"][3:22], **TOL)


def test_more_answers_than_the_widest_kernel_holds_return_without_a_launch():
    from probnmn import _hip

    dev = torch.device("cuda:0")
    out = torch.full((2 * 1025,), -777.0, device=dev)
    p = out.data_ptr()
    # (one group of two rows of 1025 answers: every buffer the kernel would touch lies inside ``out``)
    assert _hip.lib().pnmn_answer_marginal(p, 0, 0, p, p, p, 0, 0, 0, 1, 2, 1025, 0, _hip.stream_ptr(dev)) == _hip.ESHAPE
    torch.cuda.synchronize()
    assert (out == -777).all()  # nothing ran


# ---- the network and the evaluators ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=32).to(dev)
    batch = synthetic_batch(vocab, 8, seed=31)
    return vocab, pg, nmn, batch, dev


def _peaked(pg, vocab):
    """The generator's output bias made so steep that every draw takes the best-ranked token the validity rule allows:
    @end@ as soon as it may, else ``scene``, else ``count``.  Returns the bias to put back."""
    bias = pg._output_projection_layer.bias
    saved = bias.detach().clone()
    with torch.no_grad():
        for rank, token in enumerate(("count", "scene", "@end@"), start=1):
            bias[vocab.get_token_index(token, namespace="programs")] += 40.0 * rank
    return saved


def test_marginal_answers_against_the_network_row_by_row(models):
    from probnmn.data.feature_store import DeviceFeatureStore

    vocab, pg, nmn, batch, dev = models
    stoi = vocab.get_token_to_index_vocabulary("programs")
    good = batch["program"]                                                   # valid programs, length 26
    bad = encode_programs([c for c in VALIDITY_CASES if c in ("scene", "union", "count", "query_color query_color scene")], stoi)
    assert bad.size(0) == 4
    # hypotheses per question 0, 1, 3, 3, 2, 4: valid and invalid ones mixed
    programs = torch.stack([good[0], good[1], bad[0], good[2], bad[1], good[3], good[4], bad[2], bad[3], good[5], good[6], bad[0], good[7]])
    question_rows = np.array([1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 5, 5])
    log_weights = np.array([-1.0, -0.5, -0.1, -2.0, -3.0, -0.3, -1.5, -0.2, -0.4, -2.5, -0.7, -0.1, -1.1], np.float32)
    image = batch["image"][:6].to(dev)
    unknown = vocab.get_token_index("@@UNKNOWN@@", namespace="answers")

    nmn.eval()
    try:
        with torch.no_grad():
            logits, row_valid = [], []
            for r, q in enumerate(question_rows):
                out = nmn(image[q:q + 1], programs[r:r + 1], return_logits=True)
                assert sorted(out) == ["answer_logits", "loss", "predictions"]
                logits.append(out["answer_logits"].cpu().numpy()[0])
                row_valid.append(int(out["predictions"].item() != unknown))
            assert sorted(nmn(image[:1], programs[:1])) == ["loss", "predictions"]  # the default call: today's keys
        assert row_valid == [1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1]
        start = np.searchsorted(question_rows, np.arange(7))
        ref = answer_marginal_reference(np.stack(logits), row_valid, log_weights, start, unknown)
        assert ref["support"].tolist() == [0, 1, 2, 2, 0, 3]
        margins = np.array([top_two_margin(ref["log_marginal"][g:g + 1], ref["support"][g:g + 1]) for g in range(6)])
        print("top-two margins of the reference per question:", margins)
        sure = margins >= MARGIN  # (an unsupported question counts, with inf: its prediction is @@UNKNOWN@@)
        assert (sure & (ref["support"] > 0)).sum() >= 2  # supported questions whose best answer leads clearly

        def check(out, exact_rows=True):
            got = {k: v.cpu().numpy() for k, v in out.items()}
            assert got["predictions"].dtype == np.int64 and got["log_probabilities"].shape == (6, ref["log_marginal"].shape[1])
            finite = np.isfinite(ref["log_marginal"])
            assert np.array_equal(np.isneginf(got["log_probabilities"]), ~finite)
            np.testing.assert_allclose(got["log_probabilities"][finite], ref["log_marginal"][finite], **TOL)
            np.testing.assert_allclose(got["hypothesis_weights"], ref["row_weight"], **TOL)
            assert np.array_equal(got["support"], ref["support"])
            assert np.array_equal(got["predictions"][sure], ref["predictions"][sure])
            assert (got["predictions"][ref["support"] == 0] == unknown).all()
            assert np.array_equal(got["hypothesis_predictions"] == unknown, np.array(row_valid) == 0)
            return got

        from_tensor = check(nmn.marginal_answers(image, programs, question_rows, log_weights))
        check(nmn.marginal_answers(image, programs.to(dev), torch.from_numpy(question_rows).to(dev), torch.from_numpy(log_weights).to(dev)))
        in_passes = check(nmn.marginal_answers(image, programs, question_rows, log_weights, max_rows=4))
        assert np.array_equal(in_passes["predictions"], from_tensor["predictions"])
        store = DeviceFeatureStore(batch["image"].numpy(), dev, chunk_rows=3)
        resident = check(nmn.marginal_answers(store.batch(torch.arange(6)), programs, question_rows, log_weights))
        assert np.array_equal(resident["predictions"], from_tensor["predictions"])
        nhwc = check(nmn.marginal_answers(image.contiguous(memory_format=torch.channels_last), programs, question_rows, log_weights))
        assert np.array_equal(nhwc["predictions"], from_tensor["predictions"])

        # one hypothesis per question: the network's own predictions
        with torch.no_grad():
            single = nmn(image, good[:6])["predictions"]
        out = nmn.marginal_answers(image, good[:6], np.arange(6))
        assert torch.equal(out["predictions"], single) and torch.equal(out["hypothesis_predictions"], single)
        assert out["support"].tolist() == [1] * 6 and out["hypothesis_weights"].tolist() == [1.0] * 6
        # no hypothesis at all
        out = nmn.marginal_answers(image, good[:0], np.zeros(0, np.int64))
        assert out["predictions"].tolist() == [unknown] * 6 and out["support"].tolist() == [0] * 6
        with pytest.raises(ValueError):
            nmn.marginal_answers(image, good[:2], np.array([1, 0]))
        with pytest.raises(ValueError):
            nmn.marginal_answers(image, good[:2], np.array([0, 6]))
    finally:
        nmn.train()


RECORD_KEYS = {"question_index", "answer", "answer_probability", "support", "hypotheses"}


def _check_records(records, n):
    assert len(records) == n and [r["question_index"] for r in records] == list(range(n))
    for r in records:
        assert set(r) == RECORD_KEYS and len(r["hypotheses"]) == r["support"]
        assert all(set(h) == {"program", "weight", "answer"} for h in r["hypotheses"])
        if r["support"]:
            assert sum(h["weight"] for h in r["hypotheses"]) == pytest.approx(1.0, abs=1e-5)
            assert 0.0 < r["answer_probability"] <= 1.0 + 1e-6 and r["answer"] != "@@UNKNOWN@@"
            assert len({tuple(h["program"]) for h in r["hypotheses"]}) == r["support"]  # merged: all distinct
        else:
            assert r["answer"] == "@@UNKNOWN@@" and r["answer_probability"] == 0.0


@pytest.mark.parametrize("constrained", [False, True])
def test_predict_answers_marginal_over_the_beam(models, constrained):
    from probnmn.evaluators import group_hypotheses, predict_answers

    vocab, pg, nmn, batch, dev = models
    batches = [{"question": batch["question"][s].to(dev), "image": batch["image"][s].to(dev)} for s in (slice(0, 4), slice(4, 8))]
    records = predict_answers(pg, nmn, batches, vocab, beam_size=4, marginal=True, constrained=constrained)
    _check_records(records, 8)
    assert pg.training and nmn.training
    if constrained:
        assert all(r["support"] >= 1 for r in records)
    # the records are what the kernel said for the beams of the same (deterministic) search
    pg.eval(), nmn.eval()
    try:
        k = 0
        for b in batches:
            extra = {}
            if constrained:
                exclude = [getattr(pg, n) for n in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
                extra["constraint"] = nmn.engine.compiler.decoding_automaton(exclude=exclude)
            with torch.no_grad():
                beams = pg(b["question"], decoding_strategy="beam", beam_size=4, **extra)
            tokens = beams["beam_predictions"].cpu().numpy()
            valid = np.array([c.valid for c in nmn.engine.compiler.compile_batch(tokens.reshape(16, -1))]).reshape(4, 4)
            programs, rows, weights, _ = group_hypotheses(tokens, beams["beam_log_probabilities"].cpu().numpy(), valid)
            out = nmn.marginal_answers(b["image"], torch.from_numpy(programs), rows, weights)
            for i in range(4):
                a, r = int(out["predictions"][i]), records[k]
                assert r["answer"] == vocab.get_token_from_index(a, namespace="answers")
                assert r["support"] == int(out["support"][i]) == int((rows == i).sum())
                if r["support"]:
                    assert r["answer_probability"] == pytest.approx(float(out["log_probabilities"][i, a].exp()), rel=1e-5)
                k += 1
    finally:
        pg.train(), nmn.train()


def test_predict_answers_from_sampled_programs(models):
    from probnmn.evaluators import evaluate_marginal_answer_accuracy, predict_answers

    vocab, pg, nmn, batch, dev = models
    batches = [{"question": batch["question"][s].to(dev), "image": batch["image"][s].to(dev), "answer": batch["answer"][s].to(dev)}
               for s in (slice(0, 4), slice(4, 8))]
    # default options: the records of before
    torch.manual_seed(2)
    assert all(set(r) == {"question_index", "answer"} for r in predict_answers(pg, nmn, batches, vocab))

    # an untrained generator, eight valid draws per question: the repeated rows drew independently
    torch.manual_seed(3)
    records = predict_answers(pg, nmn, batches, vocab, num_programs=8, constrained_sampling=True)
    _check_records(records, 8)
    assert all(1 <= r["support"] <= 8 for r in records) and max(r["support"] for r in records) > 1
    m = evaluate_marginal_answer_accuracy(pg, nmn, batches, vocab, beam_size=4, constrained=True)
    assert set(m) == {"answer_accuracy", "single_answer_accuracy", "average_support", "average_rows_per_question"}
    assert 1.0 <= m["average_support"] == m["average_rows_per_question"] <= 4.0 and 0.0 <= m["answer_accuracy"] <= 1.0

    # a generator that always draws the same program: one hypothesis of weight 1 per question, the single-program answer
    saved = _peaked(pg, vocab)
    try:
        torch.manual_seed(4)
        records = predict_answers(pg, nmn, batches, vocab, num_programs=8, constrained_sampling=True)
        _check_records(records, 8)
        single = predict_answers(pg, nmn, batches, vocab, constrained_sampling=True)
        for r, s in zip(records, single):
            assert r["support"] == 1 and r["hypotheses"][0]["weight"] == 1.0 and r["hypotheses"][0]["program"] == s["program"]
            assert r["answer"] == s["answer"] == r["hypotheses"][0]["answer"] and s["program_valid"]
        m = evaluate_marginal_answer_accuracy(pg, nmn, batches, vocab, num_programs=8, constrained_sampling=True)
        assert m["average_rows_per_question"] == 1.0 and m["average_support"] == 1.0
        assert m["answer_accuracy"] == m["single_answer_accuracy"]
        want = sum(r["answer"] == vocab.get_token_from_index(int(a), namespace="answers")
                   for r, a in zip(records, batch["answer"].tolist())) / 8
        assert m["answer_accuracy"] == want
    finally:
        with torch.no_grad():
            pg._output_projection_layer.bias.copy_(saved)
    assert pg.training and nmn.training
