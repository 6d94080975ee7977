"""``pnmn_hypothesis_posterior`` and what is built on it, on the MI355X: the kernel against the fp64 reference of
tests/helpers/hypothesis_posterior_reference.py over ragged groups, ties, the identities of a normalised posterior, bitwise
independence of a group from its batch, clamped group bounds; the scoring passes of the reconstructor and the prior against
their own ``forward`` losses, leaving the models untouched; ``predict_answers(rerank=True)`` and
``evaluate_marginal_answer_accuracy(rerank=True)``.

Tolerances.  ``log_px`` / ``log_pz``: rtol = atol = 1e-5, the project's bar for log-softmax quantities
(tests/test_hip_kernels.py::test_answer_loss): a sum of at most five terms (z[tok] - max) - log sum exp, each a few fp32 ulps
(6e-8 relative) of its own size, all of one sign.  ``log_posterior`` / ``log_evidence``: 1e-5 * (1 + the largest |score| among
the group's usable rows) -- the posterior is a DIFFERENCE of scores, so it inherits their absolute error, not their relative
one.  ``best_row`` is compared only where the reference's two best scores differ by 100 x that; the seeds below are those
at which, on the reference alone, that leaves out no supported group."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from hypothesis_posterior_reference import hypothesis_posterior_reference, top_two_score_margin  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)
GUARD = 64     # guard words on either side of every output buffer
TX, TZ = 5, 3
FIXED_SIZES = [0, 1, 2, 3, 16, 17, 64, 65, 5, 1, 0, 7]
DEAD_GROUP = 5  # (the 17 rows: the generator rules every one of them out)
WEIGHTS = (1.0, 0.75, 0.5)
# one seed per (Vx, Vz) at which, on the reference alone, the two best scores of every supported group differ by 100 x the
# group's tolerance, with WEIGHTS and -- but for (1, 1), see ``variants`` -- with (1, 1, 0) and no log_q (searched on the CPU
# with ``ragged_inputs`` and the reference; about one seed in two does, one in thirty at (3, 2), whose few distinct scores
# tie often).  The kernel variant follows the larger vocabulary: 257 and 513 are the first widths of the NPER 8 and 16 kernels
# (one live column in their register 4 and 8), 1024 the full width; of the seeds 0 .. 39, 16, 21 and 17 hold at those pairs,
# and the first of each is taken
SEEDS = {(1, 1): 0, (3, 2): 32, (64, 45): 1, (65, 64): 0, (130, 129): 1, (257, 256): 4, (513, 512): 0, (1024, 1023): 0}


def variants(V, log_q):
    """(weights, log_q) pairs a (Vx, Vz) case runs with.  One token per vocabulary makes every likelihood log 1 = 0: without
    log_q all scores tie exactly, which ``test_exact_ties_take_the_first_row`` covers."""
    return [(WEIGHTS, log_q)] + ([((1.0, 1.0, 0.0), None)] if min(V) > 1 else [])


def pad_of(V: int) -> int:
    return 0 if V > 1 else 7  # (a vocabulary of one token: its only token must not be the padding)


def ragged_inputs(Vx: int, Vz: int, seed: int):
    """37 groups: FIXED_SIZES and 25 groups of 1 .. 8 rows.  Returns x = (logits, tokens, pad), z likewise, log_q, start."""
    rng = np.random.default_rng(100000 * Vx + 100 * Vz + seed)
    sizes = np.array(FIXED_SIZES + rng.integers(1, 9, 25).tolist())
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    R = int(start[-1])

    def term(T, V):
        pad = pad_of(V)
        logits = (rng.standard_normal((R, T, V)) * 3).astype(np.float32)
        logits[rng.random(R) < 0.1] *= 8                       # rows far out in the exponent range
        tokens = rng.integers(0, V, (R, T)).astype(np.int64)
        tokens[rng.random((R, T)) < 0.25] = pad
        tokens[rng.random(R) < 0.06] = pad                     # rows that are all padding
        for r in np.nonzero(rng.random(R) < 0.05)[0]:          # a token that is no index: beyond the vocabulary, or negative
            tokens[r, rng.integers(0, T)] = V + 3 if r % 2 else -2
        if V > 1:
            for r in np.nonzero(rng.random(R) < 0.05)[0]:      # -inf at a scored target
                t = int(rng.integers(0, T))
                if tokens[r, t] != pad and 0 <= tokens[r, t] < V:
                    logits[r, t, tokens[r, t]] = -np.inf
        return logits, tokens, pad

    x, z = term(TX, Vx), term(TZ, Vz)
    log_q = (rng.standard_normal(R) * 4 - 20).astype(np.float32)
    log_q[rng.random(R) < 0.08] = -np.inf
    log_q[start[DEAD_GROUP]:start[DEAD_GROUP + 1]] = -np.inf
    return x, z, log_q, start


def launch(x, z, log_q, group_start, weights, optional=True, n_rows=None):
    """One ``pnmn_hypothesis_posterior`` launch on numpy inputs; every output lies between GUARD sentinel words, which must
    come back untouched.  The token rows are handed over with a stride wider than T.  Returns the outputs as numpy (rows no
    group covers keep the sentinel)."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    R = n_rows if n_rows is not None else next(len(a[0]) if isinstance(a, tuple) else len(a) for a in (x, z, log_q) if a is not None)
    G = len(group_start) - 1
    # (an input without rows is still an allocation: a null pointer means "not given")
    up = lambda t: (t if t.numel() else t.new_zeros(1)).to(dev)  # noqa: E731

    def term(t):
        if t is None:
            return None, (0, 0, 0), (1, 1, 0)
        logits, tokens, pad = t
        wide = torch.full((R, tokens.shape[1] + 2), 12345, dtype=torch.long)
        wide[:, :tokens.shape[1]] = torch.from_numpy(np.ascontiguousarray(tokens))
        d_logits, d_tokens = up(torch.from_numpy(np.ascontiguousarray(logits, np.float32))), up(wide)
        return (d_logits, d_tokens), (d_logits.data_ptr(), d_tokens.data_ptr(), wide.stride(0)), (logits.shape[1], logits.shape[2], pad)

    keep_x, x_args, (Tx, Vx, pad_x) = term(x)
    keep_z, z_args, (Tz, Vz, pad_z) = term(z)
    d_q = None if log_q is None else up(torch.from_numpy(np.ascontiguousarray(log_q, np.float32)))
    d_start = torch.from_numpy(np.asarray(group_start, np.int64)).to(torch.int32).to(dev)
    bufs = {"log_px": torch.full((R + 2 * GUARD,), -777.0, dtype=torch.float32, device=dev),
            "log_pz": torch.full((R + 2 * GUARD,), -777.0, dtype=torch.float32, device=dev),
            "log_posterior": torch.full((R + 2 * GUARD,), -777.0, dtype=torch.float32, device=dev),
            "log_evidence": torch.full((G + 2 * GUARD,), -777.0, dtype=torch.float32, device=dev),
            "best_row": torch.full((G + 2 * GUARD,), -777, dtype=torch.int32, device=dev),
            "support": torch.full((G + 2 * GUARD,), -777, dtype=torch.int32, device=dev)}
    ptr = lambda name: bufs[name][GUARD:].data_ptr()  # noqa: E731
    opt = lambda name: ptr(name) if optional else 0  # noqa: E731
    rc = _hip.lib().pnmn_hypothesis_posterior(
        *x_args, *z_args, 0 if d_q is None else d_q.data_ptr(), d_start.data_ptr(), *(float(w) for w in weights), pad_x, pad_z,
        opt("log_px"), opt("log_pz"), ptr("log_posterior"), ptr("log_evidence"), ptr("best_row"), opt("support"),
        G, R, Tx, Vx, Tz, Vz, _hip.stream_ptr(dev))
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
    per_group, per_row = row_tolerance(ref, start)
    for name in ("log_px", "log_pz"):
        if ref[name] is None:
            assert (got[name] == -777).all(), name  # (a term that is not given is not written)
            continue
        inf = np.isneginf(ref[name])
        assert np.array_equal(np.isneginf(got[name]), inf) and not np.isnan(ref[name]).any(), name
        np.testing.assert_allclose(got[name][~inf], ref[name][~inf], err_msg=name, **TOL)
    usable = ref["usable"]
    assert np.array_equal(np.isfinite(got["log_posterior"]), usable)  # usability, exactly
    assert np.isneginf(got["log_posterior"][~usable]).all()           # (every row is covered here)
    assert np.array_equal(got["support"], ref["support"])
    assert (np.abs(got["log_posterior"][usable] - ref["log_posterior"][usable]) <= per_row[usable]).all()
    supported = ref["support"] > 0
    assert np.isneginf(got["log_evidence"][~supported]).all() and (got["best_row"][~supported] == -1).all()
    assert (np.abs(got["log_evidence"][supported] - ref["log_evidence"][supported]) <= per_group[supported]).all()
    assert (usable[got["best_row"][supported]]).all()
    if best:  # the MAP row is the reference's, the margin being what the caller asserted ...
        assert np.array_equal(got["best_row"], ref["best_row"])
        for g in np.nonzero(supported)[0]:  # ... and the first row with the largest posterior the device itself wrote
            lp = got["log_posterior"][start[g]:start[g + 1]]
            assert got["best_row"][g] == start[g] + int(np.argmax(lp == lp.max())), g


@pytest.mark.parametrize("V", sorted(SEEDS))
def test_kernel_against_fp64_reference(V):
    x, z, log_q, start = ragged_inputs(*V, SEEDS[V])
    assert len(start) - 1 == 37 and (np.diff(start)[:12] == FIXED_SIZES).all()
    # what the inputs are required to hold
    for logits, tokens, pad in (x, z):
        assert (tokens == pad).all(1).any() and ((tokens != pad) & ((tokens < 0) | (tokens >= logits.shape[2]))).any()
        assert logits.shape[2] == 1 or np.isneginf(logits).any()
    assert np.isneginf(log_q).any()
    for weights, q in variants(V, log_q):
        ref = hypothesis_posterior_reference(x, z, q, start, weights)
        per_group, _ = row_tolerance(ref, start)
        margin = top_two_score_margin(ref["score"], ref["usable"], start)
        print("V = %s, weights %s: smallest top-two margin / (100 x tolerance) %.3g over %d supported groups"
              % (V, weights, (margin / (100 * per_group)).min(), int((ref["support"] > 0).sum())))
        assert (margin >= 100 * per_group).all()  # (of the reference alone: no group is left out of the comparison below)
        assert ref["support"][0] == 0 and (ref["support"] > 0).sum() >= 30
        if q is not None:
            assert ref["support"][DEAD_GROUP] == 0
        got = launch(x, z, q, start, weights)
        usable = ref["usable"]
        _, per_row = row_tolerance(ref, start)
        print("    largest |log_posterior - reference| / tolerance: %.3g"
              % (np.abs(got["log_posterior"][usable] - ref["log_posterior"][usable]) / per_row[usable]).max())
        check_against_reference(got, ref, start)
        # the optional outputs left out: the required ones are the same bits
        bare = launch(x, z, q, start, weights, optional=False)
        for name in ("log_posterior", "log_evidence", "best_row"):
            assert np.array_equal(bits(bare[name]), bits(got[name])), name
        for name in ("log_px", "log_pz", "support"):
            assert (bare[name] == -777).all(), name


def test_exact_ties_take_the_first_row():
    rng = np.random.default_rng(5)
    V = 45
    for size, first, second in ((9, 2, 5), (70, 3, 67), (70, 66, 7), (130, 64, 128)):
        logits = (rng.standard_normal((size, TZ, V)) * 2).astype(np.float32)
        tokens = rng.integers(1, V, (size, TZ)).astype(np.int64)
        log_q = (rng.standard_normal(size) - 30).astype(np.float32)
        lo, hi = min(first, second), max(first, second)
        logits[hi], tokens[hi] = logits[lo], tokens[lo]   # the same row twice (in different waves), on top of the group
        log_q[hi] = log_q[lo] = 5.0
        got = launch(None, (logits, tokens, 0), log_q, [0, size], (0.0, 1.0, 1.0))
        lp = got["log_posterior"]
        assert lp[lo] == lp[hi] == lp.max() and got["log_pz"][lo] == got["log_pz"][hi]
        assert got["best_row"][0] == lo and got["support"][0] == size and (got["log_px"] == -777).all()
    # one token per vocabulary and no log_q: every usable row scores log 1 = 0, so each group's first usable row leads
    x, z, _, start = ragged_inputs(1, 1, SEEDS[(1, 1)])
    ref = hypothesis_posterior_reference(x, z, None, start, (1.0, 1.0, 0.0))
    assert (ref["score"][ref["usable"]] == 0).all() and (ref["support"] > 1).sum() >= 20 and not ref["usable"].all()
    got = launch(x, z, None, start, (1.0, 1.0, 0.0))
    check_against_reference(got, ref, start)


def test_identities_of_a_normalised_posterior():
    x, z, log_q, start = ragged_inputs(64, 45, 3)
    R, G = len(log_q), len(start) - 1
    # weights (0, 0, 1): log_softmax(log_q) over each group's rows with a finite log_q -- and the terms are still reported
    only_q = launch(x, z, log_q, start, (0.0, 0.0, 1.0))
    full = launch(x, z, log_q, start, WEIGHTS)
    for name in ("log_px", "log_pz"):
        assert np.array_equal(bits(only_q[name]), bits(full[name])), name
    for g in range(G):
        rows = np.arange(start[g], start[g + 1])
        rows = rows[np.isfinite(log_q[rows])]
        assert only_q["support"][g] == rows.size
        if rows.size:
            lq = log_q[rows].astype(np.float64)
            want = lq - lq.max() - np.log(np.exp(lq - lq.max()).sum())
            np.testing.assert_allclose(only_q["log_posterior"][rows], want, rtol=0, atol=1e-5 * (1 + np.abs(lq).max()))
    # a constant added to a group's log_q changes nothing but the evidence
    ref = hypothesis_posterior_reference(x, z, log_q, start, WEIGHTS)
    per_group, per_row = row_tolerance(ref, start)
    shifted = log_q.copy()
    shifted[start[7]:start[8]] += 7.5
    shifted[start[20]:] -= 3.25
    moved = launch(x, z, shifted, start, WEIGHTS)
    usable = ref["usable"]
    assert np.array_equal(np.isfinite(moved["log_posterior"]), usable)
    assert (np.abs(moved["log_posterior"][usable] - full["log_posterior"][usable]) <= 2 * per_row[usable]).all()
    assert np.array_equal(moved["best_row"], full["best_row"]) and np.array_equal(moved["support"], full["support"])
    assert abs(moved["log_evidence"][7] - full["log_evidence"][7] - 7.5 * WEIGHTS[2]) <= 2 * per_group[7]
    # a null term equals a zero coefficient, bit for bit
    for weights, null in (((0.0, 0.75, 0.5), (None, z, log_q)), ((1.0, 0.0, 0.5), (x, None, log_q)), ((1.0, 0.75, 0.0), (x, z, None)),
                          ((0.0, 0.0, 1.0), (None, None, log_q)), ((0.0, 1.0, 0.0), (None, z, None))):
        zero = launch(x, z, log_q, start, weights)
        gone = launch(*null, start, weights, n_rows=R)
        for name in ("log_posterior", "log_evidence", "best_row", "support"):
            assert np.array_equal(bits(zero[name]), bits(gone[name])), (weights, name)
        check_against_reference(zero, hypothesis_posterior_reference(x, z, log_q, start, weights), start, best=False)
    # a row that a dropped term alone ruled out counts again
    dropped = hypothesis_posterior_reference(x, z, log_q, start, (0.0, 0.75, 0.5))
    assert (dropped["usable"] & ~ref["usable"]).any()


def test_a_group_is_the_same_bits_alone_and_in_a_batch():
    V = (65, 64)
    x, z, log_q, start = ragged_inputs(*V, SEEDS[V])
    whole = launch(x, z, log_q, start, WEIGHTS)
    again = launch(x, z, log_q, start, WEIGHTS)
    for name in whole:
        assert np.array_equal(bits(whole[name]), bits(again[name])), name
    for g in (0, 3, 4, DEAD_GROUP, 6, 7, 11, 20, 36):
        lo, hi = int(start[g]), int(start[g + 1])
        cut = lambda t: (t[0][lo:hi], t[1][lo:hi], t[2])  # noqa: E731
        alone = launch(cut(x), cut(z), log_q[lo:hi], [0, hi - lo], WEIGHTS, n_rows=hi - lo)
        for name in ("log_px", "log_pz", "log_posterior"):
            assert np.array_equal(bits(alone[name]), bits(whole[name][lo:hi])), (g, name)
        assert bits(alone["log_evidence"])[0] == bits(whole["log_evidence"])[g] and alone["support"][0] == whole["support"][g]
        assert alone["best_row"][0] == (whole["best_row"][g] - lo if whole["best_row"][g] >= 0 else -1)


def test_group_bounds_are_clamped_into_the_arrays():
    """Correct launches of the kernel with a ``group_start`` that a caller got wrong: every bound is clamped into
    [0, n_rows] with end >= start, so nothing outside the arrays is read or written (``launch`` checks the guard words) and
    the groups that share no row with another give the same bits."""
    V = (3, 2)
    x, z, log_q, start = ragged_inputs(*V, SEEDS[V])
    R = int(start[-1])
    base = launch(x, z, log_q, start, WEIGHTS)

    # a last entry beyond n_rows and a first one below 0 clamp to what they should have been: nothing changes
    for last in (R + 1000, 2 ** 31 - 1):
        bad = start.astype(np.int64)
        bad[-1], bad[0] = last, -5
        got = launch(x, z, log_q, bad, WEIGHTS)
        for name in base:
            assert np.array_equal(bits(got[name]), bits(base[name])), (last, name)

    # every bound out of range on the same side: no group has a row, nothing but the group outputs is written
    for bad in (np.full(38, -9), np.full(38, R + 7)):
        got = launch(x, z, log_q, bad, WEIGHTS)
        assert (got["support"] == 0).all() and (got["best_row"] == -1).all() and np.isneginf(got["log_evidence"]).all()
        assert all((got[name] == -777).all() for name in ("log_px", "log_pz", "log_posterior"))

    # a decreasing pair: start[4] = 30 > start[5] = 22.  Group 3 becomes rows [3, 30), group 4 is empty; groups 3 and 5 now
    # share rows 22 .. 29, whose posterior either may write: every OTHER group keeps its bits, and the likelihood terms of
    # every row (its own, whoever writes them) stay what they were
    assert start[3] == 3 and start[4] == 6 and start[5] == 22
    bad = start.copy()
    bad[4] = 30
    got = launch(x, z, log_q, bad, WEIGHTS)
    others = np.array([g for g in range(37) if g not in (3, 4, 5)])
    for name in ("log_evidence", "best_row", "support"):
        assert np.array_equal(bits(got[name])[others], bits(base[name])[others]), name
    assert got["support"][4] == 0 and got["best_row"][4] == -1 and np.isneginf(got["log_evidence"][4])
    outside = np.r_[0:3, int(start[6]):R]
    assert np.array_equal(bits(got["log_posterior"])[outside], bits(base["log_posterior"])[outside])
    for name in ("log_px", "log_pz"):
        assert np.array_equal(bits(got[name]), bits(base[name])), name


def test_a_wider_vocabulary_than_the_widest_kernel_holds_returns_without_a_launch():
    from probnmn import _hip

    dev = torch.device("cuda:0")
    out = torch.full((2 * 3 * 1025,), -777.0, device=dev)
    p = out.data_ptr()
    # (one group of two rows of three steps: every buffer the kernel would touch lies inside ``out``)
    for Vx, Vz in ((1025, 4), (4, 1025)):
        assert _hip.lib().pnmn_hypothesis_posterior(p, p, 3, p, p, 3, 0, p, 1.0, 1.0, 0.0, 0, 0, 0, 0, p, p, p, 0, 1, 2, 3, Vx, 3, Vz,
                                                    _hip.stream_ptr(dev)) == _hip.ESHAPE
    torch.cuda.synchronize()
    assert (out == -777).all()  # nothing ran


# ---- the models and the evaluators -------------------------------------------------------------------------------------

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


def _own_losses(qr, prior, programs, questions):
    """log p(x | z) and log p(z) of each row from the models' own evaluation-mode ``forward``: per-token loss x scored tokens
    (the tokens that are not padding, and the @end@ behind them), in fp64."""
    was = qr.training, prior.training
    qr.eval(), prior.eval()
    try:
        with torch.no_grad():
            loss_x = qr(programs, questions)["loss"].double().cpu().numpy()
            loss_z = prior(programs)["loss"].double().cpu().numpy()
    finally:
        qr.train(was[0]), prior.train(was[1])
    n_x = (questions != 0).sum(1).cpu().numpy() + 1
    n_z = (programs != 0).sum(1).cpu().numpy() + 1
    return loss_x, n_x, loss_z, n_z


def test_scoring_passes_match_the_models_and_leave_them_untouched(models):
    from probnmn.evaluators import hypothesis_posterior

    vocab, pg, nmn, qr, prior, batch, dev = models
    assert qr._pad_index == prior._pad_index == 0
    question_rows = np.array([0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 6, 7])
    programs = batch["program"][[0, 1, 1, 2, 3, 4, 5, 5, 6, 7, 0, 3]].to(dev)
    questions = batch["question"].to(dev)
    log_q = np.linspace(-3.0, -0.5, 12).astype(np.float32)
    asked = questions[torch.from_numpy(question_rows).to(dev)]

    # metrics on record in both models, from evaluation passes of their own
    loss_x, n_x, loss_z, n_z = _own_losses(qr, prior, programs, asked)
    qr.eval(), prior.eval()
    qr.get_metrics(reset=False)  # (reading the metrics starts BLEU afresh whatever ``reset`` says, as the reference has it)
    before = (qr.get_metrics(reset=False), prior.get_metrics(reset=False))
    counts = (qr._log2_perplexity._count, qr._sequence_accuracy._count, prior._log2_perplexity._count)
    assert counts[0] > 0 and counts[2] > 0
    qr.train()                                                              # one model in each mode
    torch.manual_seed(11)
    state = torch.get_rng_state()

    out = hypothesis_posterior(qr, prior, questions, programs, question_rows, log_q=log_q, weights=(1.0, 1.0, 0.25))
    in_passes = hypothesis_posterior(qr, prior, questions, programs.cpu(), question_rows, log_q=log_q, weights=(1.0, 1.0, 0.25),
                                     max_rows=5)
    got = {k: v.cpu().numpy() for k, v in out.items()}

    assert torch.equal(torch.get_rng_state(), state)                        # no seed was drawn
    assert qr.training and not prior.training                               # the flags are back
    qr.eval()
    assert (qr.get_metrics(reset=False), prior.get_metrics(reset=False)) == before
    assert (qr._log2_perplexity._count, qr._sequence_accuracy._count, prior._log2_perplexity._count) == counts
    assert qr._bleu._reference_length == 0 and not qr._bleu._pending       # nothing reached BLEU since it started afresh
    qr.train()

    # the sums are the models' own per-token losses times the scored tokens
    np.testing.assert_allclose(-got["log_reconstruction"] / n_x, loss_x, **TOL)
    np.testing.assert_allclose(-got["log_prior"] / n_z, loss_z, **TOL)
    score = -(loss_x * n_x) - (loss_z * n_z) + 0.25 * log_q
    for g in range(8):
        rows = np.nonzero(question_rows == g)[0]
        s = score[rows]
        tol = 1e-5 * (1 + np.abs(s).max())
        assert got["support"][g] == rows.size
        assert abs(got["log_evidence"][g] - (s.max() + np.log(np.exp(s - s.max()).sum()))) <= tol
        assert (np.abs(got["log_posterior"][rows] - (s - s.max() - np.log(np.exp(s - s.max()).sum()))) <= tol).all()
        if rows.size == 1 or np.sort(s)[-1] - np.sort(s)[-2] >= 100 * tol:
            assert got["best_row"][g] == rows[int(s.argmax())]
    # passes of five rows: a row does not depend on its pass (to the rounding of the library GEMMs, which see other shapes)
    again = {k: v.cpu().numpy() for k, v in in_passes.items()}
    for name in ("log_reconstruction", "log_prior"):
        np.testing.assert_allclose(again[name], got[name], err_msg=name, **TOL)
    worst = 1e-5 * (1 + np.abs(score).max())
    assert (np.abs(again["log_posterior"] - got["log_posterior"]) <= worst).all()
    assert (np.abs(again["log_evidence"] - got["log_evidence"]) <= worst).all() and np.array_equal(again["support"], got["support"])

    # one model alone; no hypothesis at all
    only = hypothesis_posterior(None, prior, questions, programs, question_rows, weights=(0.0, 1.0, 0.0))
    assert torch.isnan(only["log_reconstruction"]).all()
    np.testing.assert_allclose(only["log_prior"].cpu().numpy(), got["log_prior"], **TOL)
    none = hypothesis_posterior(qr, prior, questions, programs[:0], np.zeros(0, np.int64))
    assert none["support"].tolist() == [0] * 8 and none["best_row"].tolist() == [-1] * 8
    assert torch.isneginf(none["log_evidence"]).all() and none["log_posterior"].shape == (0,)
    with pytest.raises(ValueError):
        hypothesis_posterior(qr, prior, questions, programs[:2], np.array([1, 0]))
    with pytest.raises(ValueError):
        hypothesis_posterior(qr, prior, questions, programs[:2], np.array([0, 8]))
    prior.train()


RERANKED_KEYS = {"question_index", "answer", "answer_probability", "support", "hypotheses", "map_program", "map_answer"}


def _batches(batch, dev, answers=False):
    keys = ("question", "image") + (("answer",) if answers else ())
    return [{k: batch[k][s].to(dev) for k in keys} for s in (slice(0, 4), slice(4, 8))]


def test_predict_answers_reranked_by_the_generator_alone_is_the_marginal_answer(models):
    from probnmn.evaluators import predict_answers

    vocab, pg, nmn, qr, prior, batch, dev = models
    batches = _batches(batch, dev)
    plain = predict_answers(pg, nmn, batches, vocab, beam_size=4, marginal=True, constrained=True)
    assert all(set(r) == RERANKED_KEYS - {"map_program", "map_answer"} for r in plain)  # (rerank=False: today's records)
    for given in ((qr, prior), (None, None)):
        reranked = predict_answers(pg, nmn, batches, vocab, beam_size=4, constrained=True, rerank=True,
                                   question_reconstructor=given[0], program_prior=given[1], rerank_weights=(0, 0, 1))
        assert len(reranked) == len(plain) == 8
        for r, p in zip(reranked, plain):
            assert set(r) == RERANKED_KEYS and r["support"] == p["support"] >= 1
            assert [h["program"] for h in r["hypotheses"]] == [h["program"] for h in p["hypotheses"]]
            np.testing.assert_allclose([h["weight"] for h in r["hypotheses"]], [h["weight"] for h in p["hypotheses"]], **TOL)
            assert r["answer_probability"] == pytest.approx(p["answer_probability"], rel=1e-5, abs=1e-5)
            # (the same answer, unless two answers are tied within the tolerance)
            assert r["answer"] == p["answer"] or abs(r["answer_probability"] - p["answer_probability"]) <= 1e-5
            assert all((h["log_prior"] is None) == (given[1] is None) and (h["log_reconstruction"] is None) == (given[0] is None)
                       for h in r["hypotheses"])
    assert pg.training and nmn.training and qr.training and prior.training


def test_predict_answers_reranked_by_the_generative_model(models):
    from probnmn.evaluators import evaluate_marginal_answer_accuracy, group_hypotheses, predict_answers

    vocab, pg, nmn, qr, prior, batch, dev = models
    batches = _batches(batch, dev, answers=True)
    records = predict_answers(pg, nmn, batches, vocab, beam_size=4, constrained=True, rerank=True, question_reconstructor=qr,
                              program_prior=prior)
    assert len(records) == 8 and [r["question_index"] for r in records] == list(range(8))
    exclude = [getattr(pg, n) for n in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
    constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)
    k = 0
    several = 0
    for b in batches:
        pg.eval()
        with torch.no_grad():
            beams = pg(b["question"], decoding_strategy="beam", beam_size=4, constraint=constraint)
        pg.train()
        tokens = beams["beam_predictions"].cpu().numpy()
        valid = np.array([c.valid for c in nmn.engine.compiler.compile_batch(tokens.reshape(16, -1))]).reshape(4, 4)
        programs, rows, _, _ = group_hypotheses(tokens, beams["beam_log_probabilities"].cpu().numpy(), valid)
        on_dev = torch.from_numpy(programs).to(dev)
        loss_x, n_x, loss_z, n_z = _own_losses(qr, prior, on_dev, b["question"][torch.from_numpy(rows).to(dev)])
        score = -(loss_x * n_x) - (loss_z * n_z)
        for i in range(4):
            r = records[k]
            k += 1
            mine = np.nonzero(rows == i)[0]
            assert set(r) == RERANKED_KEYS and r["support"] == mine.size == len(r["hypotheses"]) >= 1
            s = score[mine]
            tol = 1e-5 * (1 + np.abs(s).max())
            want = np.exp(s - s.max() - np.log(np.exp(s - s.max()).sum()))  # the reference posterior, from the models' own losses
            weights = np.array([h["weight"] for h in r["hypotheses"]])
            assert (np.abs(weights - want) <= tol).all(), (weights, want)
            np.testing.assert_allclose([-h["log_reconstruction"] for h in r["hypotheses"]] / n_x[mine], loss_x[mine], **TOL)
            np.testing.assert_allclose([-h["log_prior"] for h in r["hypotheses"]] / n_z[mine], loss_z[mine], **TOL)
            # the MAP hypothesis is the heaviest one, and ``map_answer`` its own answer
            heaviest = [h for h in r["hypotheses"] if h["weight"] == weights.max()]
            assert any(r["map_program"] == h["program"] and r["map_answer"] == h["answer"] for h in heaviest)
            assert 0.0 < r["answer_probability"] <= 1.0 + 1e-6 and sum(weights) == pytest.approx(1.0, abs=1e-5)
            several += mine.size > 1
    assert several >= 4  # (the posterior had something to rerank)

    m = evaluate_marginal_answer_accuracy(pg, nmn, batches, vocab, beam_size=4, constrained=True, rerank=True,
                                          question_reconstructor=qr, program_prior=prior)
    assert set(m) == {"answer_accuracy", "single_answer_accuracy", "average_support", "average_rows_per_question", "map_answer_accuracy"}
    assert 0.0 <= m["map_answer_accuracy"] <= 1.0 and 0.0 <= m["answer_accuracy"] <= 1.0 and 1.0 <= m["average_support"] <= 4.0
    want = sum(r["map_answer"] == vocab.get_token_from_index(int(a), namespace="answers")
               for r, a in zip(records, batch["answer"].tolist())) / 8
    assert m["map_answer_accuracy"] == want
    plain = evaluate_marginal_answer_accuracy(pg, nmn, batches, vocab, beam_size=4, constrained=True)
    assert "map_answer_accuracy" not in plain and plain["single_answer_accuracy"] == m["single_answer_accuracy"]
    assert pg.training and nmn.training and qr.training and prior.training
