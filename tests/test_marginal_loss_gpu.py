"""Marginal-likelihood module training on the MI355X: ``pnmn_answer_posterior`` in gradient mode (no ``best_row``; ``d_logits``
in ``log_answer``'s place) against the fp64 reference of tests/helpers/marginal_loss_reference.py over the ragged groups of
the posterior tests, its shared outputs bit for bit against a plain launch, bitwise independence of a group from its batch,
clamped group bounds, the argument checks, K = 1 against ``pnmn_answer_loss``; the autograd node; then
``NeuralModuleNetwork.marginal_answer_loss`` and ``ModuleTrainingStep(objective="marginal")`` on a tiny network.

Tolerance of ``d_logits``: |w_a| * 2e-5 * (1 + the largest |score| among the group's usable rows).  d_logits is w_a * share *
(softmax - onehot): the share exp(log_posterior) inherits ``log_posterior``'s absolute bar 1e-5 * (1 + max |score|) as a
relative error, the softmax factor inherits the log-softmax bar 1e-5 the same way, and both factors are at most 1 in size.
Zeros (rows that do not count) and the signs of a row's entries are compared exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from answer_posterior_cases import ANSWERS, BEYOND_GROUP, DEAD_GROUP, NEGATIVE_GROUP, SEEDS, ragged_inputs  # noqa: E402
from marginal_loss_reference import marginal_loss_reference  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64     # guard words on either side of every output buffer
SHARED = ("log_posterior", "log_evidence", "row_predictions", "support", "consistent_count", "first_consistent")
ROW_OUTPUTS = ("d_logits", "row_predictions", "log_posterior")
GROUP_OUTPUTS = ("log_evidence", "support", "consistent_count", "first_consistent")
INVALID_PROGRAM_LOSS = np.float32(3.33)


def launch(logits, valid, log_weight, answers, group_start, w_a, unknown, grad=True):
    """One ``pnmn_answer_posterior`` launch on numpy inputs, in gradient mode (``d_logits`` [R, A] where a plain launch has
    ``log_answer``, no ``best_row``) or plain; every output lies between GUARD sentinel words, which must come back untouched.
    Returns the outputs as numpy (what no group covers keeps the sentinel)."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    R, A = logits.shape
    G = len(group_start) - 1
    up = lambda a, dt: None if a is None else (torch.from_numpy(np.ascontiguousarray(a)).to(dt) if len(a) else torch.zeros(1, dtype=dt)).to(dev)  # noqa: E731
    d_in, d_valid, d_lw = up(logits, torch.float32), up(valid, torch.int32), up(log_weight, torch.float32)
    d_answers = up(np.asarray(answers, np.int64), torch.long)
    d_start = up(np.asarray(group_start, np.int64), torch.int32)
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    bufs = {"d_logits" if grad else "log_answer": torch.full(((R * A if grad else R) + 2 * GUARD,), -777.0, **f),
            "row_predictions": torch.full((R + 2 * GUARD,), -777, dtype=torch.long, device=dev),
            "log_posterior": torch.full((R + 2 * GUARD,), -777.0, **f), "log_evidence": torch.full((G + 2 * GUARD,), -777.0, **f),
            "support": torch.full((G + 2 * GUARD,), -777, **i), "consistent_count": torch.full((G + 2 * GUARD,), -777, **i),
            "first_consistent": torch.full((G + 2 * GUARD,), -777, **i)}
    if not grad:
        bufs["best_row"] = torch.full((G + 2 * GUARD,), -777, **i)
    ptr = lambda name: bufs[name][GUARD:].data_ptr()  # noqa: E731
    rc = _hip.lib().pnmn_answer_posterior(
        d_in.data_ptr(), 0 if d_valid is None else d_valid.data_ptr(), 0 if d_lw is None else d_lw.data_ptr(),
        d_answers.data_ptr(), d_start.data_ptr(), float(w_a), ptr("d_logits" if grad else "log_answer"), ptr("row_predictions"),
        ptr("log_posterior"), ptr("log_evidence"), 0 if grad else ptr("best_row"), ptr("support"), ptr("consistent_count"),
        ptr("first_consistent"), G, R, A, unknown, _hip.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == -777).all() and (host[-GUARD:] == -777).all(), name
        out[name] = host[GUARD:-GUARD]
    if grad:
        out["d_logits"] = out["d_logits"].reshape(R, A)
    return out


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def row_bars(ref, start, w_a):
    """|w_a| * 2e-5 * (1 + largest |score| of the group), spread over the group's rows."""
    per_row = np.zeros(ref["score"].size)
    for g in range(len(start) - 1):
        per_row[start[g]:start[g + 1]] = abs(w_a) * 2e-5 * (1.0 + ref["max_abs_score"][g])
    return per_row


def check_gradient(got, ref, answers, start, w_a, A):
    """``d_logits`` of a launch whose groups cover every row, against the reference; returns the largest error / bar."""
    d, usable = got["d_logits"], ref["usable"]
    bar = row_bars(ref, start, w_a)
    assert not np.isnan(d).any() and (d[~usable] == 0).all()  # rows that do not count: zeros, exactly
    group_of = np.repeat(np.arange(len(start) - 1), np.diff(start))
    target = np.zeros_like(d, dtype=bool)
    known = usable & (answers[group_of] >= 0) & (answers[group_of] < A)
    assert np.array_equal(known, usable) or w_a == 0  # (an answer that is no index leaves no usable row)
    target[np.nonzero(known)[0], answers[group_of][known]] = True
    assert (d[target] <= 0).all() and (d[usable][~target[usable]] >= 0).all()  # the answer pulls down, the others up: exactly
    assert (np.abs(d[usable].astype(np.float64).sum(1)) <= bar[usable]).all()  # a usable row sums to 0
    err = np.abs(d.astype(np.float64) - ref["d_logits"]) / np.maximum(bar, 1e-300)[:, None]
    worst = float(err[usable].max()) if usable.any() else 0.0
    assert worst <= 1.0, worst
    return worst


@pytest.mark.parametrize("A", ANSWERS)
def test_gradient_kernel_against_fp64_reference(A):
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    for lw in (log_weight, None):
        for w_a in (1.0, 0.5):
            ref = marginal_loss_reference(logits, valid, lw, answers, start, w_a, A)
            assert (ref["support"] > 0).sum() >= 28 and not ref["usable"].all() and ref["covered"].all()
            got = launch(logits, valid, lw, answers, start, w_a, A)
            worst = check_gradient(got, ref, answers, start, w_a, A)
            print("A = %d, w_a %s, weights %s: largest |d_logits - reference| / bar %.3g over %d usable rows"
                  % (A, w_a, "given" if lw is not None else "null", worst, int(ref["usable"].sum())))
            # the loss itself, and every output the two modes share: the bits of a plain launch on the same inputs
            sup = ref["support"] > 0
            assert (np.abs(got["log_evidence"][sup] - ref["log_evidence"][sup]) <= 1e-5 * (1 + ref["max_abs_score"][sup])).all()
            assert np.isneginf(got["log_evidence"][~sup]).all() and np.array_equal(got["support"], ref["support"])
            plain = launch(logits, valid, lw, answers, start, w_a, A, grad=False)
            for name in SHARED:
                assert np.array_equal(bits(got[name]), bits(plain[name])), name
    # w_a == 0: every written value is 0 -- and every row is written
    got = launch(logits, valid, log_weight, answers, start, 0.0, A)
    assert (got["d_logits"] == 0).all() and (got["support"] > 0).sum() >= 28
    plain = launch(logits, valid, log_weight, answers, start, 0.0, A, grad=False)
    for name in SHARED:
        assert np.array_equal(bits(got[name]), bits(plain[name])), name


def test_a_groups_gradient_is_the_same_bits_alone_and_in_a_batch():
    A = 65
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    whole = launch(logits, valid, log_weight, answers, start, 0.5, A)
    again = launch(logits, valid, log_weight, answers, start, 0.5, A)
    for name in whole:
        assert np.array_equal(bits(whole[name]), bits(again[name])), name
    assert (whole["d_logits"] != 0).any()
    for g in (0, 3, 4, DEAD_GROUP, 6, 7, BEYOND_GROUP, NEGATIVE_GROUP, 20, 36):
        lo, hi = int(start[g]), int(start[g + 1])
        alone = launch(logits[lo:hi], valid[lo:hi], log_weight[lo:hi], answers[g:g + 1], [0, hi - lo], 0.5, A)
        for name in ROW_OUTPUTS:
            assert np.array_equal(bits(alone[name]), bits(whole[name][lo:hi])), (g, name)
        for name in ("log_evidence", "support", "consistent_count"):
            assert bits(alone[name])[0] == bits(whole[name])[g], (g, name)


def test_group_bounds_are_clamped_into_the_arrays():
    """The three malformed ``group_start`` cases of the posterior test, in gradient mode: nothing outside the arrays is read
    or written (``launch`` checks the guard words around d_logits too) and the groups that share no row with another keep
    their bits."""
    A = 28
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    R = int(start[-1])
    base = launch(logits, valid, log_weight, answers, start, 1.0, A)

    for last in (R + 1000, 2 ** 31 - 1):
        bad = start.astype(np.int64)
        bad[-1], bad[0] = last, -5
        got = launch(logits, valid, log_weight, answers, bad, 1.0, A)
        for name in base:
            assert np.array_equal(bits(got[name]), bits(base[name])), (last, name)

    for bad in (np.full(38, -9), np.full(38, R + 7)):
        got = launch(logits, valid, log_weight, answers, bad, 1.0, A)
        assert (got["support"] == 0).all() and np.isneginf(got["log_evidence"]).all()
        assert all((got[name] == -777).all() for name in ROW_OUTPUTS)  # no group has a row: no row is written

    assert start[3] == 3 and start[4] == 6 and start[5] == 22
    bad = start.copy()
    bad[4] = 30   # groups 3 and 5 now share rows 22 .. 29, group 4 is empty: every OTHER group keeps its bits
    got = launch(logits, valid, log_weight, answers, bad, 1.0, A)
    others = np.array([g for g in range(37) if g not in (3, 4, 5)])
    for name in GROUP_OUTPUTS:
        assert np.array_equal(bits(got[name])[others], bits(base[name])[others]), name
    assert got["support"][4] == 0 and np.isneginf(got["log_evidence"][4])
    outside = np.r_[0:3, int(start[6]):R]
    for name in ROW_OUTPUTS:
        assert np.array_equal(bits(got[name])[outside], bits(base[name])[outside]), name
    assert not np.isnan(got["d_logits"]).any() and (got["d_logits"] != -777).all()  # every row is covered, whoever wrote it


def test_argument_errors_return_without_a_launch():
    from probnmn import _hip

    dev = torch.device("cuda:0")
    fn = _hip.lib().pnmn_answer_posterior
    out = torch.full((64,), -777.0, device=dev)
    p = out.data_ptr()

    def call(logits=p, answers=p, group_start=p, w_a=1.0, d_logits=p, log_posterior=p, log_evidence=p, n_groups=1, n_rows=2, A=4):
        return fn(logits, 0, 0, answers, group_start, w_a, d_logits, 0, log_posterior, log_evidence, 0, 0, 0, 0, n_groups, n_rows, A, 0,
                  _hip.stream_ptr(dev))

    for missing in ("group_start", "answers", "log_posterior", "log_evidence", "logits", "d_logits"):
        assert call(**{missing: 0}) == _hip.EINVAL, missing
    assert call(n_rows=-1) == _hip.EINVAL and call(n_groups=-1) == _hip.EINVAL and call(A=0) == _hip.EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(w_a=bad) == _hip.EINVAL
    assert call(A=1025) == _hip.ESHAPE and call(n_groups=0) == 0
    torch.cuda.synchronize()
    assert (out == -777).all()  # nothing ran


def test_one_row_per_group_is_the_answer_loss():
    """K = 1, uniform weights, w_a = 1: -log_evidence and d_logits are ``pnmn_answer_loss``'s loss and dlogits (scale 1) within
    rtol = atol = 1e-5, the bar of tests/test_hip_kernels.py::test_answer_loss; an invalid row has a zero gradient on both sides."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100)
    n, A = 37, 28
    logits = (rng.standard_normal((n, A)) * 3).astype(np.float32)
    answers = rng.integers(0, A, n).astype(np.int64)
    valid = (rng.random(n) > 0.3).astype(np.int32)
    assert 0 < valid.sum() < n
    got = launch(logits, valid, None, answers, np.arange(n + 1), 1.0, A)
    d = [torch.from_numpy(a).to(dev) for a in (logits, answers, valid)]
    predictions = torch.empty(n, dtype=torch.long, device=dev)
    loss, dlogits = torch.empty(n, device=dev), torch.empty(n, A, device=dev)
    _hip.check(_hip.lib().pnmn_answer_loss(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), predictions.data_ptr(), loss.data_ptr(),
                                           dlogits.data_ptr(), n, A, A, 1.0, _hip.stream_ptr(dev)), "answer_loss")
    torch.cuda.synchronize()
    ok = valid != 0
    assert np.array_equal(got["support"], valid) and np.isneginf(got["log_evidence"][~ok]).all()
    np.testing.assert_allclose(-got["log_evidence"][ok], loss.cpu().numpy()[ok], rtol=1e-5, atol=1e-5)
    assert (loss.cpu().numpy()[~ok] == INVALID_PROGRAM_LOSS).all()
    np.testing.assert_allclose(got["d_logits"], dlogits.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert (got["d_logits"][~ok] == 0).all() and (dlogits.cpu().numpy()[~ok] == 0).all() and (got["d_logits"][ok] != 0).any()
    assert np.array_equal(got["row_predictions"], predictions.cpu().numpy())


def test_autograd_node_on_leaf_logits():
    from probnmn.models.nmn import _MarginalAnswerLoss

    dev = torch.device("cuda:0")
    A = 28
    logits, valid, log_weight, answers, start = ragged_inputs(A, SEEDS[A])
    ref = marginal_loss_reference(logits, valid, log_weight, answers, start, 0.5, A)
    bar = row_bars(ref, start, 0.5)
    usable, sup = ref["usable"], ref["support"] > 0
    fixed = [torch.from_numpy(a).to(dev) for a in (answers, valid, log_weight, start)]
    upstream = np.linspace(-2.0, 3.0, 37)
    group_of = np.repeat(np.arange(37), np.diff(start))
    for scale in (np.ones(37), upstream):  # loss.sum(), then a different upstream gradient per question
        leaf = torch.from_numpy(logits).to(dev).requires_grad_(True)
        loss, log_posterior, predictions, support, consistent = _MarginalAnswerLoss.apply(leaf, *fixed, 0.5, A)
        assert loss.requires_grad and not any(t.requires_grad for t in (log_posterior, predictions, support, consistent))
        (loss * torch.from_numpy(scale).to(dev, torch.float32)).sum().backward()
        got = loss.detach().cpu().numpy()
        assert (np.abs(-got[sup] - ref["log_evidence"][sup]) <= 1e-5 * (1 + ref["max_abs_score"][sup])).all()
        assert (got[~sup] == INVALID_PROGRAM_LOSS).all() and np.array_equal(support.cpu().numpy(), ref["support"])
        assert np.array_equal(consistent.cpu().numpy(), ref["consistent_count"])
        assert np.array_equal(predictions.cpu().numpy(), ref["row_predictions"])
        assert np.array_equal(np.isfinite(log_posterior.cpu().numpy()), usable)
        grad = leaf.grad.cpu().numpy().astype(np.float64)
        want = ref["d_logits"] * scale[group_of][:, None]
        err = np.abs(grad - want) / (bar * np.maximum(np.abs(scale[group_of]), 1e-300))[:, None]
        print("upstream %s: largest |d logits - reference| / bar %.3g" % ("ones" if scale is not upstream else "per question", err[usable].max()))
        assert (err[usable] <= 1.0 + 1e-6).all() and (grad[~usable] == 0).all()  # (1e-6: the one fp32 multiply by the upstream value)
    with pytest.raises(ValueError):
        _MarginalAnswerLoss.apply(torch.from_numpy(logits).to(dev).requires_grad_(True), fixed[0], fixed[1],
                                  fixed[2].clone().requires_grad_(True), fixed[3], 0.5, A)


# ---- the network and the trainer -----------------------------------------------------------------------------------------

def _tiny(seed=0):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    pg = ProgramGenerator(vocab).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=32).to(dev)
    return vocab, pg, nmn, synthetic_batch(vocab, 8, seed=31), dev


@pytest.fixture(scope="module")
def models():
    return _tiny()


def _zero_grads(nmn):
    for p in nmn.parameters():
        p.grad = None


def test_marginal_answer_loss_of_the_network(models):
    vocab, pg, nmn, batch, dev = models
    image, answers = batch["image"].to(dev), batch["answer"].to(dev)
    nmn.train()
    head = nmn.classifier[6].weight

    # one hypothesis per question: the NMN's own loss on those programs
    rows = torch.arange(8, device=dev)
    _zero_grads(nmn)
    own = nmn(image, batch["program"], answers, rows=rows)
    own["loss"].sum().backward()
    own_loss, own_grad = own["loss"].detach().cpu().numpy(), head.grad.detach().clone()
    nmn.get_metrics(reset=True)
    metrics = nmn.get_metrics(reset=False)
    _zero_grads(nmn)
    out = nmn.marginal_answer_loss(image, batch["program"], np.arange(8), answers)
    assert set(out) == {"loss", "log_posterior", "hypothesis_predictions", "support", "consistent_count"}
    assert out["loss"].requires_grad and not any(out[k].requires_grad for k in out if k != "loss")
    out["loss"].sum().backward()
    assert out["support"].tolist() == [1] * 8 and (out["log_posterior"] == 0).all()  # (valid programs, each alone in its group)
    np.testing.assert_allclose(out["loss"].detach().cpu().numpy(), own_loss, rtol=0, atol=1e-5)
    once_loss, once_grad = out["loss"].detach().clone(), head.grad.detach().clone()
    scale = float(own_grad.abs().max())
    assert scale > 0 and float((once_grad - own_grad).abs().max()) <= 1e-4 * scale
    trunk = [nmn.stem[0].weight.grad, nmn.classifier[0].weight.grad, nmn.classifier[4].weight.grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in trunk)
    assert np.array_equal(out["hypothesis_predictions"].cpu().numpy(), own["predictions"].cpu().numpy())

    # question 2's program given twice, with weights log 0.3 and log 0.7: the loss and the gradient of the program given once
    qrows = np.array([0, 1, 2, 2, 3, 4, 5, 6, 7])
    programs = batch["program"][qrows]
    log_weights = np.zeros(9, np.float32)
    log_weights[2], log_weights[3] = np.log(0.3), np.log(0.7)
    _zero_grads(nmn)
    twice = nmn.marginal_answer_loss(image, programs, qrows, answers, log_weights)
    twice["loss"].sum().backward()
    assert twice["support"].tolist() == [1, 1, 2, 1, 1, 1, 1, 1]
    np.testing.assert_allclose(twice["loss"].detach().cpu().numpy(), once_loss.cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(twice["log_posterior"].cpu().numpy()[2:4], np.log([0.3, 0.7]), rtol=0, atol=1e-5)
    assert float((head.grad - once_grad).abs().max()) <= 1e-4 * scale

    # question 4 without a hypothesis: the constant, and no gradient from it
    qrows = np.array([0, 1, 2, 3, 5, 6, 7])
    _zero_grads(nmn)
    out = nmn.marginal_answer_loss(image, batch["program"][qrows], qrows, answers.cpu(), answer_weight=1.0)
    got = out["loss"].detach().cpu().numpy()
    assert got[4] == INVALID_PROGRAM_LOSS and out["support"].tolist() == [1, 1, 1, 1, 0, 1, 1, 1]
    np.testing.assert_allclose(np.delete(got, 4), np.delete(once_loss.cpu().numpy(), 4), rtol=0, atol=1e-5)
    (from_none,) = torch.autograd.grad(out["loss"][4], head, retain_graph=True)
    assert (from_none == 0).all()
    (from_one,) = torch.autograd.grad(out["loss"][3], head)
    assert (from_one != 0).any()

    # no hypothesis at all; arguments that are wrong
    none = nmn.marginal_answer_loss(image, batch["program"][:0], np.zeros(0, np.int64), answers)
    assert (none["loss"].cpu().numpy() == INVALID_PROGRAM_LOSS).all() and none["support"].tolist() == [0] * 8 and not none["loss"].requires_grad
    for bad in (dict(question_rows=np.array([1, 0])), dict(question_rows=np.array([0, 8])), dict(answers=answers[:7]),
                dict(answers=answers.float()), dict(answer_weight=float("nan")), dict(answer_weight=None),
                dict(log_weights=np.zeros(3)), dict(log_weights=torch.zeros(2, requires_grad=True))):
        kwargs = dict(question_rows=np.array([0, 1]), answers=answers)
        kwargs.update(bad)
        with pytest.raises(ValueError):
            nmn.marginal_answer_loss(image, batch["program"][:2], kwargs.pop("question_rows"), kwargs.pop("answers"), **kwargs)
    with pytest.raises(TypeError):
        nmn.marginal_answer_loss(image, batch["program"][:2], np.array([0, 1]), answers, max_rows=1)  # (one pass: there is no max_rows)
    assert nmn.training and nmn.get_metrics(reset=False) == metrics  # the flag and the metrics are what they were
    nmn.eval()
    nmn.marginal_answer_loss(image, batch["program"], np.arange(8), answers)
    assert not nmn.training
    nmn.train()
    _zero_grads(nmn)


def test_marginal_module_training_step():
    from probnmn import hypothesis_rows
    from probnmn.trainers.module_training import ModuleTrainingStep

    vocab, pg, nmn, batch, dev = _tiny(seed=1)
    dbatch = {k: batch[k].to(dev) for k in ("question", "image", "answer")}
    before = {n: p.detach().clone() for n, p in nmn.named_parameters()}
    frozen = {n: p.detach().clone() for n, p in pg.named_parameters()}

    # the same deterministic, constrained beam the step will decode, scored by the plain posterior launch
    exclude = [getattr(pg, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
    constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)
    pg.eval()
    with torch.no_grad():
        queued = hypothesis_rows.queue_hypotheses(pg, dbatch, 0, hypothesis_rows.HostCopies(), 4, None, constraint, False, {}, True)
    pg.train()
    _, programs, question_rows, log_weights, _, _ = hypothesis_rows.awaited_hypotheses(nmn, queued)
    R = len(question_rows)
    assert 8 <= R <= 32 and len(set(question_rows.tolist())) == 8  # (a constrained beam: every question has a valid hypothesis)
    posterior = nmn.answer_posterior(dbatch["image"], torch.from_numpy(programs), question_rows, dbatch["answer"], log_weights)
    evidence, support = posterior["log_evidence"].cpu().numpy().astype(np.float64), posterior["support"].cpu().numpy()
    want = np.where(support > 0, -evidence, float(INVALID_PROGRAM_LOSS))
    score = (posterior["log_posterior"].cpu().numpy().astype(np.float64) + evidence[question_rows])
    bars = np.array([1e-5 * (1 + np.abs(score[question_rows == g][np.isfinite(score[question_rows == g])]).max(initial=0.0))
                     for g in range(8)])

    step = ModuleTrainingStep(nmn, lr=1e-3, program_generator=pg, objective="marginal", beam_size=4, constrained=True)
    first = step.step(dbatch)
    assert set(first) == {"loss", "metrics", "support", "rows"} and first["metrics"] is None and first["rows"] == R
    assert float(first["support"]) == pytest.approx(support.mean())
    print("first marginal loss %.6f, from answer_posterior %.6f, bar %.3g; %d rows, support %.3f"
          % (float(first["loss"]), want.mean(), bars.mean(), R, float(first["support"])))
    assert abs(float(first["loss"]) - want.mean()) <= bars.mean()
    assert pg.training and nmn.training and step.iteration == 1
    moved = [n for n, p in nmn.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert "classifier.6.weight" in moved and "stem.0.weight" in moved and len(moved) > 10
    assert all(torch.equal(p.detach(), frozen[n]) for n, p in pg.named_parameters())  # the generator is frozen

    losses = [float(first["loss"])] + [float(step.step(dbatch)["loss"]) for _ in range(19)]
    print("marginal loss over 20 steps on the fixed batch: %.4f -> %.4f" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    step.close()

    # the sampled hypotheses: num_programs draws per question, uniformly weighted, invalid ones dropped, equal ones merged
    sampled = ModuleTrainingStep(nmn, program_generator=pg, objective="marginal", num_programs=4)
    out = sampled.step(dbatch)
    assert 0 <= out["rows"] <= 32 and out["metrics"] is None and np.isfinite(float(out["loss"]))
    sampled.close()
