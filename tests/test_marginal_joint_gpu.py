"""Joint marginal-likelihood training on the MI355X: the differentiable scoring pass of the program generator against its
plain one and against the beam's own scores, ``NeuralModuleNetwork.answer_log_likelihood`` against ``forward``, the objective
against ``marginal_answer_loss`` on the same candidates, and ``MarginalJointStep`` on a fixed batch of 8 questions.

Tolerances are the project's own for each quantity: 1e-5 for a log-softmax quantity (tests/test_hip_kernels.py::
test_answer_loss), 1e-4 per decoded token for a sequence score against the beam's (tests/test_beam_gpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID_PROGRAM_LOSS = np.float32(3.33)


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


def _sequence_scores(logits, targets, pad):
    """sum over the targets that are not padding of log_softmax(logits)[target], fp64 [R] on the host."""
    lp = torch.log_softmax(logits.detach().double(), -1).gather(2, targets.unsqueeze(-1)).squeeze(-1)
    return (lp * (targets != pad)).sum(1).cpu().numpy()


def _constrained_beam(pg, nmn, dbatch, K=4):
    """The candidates ``MarginalJointStep(constrained=True, beam_size=K)`` decodes: (programs [R, T], question_rows [R], the
    beam's merged log-weights [R])."""
    from probnmn import hypothesis_rows

    exclude = [getattr(pg, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
    constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)
    was = pg.training
    pg.eval()
    with torch.no_grad():
        queued = hypothesis_rows.queue_hypotheses(pg, dbatch, 0, hypothesis_rows.HostCopies(), K, None, constraint, False, {}, True)
    pg.train(was)
    _, programs, question_rows, log_weights, _, _ = hypothesis_rows.awaited_hypotheses(nmn, queued)
    return programs, question_rows, log_weights


def test_teacher_forced_logits_with_a_graph(models):
    vocab, pg, nmn, batch, dev = models
    question, program = batch["question"].to(dev), batch["program"].to(dev)
    pg.eval()
    pg.get_metrics(reset=False)
    before = pg.get_metrics(reset=False)
    plain, plain_targets = pg.teacher_forced_logits(question, program)
    assert not plain.requires_grad and plain.grad_fn is None  # (grad mode is on: the plain call still builds no graph)
    for p in pg.parameters():
        p.grad = None
    logits, targets = pg.teacher_forced_logits(question, program, differentiable=True)
    assert logits.requires_grad and torch.equal(targets, plain_targets) and logits.shape == plain.shape
    worst = float((logits.detach() - plain).abs().max())
    print("eval() mode: largest |differentiable - plain| logit %.3g" % worst)
    assert worst <= 1e-5
    score = torch.log_softmax(logits, -1).gather(2, targets.unsqueeze(-1)).squeeze(-1) * (targets != pg._pad_index)
    score.sum().backward()
    unreached = [n for n, p in pg.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())
                 or not float(p.grad.abs().max()) > 0]
    assert not unreached, unreached
    assert not pg.training and pg.get_metrics(reset=False) == before
    pg.train()
    state = torch.get_rng_state()
    again, _ = pg.teacher_forced_logits(question, program)
    assert pg.training and torch.equal(again, plain) and torch.equal(torch.get_rng_state(), state) and not again.requires_grad
    trained, _ = pg.teacher_forced_logits(question, program, differentiable=True)
    assert pg.training and trained.requires_grad and bool(torch.isfinite(trained).all())
    with pytest.raises(TypeError):
        pg.teacher_forced_logits(question, program, True)  # (keyword only)
    for p in pg.parameters():
        p.grad = None


def _beam_against_teacher_forcing(pg, nmn, dbatch, dev, what):
    """The teacher-forced score of every hypothesis of a constrained beam of 4, over the tokens the beam scored, against
    ``beam_log_probabilities`` within 1e-4 per step; returns how many hypotheses ended within the decoding steps."""
    from probnmn.trainers.marginal_training import candidate_targets

    exclude = [getattr(pg, name) for name in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
    constraint = nmn.engine.compiler.decoding_automaton(exclude=exclude)
    pg.eval()
    with torch.no_grad():
        beams = pg(dbatch["question"], decoding_strategy="beam", beam_size=4, constraint=constraint)
    tokens, scores = beams["beam_predictions"], beams["beam_log_probabilities"]
    B, K, T = tokens.shape
    rows = torch.arange(B, device=dev).repeat_interleave(K)
    logits, targets = pg.teacher_forced_logits(dbatch["question"][rows], candidate_targets(tokens.view(B * K, T), pg),
                                               differentiable=True)
    pg.train()
    assert targets.shape == (B * K, T + 1)
    # a hypothesis that ended within the T steps: every target, its @end@ among them, is a token the beam scored.  One that ran
    # out of steps has no @end@ of its own: the boundary @end@ behind its T tokens is the one target the beam did not score
    ended = (tokens.view(B * K, T) == pg._end_index).any(1)
    scored = targets.clone()
    scored[~ended, T] = pg._pad_index
    got = _sequence_scores(logits, scored, pg._pad_index)
    want = scores.view(-1).double().cpu().numpy()
    live = np.isfinite(want) & (want > -1e30)
    steps = targets.size(1)
    print("%s generator: teacher-forced score against the beam's over %d of %d hypotheses (%d ended): largest difference %.3g "
          "(bar %.3g)" % (what, int(live.sum()), B * K, int(ended.sum()), np.abs(got[live] - want[live]).max(), 1e-4 * steps))
    assert live.sum() >= 16
    np.testing.assert_allclose(got[live], want[live], rtol=0, atol=1e-4 * steps)
    return int((ended.cpu().numpy() & live).sum())


def test_sequence_score_is_the_beams_own(models):
    """1e-4 per step is tests/test_beam_gpu.py's bar for the same quantity.  An untrained generator's constrained hypotheses
    fill the decoding steps and end without an @end@; one fitted to the batch's own programs ends them, so both ways of
    ``candidate_targets`` are compared."""
    from probnmn.optim import ClampAdam

    vocab, pg, nmn, batch, dev = models
    dbatch = {k: batch[k].to(dev) for k in ("question", "image", "answer")}
    _beam_against_teacher_forcing(pg, nmn, dbatch, dev, "untrained")
    fitted = _tiny(seed=3)[1]
    opt = ClampAdam(list(fitted.parameters()), lr=2e-3, clamp=5.0)
    program = batch["program"].to(dev)
    for _ in range(100):  # (bench.py's fit of the generator: supervised teacher forcing on the batch)
        opt.zero_grad()
        fitted(dbatch["question"], program, decoding_strategy="sampling", need_predictions=False)["loss"].mean().backward()
        opt.step()
    assert _beam_against_teacher_forcing(fitted, nmn, dbatch, dev, "fitted") >= 8


def test_answer_log_likelihood_is_forwards_loss(models):
    vocab, pg, nmn, batch, dev = models
    image, answers = batch["image"].to(dev), batch["answer"].to(dev)
    nmn.train()
    qrows = np.array([0, 1, 2, 2, 3, 5, 6, 7, 7])
    programs = batch["program"][[0, 1, 2, 3, 3, 5, 6, 7, 0]]
    rows = torch.from_numpy(qrows).to(dev)
    nmn.get_metrics(reset=True)
    metrics = nmn.get_metrics(reset=False)
    own = nmn(image, programs, answers[rows], rows=rows)
    nmn.get_metrics(reset=True)
    out = nmn.answer_log_likelihood(image, programs, qrows, answers)
    assert set(out) == {"log_answer", "hypothesis_predictions"}
    assert out["log_answer"].requires_grad and not out["hypothesis_predictions"].requires_grad
    np.testing.assert_allclose(out["log_answer"].detach().cpu().numpy(), -own["loss"].detach().cpu().numpy(), rtol=0, atol=1e-5)
    assert torch.equal(out["hypothesis_predictions"], own["predictions"])
    head = nmn.classifier[6].weight
    (g,) = torch.autograd.grad(out["log_answer"].sum(), head)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert nmn.training and nmn.get_metrics(reset=False) == metrics
    with torch.no_grad():
        constant = nmn.answer_log_likelihood(image, programs, qrows, answers)["log_answer"]
    assert not constant.requires_grad
    np.testing.assert_allclose(constant.cpu().numpy(), out["log_answer"].detach().cpu().numpy(), rtol=0, atol=1e-5)
    # an invalid program is no candidate: -inf
    broken = programs.clone()
    broken[4] = broken[4].flip(0)
    assert not nmn.engine.compiler.compile_batch(broken.numpy())[4].valid
    ruled_out = nmn.answer_log_likelihood(image, broken, qrows, answers)["log_answer"].detach().cpu().numpy()
    assert np.isneginf(ruled_out[4]) and np.isfinite(np.delete(ruled_out, 4)).all()
    none = nmn.answer_log_likelihood(image, programs[:0], np.zeros(0, np.int64), answers)
    assert none["log_answer"].shape == (0,) and none["hypothesis_predictions"].shape == (0,)
    for bad in (dict(question_rows=np.array([1, 0])), dict(question_rows=np.array([0, 8])), dict(answers=answers[:7]),
                dict(answers=answers.float())):
        kwargs = dict(question_rows=np.array([0, 1]), answers=answers)
        kwargs.update(bad)
        with pytest.raises(ValueError):
            nmn.answer_log_likelihood(image, programs[:2], kwargs["question_rows"], kwargs["answers"])
    for p in nmn.parameters():
        p.grad = None


def test_objective_against_the_marginal_answer_loss(models):
    from probnmn import _hip, hypothesis_rows
    from probnmn.modules.marginal_likelihood import sequence_marginal_loss
    from probnmn.trainers.marginal_training import candidate_targets

    vocab, pg, nmn, batch, dev = models
    dbatch = {k: batch[k].to(dev) for k in ("question", "image", "answer")}
    programs, question_rows, _ = _constrained_beam(pg, nmn, dbatch)
    R = len(question_rows)
    assert 8 <= R <= 32 and len(set(question_rows.tolist())) == 8
    rows = torch.from_numpy(question_rows).to(dev)
    on_dev = torch.from_numpy(programs).to(dev)
    pg.eval(), nmn.train()
    logits, targets = pg.teacher_forced_logits(dbatch["question"][rows], candidate_targets(on_dev, pg), differentiable=True)
    pg.train()
    group_start = hypothesis_rows.group_start_on_device(question_rows, 8, dev)
    # lq: the teacher-forced scores as ``pnmn_hypothesis_posterior`` reports them for these logits in reranking (a plain launch)
    lq_dev = torch.empty(R, dtype=torch.float32, device=dev)
    unused = [torch.empty(R, dtype=torch.float32, device=dev), torch.empty(8, dtype=torch.float32, device=dev),
              torch.empty(8, dtype=torch.int32, device=dev)]
    flat = logits.detach().contiguous()
    _hip.check(_hip.lib().pnmn_hypothesis_posterior(
        flat.data_ptr(), targets.data_ptr(), targets.stride(0), 0, 0, 0, 0, group_start.data_ptr(), 1.0, 0.0, 0.0, pg._pad_index, 0,
        lq_dev.data_ptr(), 0, unused[0].data_ptr(), unused[1].data_ptr(), unused[2].data_ptr(), 0, 8, R, flat.size(1), flat.size(2),
        1, 1, _hip.stream_ptr(dev)), "hypothesis_posterior")
    lq = lq_dev.double().cpu().numpy()
    np.testing.assert_allclose(lq, _sequence_scores(logits, targets, pg._pad_index), rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        log_answer = nmn.answer_log_likelihood(dbatch["image"], on_dev, question_rows, dbatch["answer"])["log_answer"]
        existing = nmn.marginal_answer_loss(dbatch["image"], on_dev, question_rows, dbatch["answer"],
                                            lq_dev)
    loss,log_posterior, support = sequence_marginal_loss(x=(logits, targets, pg._pad_index), log_q=log_answer,
                                                          group_start=group_start, weights=(1.0, 0.0, 1.0))
    assert np.array_equal(support.cpu().numpy(), existing["support"].cpu().numpy()) and (support > 0).all()
    norm = np.array([np.logaddexp.reduce(lq[question_rows == g]) for g in range(8)])
    got, want = loss.detach().double().cpu().numpy() + norm, existing["loss"].double().cpu().numpy()
    print("L_g + logsumexp_g(lq) against marginal_answer_loss: largest difference %.3g (bar 1e-5); largest |lq| %.3g"
          % (np.abs(got - want).max(), np.abs(lq).max()))
    score = lq + log_answer.double().cpu().numpy()
    bar = 1e-5 * (1 + np.abs(score).max())
    worst = np.abs(log_posterior.cpu().numpy() - existing["log_posterior"].cpu().numpy()).max()
    print("log_posterior: largest difference %.3g (bar %.3g)" % (worst, bar))
    assert worst <= bar
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


def _moved(model, before):
    return [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]


def test_marginal_joint_step():
    from probnmn.trainers import MarginalJointStep

    vocab, pg, nmn, batch, dev = _tiny(seed=1)
    dbatch = {k: batch[k].to(dev) for k in ("question", "image", "answer")}
    pg_before = {n: p.detach().clone() for n, p in pg.named_parameters()}
    nmn_before = {n: p.detach().clone() for n, p in nmn.named_parameters()}
    R = len(_constrained_beam(pg, nmn, dbatch)[1])

    step = MarginalJointStep(pg, nmn, beam_size=4, constrained=True, lr=1e-3)
    first = step.step(dbatch)
    assert set(first) == {"loss", "support", "rows", "posterior_on_map"} and first["rows"] == R
    assert 1.0 <= float(first["support"]) <= 4.0 and 0.25 - 1e-6 <= float(first["posterior_on_map"]) <= 1.0 + 1e-6
    assert pg.training and nmn.training and step.iteration == 1 and set(step.models) == {"program_generator", "nmn"}
    moved = _moved(nmn, nmn_before)
    assert "classifier.6.weight" in moved and "stem.0.weight" in moved and len(moved) > 10
    assert len(_moved(pg, pg_before)) > 10
    losses = [float(first["loss"])] + [float(step.step(dbatch)["loss"]) for _ in range(19)]
    print("joint marginal loss over 20 steps on the fixed batch: %.4f -> %.4f" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    step.close()

    # the generator alone: the modules are constants of the objective
    pg_before = {n: p.detach().clone() for n, p in pg.named_parameters()}
    nmn_before = {n: p.detach().clone() for n, p in nmn.named_parameters()}
    alone = MarginalJointStep(pg, nmn, beam_size=4, constrained=True, train_modules=False, lr=1e-3)
    out = alone.step(dbatch)
    assert set(alone.models) == {"program_generator"} and np.isfinite(float(out["loss"])) and out["rows"] >= 8
    assert not _moved(nmn, nmn_before) and len(_moved(pg, pg_before)) > 10
    # a stochastic beam: the same report
    alone.close()
    explore = MarginalJointStep(pg, nmn, beam_size=4, constrained=True, without_replacement=True, train_modules=False)
    out = explore.step(dbatch)
    assert 8 <= out["rows"] <= 32 and np.isfinite(float(out["loss"])) and 1.0 <= float(out["support"]) <= 4.0
    explore.close()


def test_a_batch_without_a_valid_candidate_pays_the_constant():
    from probnmn.runtime import program_compiler as pc
    from probnmn.trainers import MarginalJointStep

    vocab, pg, nmn, batch, dev = _tiny(seed=2)
    dbatch = {k: batch[k].to(dev) for k in ("question", "image", "answer")}
    # a generator that emits one attention token for ever: no hypothesis of its (unconstrained) beam is a program -- one that
    # differs from the endless row in a single token is none either, since a valid program needs a scene at its end AND a
    # query at its start
    tokens = vocab.get_token_to_index_vocabulary("programs")
    stuck = next(i for t, i in sorted(tokens.items(), key=lambda kv: kv[1]) if pc.classify_token(t) == pc.ATT)
    with torch.no_grad():
        pg._output_projection_layer.bias[stuck] = 1e4
    pg_before = {n: p.detach().clone() for n, p in pg.named_parameters()}
    nmn_before = {n: p.detach().clone() for n, p in nmn.named_parameters()}
    step = MarginalJointStep(pg, nmn, beam_size=4, lr=1e-3)
    out = step.step(dbatch)
    assert out["rows"] == 0 and float(out["loss"]) == INVALID_PROGRAM_LOSS and float(out["support"]) == 0.0
    assert np.isnan(float(out["posterior_on_map"])) and step.iteration == 1
    assert not _moved(pg, pg_before) and not _moved(nmn, nmn_before)
    step.close()
