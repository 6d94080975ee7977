"""Grammar-masked logits on the MI355X: ``pnmn_grammar_logits`` / ``_bwd`` against the fp64 host reference of
tests/helpers/grammar_logits_reference.py, their composition with the sequence losses, ``decoding_strategy="grammar_sampling"``
and ``teacher_forced_logits(constraint=)`` of the program generator, and one step of the three trainers under the grammar.

Bars.  ``masked`` and the backward pass copy or fill: bit for bit.  ``outside`` counts: exact.  ``log_mass`` and the losses are
the lse arithmetic of ``pnmn_seq_nll_fwd``: rtol = atol = 1e-5, gradients rtol 1e-4 / atol 1e-6 (tests/test_hip_kernels.py::
test_sequence_nll_fwd_bwd).  The sampled pass against the teacher-forced pass over its own predictions runs two decoder modes:
its bar is four times the gap the existing "sampling" strategy shows on the same model and seed, plus 1e-6."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import constrained_choice as cc  # noqa: E402
import filtered_inputs as fi  # noqa: E402
import grammar_logits_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, UNK, START, END = fi.PAD, fi.UNK, fi.START, 3
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)


@pytest.fixture(scope="module")
def grammar():
    """(compiler, automaton) of the CLEVR program vocabulary: V = 44, end = 3."""
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    return comp, comp.decoding_automaton(exclude=(PAD, UNK, START, END))


def _cyclic_automaton(V):
    """Three states over three token classes (class = token mod 3, next = state + class mod 3, state 0 accepts): sets that
    change with the state at any vocabulary size."""
    nxt = np.array([[(s + c) % 3 for c in range(3)] for s in range(3)], np.uint8)
    return SimpleNamespace(token_class=(np.arange(V) % 3).astype(np.uint8), next_state=nxt, min_left=np.array([0, 1, 1], np.uint8))


def _automata(V, grammar):
    out = [("trivial", cc.trivial_tables(V, END)[1]), ("cyclic", _cyclic_automaton(V))]
    return out + [("clevr", grammar[1])] if V == 44 else out


def _rows(tab, B, T, V, horizon, rng, first_kind):
    """tokens [B, T]: row b is of kind (first_kind + b) mod 5 -- 0 a row the constrained sampler could emit (its @end@
    repeated), 1 the same with an illegal token (@start@) mid-row, 2 with tokens outside [0, V), 3 all padding, 4 an early
    @end@ with padding behind it."""
    s, f = np.zeros(B, np.int64), np.zeros(B, bool)
    tokens = np.zeros((B, T), np.int64)
    for t in range(T):
        mask = cc.allowed_mask(tab, s, f, t, max(horizon, T), V, PAD, UNK, START)
        tokens[:, t] = [rng.choice(np.flatnonzero(m)) for m in mask]
        s, f = cc.advance(tab, s, f, tokens[:, t])
    kinds = (first_kind + np.arange(B)) % 5
    for b, kind in enumerate(kinds):
        if kind == 1:
            tokens[b, T // 2] = START
        elif kind == 2:
            tokens[b, T // 2] = V + 5
            tokens[b, T - 1] = -1 if T > 1 else V
        elif kind == 3:
            tokens[b] = PAD
        elif kind == 4:
            tokens[b, min(1, T - 1)] = END
            tokens[b, min(1, T - 1) + 1:] = PAD
    return tokens


def _run(logits, tokens, auto, horizon):
    from probnmn.modules.grammar import grammar_logits

    masked, log_mass, outside = grammar_logits(logits, tokens, auto, horizon, PAD, UNK, START, END)
    return masked, log_mass, outside


@pytest.mark.parametrize("V", [7, 44, 65, 128])
@pytest.mark.parametrize("T", [1, 5, 27])
@pytest.mark.parametrize("B", [1, 9, 33])
def test_kernel_against_the_reference(grammar, B, T, V):
    rng = np.random.default_rng(1000 * B + 10 * T + V)
    for name, auto in _automata(V, grammar):
        tab = cc.Tables(auto, END)
        for horizon in sorted({max(1, T // 2), T, T + 3}):
            what = "%s automaton, B %d T %d V %d, horizon %d" % (name, B, T, V, horizon)
            tokens_h = _rows(tab, B, T, V, horizon, rng, first_kind=(B + T + horizon) % 5)
            # one step more than the kernel is given, on both: the views logits[:, :-1] / tokens[:, 1:] are strided
            wide = torch.from_numpy(rng.normal(0, 3, (B, T + 1, V)).astype(np.float32)).to(DEV)
            tokens_wide = torch.from_numpy(np.concatenate((np.full((B, 1), START), tokens_h), 1)).to(DEV)
            logits, tokens = wide[:, :-1].requires_grad_(), tokens_wide[:, 1:]
            assert B == 1 or (not logits.is_contiguous() and not tokens.is_contiguous())
            masked, log_mass, outside = _run(logits, tokens, auto, horizon)
            z = logits.detach().cpu().numpy()
            ref_masked, sets, ref_mass, ref_outside = gr.grammar_logits_ref(z, tokens_h, tab, horizon, PAD, UNK, START)
            want_bits = np.where(sets, z.view(np.int32), NEG_INF_BITS)
            assert np.array_equal(masked.detach().cpu().numpy().view(np.int32), want_bits), what
            assert sets.any(2).all(), what                                                    # no step is all -inf
            assert np.array_equal(outside.cpu().numpy(), ref_outside), (what, outside.cpu().numpy(), ref_outside)
            got_mass = log_mass.cpu().numpy()
            assert (got_mass <= 0).all() and not log_mass.requires_grad and not outside.requires_grad, what
            np.testing.assert_allclose(got_mass, ref_mass, rtol=1e-5, atol=1e-5, err_msg=what)
            assert (got_mass[sets.all(2)] == 0).all(), what                                   # an unmasked step: exactly 0
            # backward: a copy inside the sets, 0 outside
            d_masked = torch.from_numpy(rng.normal(0, 1, (B, T, V)).astype(np.float32)).to(DEV)
            (d_logits,) = torch.autograd.grad(masked, logits, d_masked)
            want_grad = np.where(sets, d_masked.cpu().numpy(), np.float32(0))
            assert np.array_equal(d_logits.cpu().numpy().view(np.int32), want_grad.view(np.int32)), what
            # the contiguous copies give the same bits, and so does a row on its own
            again = _run(logits.detach().contiguous(), tokens.contiguous(), auto, horizon)
            assert all(torch.equal(a, b) for a, b in zip(again, (masked.detach(), log_mass, outside))), what
            for b in sorted({0, B // 2, B - 1}):
                alone = _run(logits.detach()[b:b + 1], tokens[b:b + 1], auto, horizon)
                assert torch.equal(alone[0].view(torch.int32), masked.detach()[b:b + 1].view(torch.int32)), (what, b)
                assert torch.equal(alone[1], log_mass[b:b + 1]) and torch.equal(alone[2], outside[b:b + 1]), (what, b)


def test_optional_outputs_and_an_empty_batch(grammar):
    from probnmn import _hip, _hip_grammar
    from probnmn.modules.seq2seq_base import constraint_tables

    _, auto = grammar
    B, T, V = 5, 6, 44
    rng = np.random.default_rng(2)
    tab = cc.Tables(auto, END)
    tokens_h = _rows(tab, B, T, V, T, rng, 0)
    logits, tokens = torch.from_numpy(rng.normal(0, 3, (B, T, V)).astype(np.float32)).to(DEV), torch.from_numpy(tokens_h).to(DEV)
    full = _run(logits, tokens, auto, T)
    tc, ns, ml, end = constraint_tables(auto, V, END)
    masked = torch.full((B, T, V), 7.0, device=DEV)
    _hip.check(_hip_grammar.lib().pnmn_grammar_logits(
        logits.data_ptr(), T * V, tokens.data_ptr(), T, masked.data_ptr(), T * V, 0, 0, B, T, V, T, PAD, UNK, START, end,
        tc.ctypes.data, ns.ctypes.data, ml.ctypes.data, ns.shape[0], ns.shape[1], _hip.stream_ptr(logits.device)), "grammar_logits")
    assert torch.equal(masked.view(torch.int32), full[0].view(torch.int32))
    empty = _run(logits[:0], tokens[:0], auto, T)
    assert empty[0].shape == (0, T, V) and empty[1].shape == (0, T) and empty[2].shape == (0,)
    with pytest.raises(ValueError):
        _run(logits, tokens[:, :-1], auto, T)
    with pytest.raises(ValueError):
        _run(logits, tokens, cc.trivial_tables(V + 1, END)[1], T)


def test_composition_with_the_sequence_losses(grammar):
    from probnmn.modules.marginal_likelihood import sequence_marginal_loss
    from probnmn.modules.seq2seq_base import sequence_nll

    _, auto = grammar
    B, T, V = 9, 12, 44
    rng = np.random.default_rng(4)
    tab = cc.Tables(auto, END)
    raw = _rows(tab, B, T, V, T, rng, first_kind=0)  # (rows of every kind: the losses must stay finite)
    scored = np.where((raw >= 0) & (raw < V), raw, END)  # (the sequence losses index the row: tokens inside [0, V) only)
    trimmed = scored.copy()
    for row in trimmed:
        ends = np.flatnonzero(row == END)
        if ends.size:
            row[ends[0] + 1:] = PAD
    assert ((trimmed == scored) | (trimmed == PAD)).all() and trimmed.min() >= 0 and trimmed.max() < V
    logits = torch.from_numpy(rng.normal(0, 3, (B, T, V)).astype(np.float32)).to(DEV).requires_grad_()
    tokens, mask_tokens = torch.from_numpy(scored).to(DEV), torch.from_numpy(trimmed).to(DEV)
    masked, _, _ = _run(logits, tokens, auto, T)
    loss = sequence_nll(masked, tokens, mask_tokens, PAD, 1e-12)
    loss.sum().backward()
    z = logits.detach().cpu().numpy()
    ref_masked, sets, _, _ = gr.grammar_logits_ref(z, scored, tab, T, PAD, UNK, START)
    ref_loss, ref_grad = gr.sequence_nll_ref(ref_masked, scored, trimmed, PAD, 1e-12)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref_loss, rtol=1e-5, atol=1e-5)
    grad = logits.grad.cpu().numpy()
    np.testing.assert_allclose(grad, np.where(sets, ref_grad, 0.0), rtol=1e-4, atol=1e-6)
    assert np.isfinite(grad).all() and (grad[~sets] == 0).all() and np.abs(grad[sets]).max() > 0
    # the gradient mode of the sequence marginal over the same masked logits: finite, 0 at every masked entry
    logits.grad = None
    masked, _, _ = _run(logits, tokens, auto, T)
    group_start = torch.tensor([0, 2, 5, B], dtype=torch.int32, device=DEV)
    loss_g, log_posterior, support = sequence_marginal_loss(x=(masked, mask_tokens, PAD), group_start=group_start,
                                                            weights=(1.0, 0.0, 0.0))
    loss_g.sum().backward()
    grad = logits.grad.cpu().numpy()
    assert np.isfinite(loss_g.detach().cpu().numpy()).all() and np.isfinite(log_posterior.cpu().numpy()).all()
    assert np.isfinite(grad).all() and (grad[~sets] == 0).all() and np.abs(grad[sets]).max() > 0


# ---- the model -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def generator(grammar):
    """A fresh ProgramGenerator (dropout 0) whose @end@ bias is raised, so that sampled rows end inside the decoding steps,
    six questions, and the automaton."""
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(5)
    pg = ProgramGenerator(vocab, dropout=0.0).to(DEV)
    with torch.no_grad():
        pg._output_projection_layer.bias[END] += 1.0
    pg.train()
    return pg, synthetic_batch(vocab, 6, seed=17)["question"].to(DEV), grammar[1], grammar[0]


def _own_targets(pg, predictions):
    from probnmn.trainers.marginal_training import candidate_targets

    return candidate_targets(predictions, pg)


def _row_log_probabilities(logits, targets):
    lp = torch.log_softmax(logits.detach().double(), -1).gather(2, targets.unsqueeze(-1)).squeeze(-1)
    return (lp * (targets != PAD)).sum(1).cpu().numpy()


def test_grammar_sampling_is_the_constrained_sampler_with_a_graph(generator):
    pg, question, auto, comp = generator
    T = pg._max_decoding_steps
    torch.manual_seed(11)
    drawn = pg(question, decoding_strategy="constrained_sampling", constraint=auto)
    after = torch.get_rng_state()
    torch.manual_seed(11)
    out = pg(question, decoding_strategy="grammar_sampling", constraint=auto)
    assert torch.equal(torch.get_rng_state(), after)                            # one seed, as "sampling" draws it
    assert set(out) == {"predictions", "loss", "grammar_log_mass", "grammar_outside"}
    assert torch.equal(out["predictions"], drawn["predictions"]) and out["loss"].requires_grad
    rows = out["predictions"].cpu().numpy()
    assert all(auto.accepts(cc.cut_at_end(row, END)) and comp.compile(cc.cut_at_end(row, END)).valid for row in rows)
    assert (out["grammar_outside"] == 0).all() and out["grammar_outside"].dtype == torch.int32
    assert (out["grammar_log_mass"] <= 0).all() and not out["grammar_log_mass"].requires_grad
    # q_c >= q on the samples: the constrained sampler's own loss is under q
    assert (out["loss"].detach() <= drawn["loss"] + 1e-5).all()

    # teacher forced on its own rows, against the fp64 masked log-softmax of teacher_forced_logits(constraint=)
    targets_in = _own_targets(pg, out["predictions"])
    forced = pg(question, targets_in, decoding_strategy="grammar_sampling", constraint=auto)
    assert set(forced) == {"loss", "grammar_log_mass", "grammar_outside"} and (forced["grammar_outside"] == 0).all()
    masked, targets = pg.teacher_forced_logits(question, targets_in, constraint=auto)
    plain, _ = pg.teacher_forced_logits(question, targets_in)
    assert not masked.requires_grad and targets.shape == (6, T + 1)
    log_qc, log_q = _row_log_probabilities(masked, targets), _row_log_probabilities(plain, targets)
    weights = (targets != PAD).sum(1).double().cpu().numpy()
    np.testing.assert_allclose(forced["loss"].detach().cpu().numpy(), -log_qc / (weights + 1e-13), rtol=0, atol=1e-5)
    assert (log_qc >= log_q).all() and np.isfinite(log_qc).all()
    np.testing.assert_allclose(forced["grammar_log_mass"].cpu().numpy(), log_q - log_qc, rtol=1e-5, atol=1e-4)
    inside = torch.isfinite(masked)
    assert torch.equal(masked[inside], plain[inside]) and inside.any(2).all() and not inside.all()
    graph, _ = pg.teacher_forced_logits(question, targets_in, differentiable=True, constraint=auto)
    assert graph.requires_grad and torch.equal(torch.isfinite(graph), inside)

    # the sampled pass against the teacher-forced pass over its own predictions, and the same gap of "sampling"
    def gap(sampled, forced_loss, rescale):
        pred = sampled["predictions"].cpu().numpy()
        ended = (pred == END).any(1)
        comparable = (pred[:, 0] != PAD) & (ended | rescale)                    # (a row that starts with @end@ is trimmed away)
        # a row of T tokens without an @end@: teacher forcing scores the boundary @end@ behind it as well -- under the grammar
        # at no cost, so its mean over T + 1 steps is the sampled pass's over T, rescaled
        scale = np.where(ended, 1.0, (T + 1.0) / T)
        diff = np.abs(sampled["loss"].detach().double().cpu().numpy() - forced_loss.detach().double().cpu().numpy() * scale)
        return float(diff[comparable].max()), int(comparable.sum())

    torch.manual_seed(11)
    plain_sampled = pg(question, decoding_strategy="sampling")
    plain_forced = pg(question, _own_targets(pg, plain_sampled["predictions"]), decoding_strategy="sampling", need_predictions=False)
    base, n_base = gap(plain_sampled, plain_forced["loss"], False)
    mine, n_mine = gap(out, forced["loss"], True)
    print("sampled loss against the teacher-forced loss of its own predictions: \"sampling\" %.3g over %d rows, "
          "\"grammar_sampling\" %.3g over %d rows (bar %.3g)" % (base, n_base, mine, n_mine, 4 * base + 1e-6))
    assert n_base >= 1 and n_mine >= 2
    assert mine <= 4 * base + 1e-6

    # gradients: finite everywhere, and no gradient at all for the tokens no set ever holds
    for p in pg.parameters():
        p.grad = None
    out["loss"].sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in pg.parameters())
    bias_grad = pg._output_projection_layer.bias.grad
    assert (bias_grad[[PAD, UNK, START]] == 0).all() and float(bias_grad.abs().max()) > 0
    assert float(pg._encoder._module.weight_hh_l0.grad.abs().max()) > 0        # (the graph reaches the encoder)
    for p in pg.parameters():
        p.grad = None


def test_existing_strategies_keep_their_bits(generator):
    """"sampling" and "constrained_sampling" from one seed, before and after a grammar pass in between."""
    pg, question, auto, _ = generator

    def both():
        torch.manual_seed(3)
        a = pg(question, decoding_strategy="sampling")
        b = pg(question, decoding_strategy="constrained_sampling", constraint=auto)
        return a["predictions"], a["loss"].detach(), b["predictions"], b["loss"]

    first = both()
    pg(question, decoding_strategy="grammar_sampling", constraint=auto)["loss"].sum().backward()
    for p in pg.parameters():
        p.grad = None
    assert all(torch.equal(x, y) for x, y in zip(first, both()))


# ---- the trainers ----------------------------------------------------------------------------------------------------------

def _trainer_models(seed, with_nmn):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    dev = torch.device(DEV)
    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    pg, qr, prior = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev), ProgramPrior(vocab, hidden_size=256).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=32).to(dev) if with_nmn else None
    batch = synthetic_batch(vocab, 8, seed=23)
    supervision = batch["supervision"].clone()
    supervision[:4], supervision[4:] = 1, 0
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    dbatch["supervision"] = supervision
    return pg, qr, prior, nmn, dbatch


def _snapshot(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _moved(model, before):
    return [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]


def _all_valid(comp, programs):
    rows = programs.cpu().numpy()
    return all(comp.compile(cc.cut_at_end(row, END)).valid for row in rows)


def test_question_coding_step_under_the_grammar(grammar):
    from probnmn.trainers.joint_training import QuestionCodingStep

    comp, auto = grammar
    pg, qr, prior, _, dbatch = _trainer_models(1, False)
    before = _snapshot(pg), _snapshot(qr)
    step = QuestionCodingStep(pg, qr, prior, constraint=auto)
    assert step._planned_encoder_workgroups(dbatch, torch.arange(4), torch.arange(4, 8)) == 0
    out = step.step(dbatch)
    assert not step.__dict__.get("_plans")                                    # no plan is built
    assert out["programs"].shape[0] == 4 and _all_valid(comp, out["programs"])
    assert int(out["grammar"]["outside"]) == 0 and float(out["grammar"]["log_mass"]) < 0
    assert np.isfinite(float(out["objective"])) and all(np.isfinite(float(v)) for v in out["elbo"].values())
    assert all(np.isfinite(float(v)) for v in out["loss"].values())
    assert len(_moved(pg, before[0])) > 10 and len(_moved(qr, before[1])) > 10
    many = QuestionCodingStep(pg, qr, prior, constraint=auto, num_samples=2)
    out = many.step(dbatch)
    assert out["programs"].shape[0] == 8 and _all_valid(comp, out["programs"]) and np.isfinite(float(out["objective"]))
    step.close(), many.close()


def test_joint_training_step_under_the_grammar(grammar):
    from probnmn.trainers.joint_training import JointTrainingStep

    comp, auto = grammar
    pg, qr, prior, nmn, dbatch = _trainer_models(2, True)
    before = _snapshot(pg), _snapshot(nmn)
    step = JointTrainingStep(pg, qr, prior, nmn, lr=1e-4, constraint=auto)
    out = step.step(dbatch)
    assert not step.__dict__.get("_plans")
    programs = out["programs"].cpu().numpy()
    assert programs.shape[0] == 4 and _all_valid(comp, out["programs"])
    # the NMN ran every unsupervised row: each is a program its compiler accepts, none paid the invalid-program constant
    assert all(c.valid for c in nmn.engine.compiler.compile_batch(programs))
    assert int(out["grammar"]["outside"]) == 0 and float(out["grammar"]["log_mass"]) < 0
    assert np.isfinite(float(out["objective"])) and all(np.isfinite(float(v)) for v in out["elbo"].values())
    assert all(np.isfinite(float(v)) for v in out["loss"].values())
    assert len(_moved(pg, before[0])) > 10 and "classifier.6.weight" in _moved(nmn, before[1])
    step.close()


def test_marginal_joint_step_grammar_normalised():
    from probnmn.trainers import MarginalJointStep

    pg, _, _, nmn, dbatch = _trainer_models(3, True)
    before = _snapshot(pg)
    step = MarginalJointStep(pg, nmn, beam_size=4, constrained=True, grammar_normalised=True, lr=1e-3)
    out = step.step({k: dbatch[k] for k in ("question", "image", "answer")})
    assert out["rows"] >= 8 and np.isfinite(float(out["loss"])) and 1.0 <= float(out["support"]) <= 4.0
    assert len(_moved(pg, before)) > 10
    step.close()
    # q_c >= q on every candidate, so the grammar-normalised loss of the same models is at most the plain one
    a = _trainer_models(3, True)
    b = _trainer_models(3, True)
    feed = {k: dbatch[k] for k in ("question", "image", "answer")}
    plain = MarginalJointStep(a[0], a[3], beam_size=4, constrained=True, lr=1e-3).step(feed)
    normalised = MarginalJointStep(b[0], b[3], beam_size=4, constrained=True, grammar_normalised=True, lr=1e-3).step(feed)
    assert plain["rows"] == normalised["rows"] and float(normalised["loss"]) <= float(plain["loss"]) + 1e-5


def test_without_a_grammar_the_steps_are_unchanged(grammar):
    """``constraint=None`` / ``grammar_normalised=False`` are the steps as they were: the same outputs (the sampled programs,
    every loss term and statistic of the iteration), bit for bit, as a step built without the keywords from the same seed --
    through the launch plan, which a step without a grammar still builds.  (The parameters behind the step are not compared:
    the weight-gradient kernels accumulate with floating-point atomics, so two runs of one step differ in their last bits.)"""
    from probnmn.trainers import MarginalJointStep
    from probnmn.trainers.joint_training import JointTrainingStep, QuestionCodingStep

    def run(make, seed, with_nmn, feed=None):
        pg, qr, prior, nmn, dbatch = _trainer_models(seed, with_nmn)
        step = make(pg, qr, prior, nmn)
        torch.manual_seed(9)
        out = step.step(dbatch if feed is None else {k: dbatch[k] for k in feed})
        plans = bool(step.__dict__.get("_plans"))
        step.close()
        return out, plans

    def same(x, y):
        if isinstance(x, dict):
            return set(x) == set(y) and all(same(x[k], y[k]) for k in x)
        return torch.equal(x, y) if torch.is_tensor(x) else x == y

    pairs = [
        (lambda pg, qr, prior, nmn: QuestionCodingStep(pg, qr, prior), lambda pg, qr, prior, nmn: QuestionCodingStep(pg, qr, prior, constraint=None), False, None),
        (lambda pg, qr, prior, nmn: JointTrainingStep(pg, qr, prior, nmn, lr=1e-4),
         lambda pg, qr, prior, nmn: JointTrainingStep(pg, qr, prior, nmn, lr=1e-4, constraint=None), True, None),
        (lambda pg, qr, prior, nmn: MarginalJointStep(pg, nmn, beam_size=4, constrained=True),
         lambda pg, qr, prior, nmn: MarginalJointStep(pg, nmn, beam_size=4, constrained=True, grammar_normalised=False), True,
         ("question", "image", "answer")),
    ]
    for before, after, with_nmn, feed in pairs:
        a, b = run(before, 4, with_nmn, feed), run(after, 4, with_nmn, feed)
        assert "grammar" not in a[0] and same(a[0], b[0])
        assert a[1] == b[1] and (feed is not None or a[1])  # (the question-coding and joint steps ran their plan)
