"""``pnmn_importance_bound`` and what is built on it, on the MI355X: the kernel against the fp64 reference of
tests/helpers/importance_bound_reference.py over every sample count and vocabulary width at which it takes another path, with
a dominating sample (the cancellation case of the leave-one-out terms) and questions a single row rules out; guard words
around every output; the bits it shares with ``pnmn_hypothesis_posterior``, between its two modes and between a question
alone and in a batch; ``importance_weighted_bound`` under autograd; ``evaluate_question_evidence`` and one
``ImportanceWeightedCodingStep`` on small models.

Tolerances -- derived, not measured.  ``log_px`` / ``log_pz`` / ``log_q``: rtol = atol = 1e-5, the project's bar for
log-softmax sums (tests/test_hypothesis_posterior_gpu.py): at most Tx = 5 (70 in one case) terms (z[tok] - max) - log sum
exp, each a few fp32 ulps (6e-8 relative) of its own size, all of one sign.  log w = lx + beta (lp - lq) combines three such
sums, so it inherits their ABSOLUTE errors: tol_g = 1e-5 (1 + max over the question's rows of |lx| + beta (|lp| + |lq|)), for
``log_weight`` and for ``bound`` (a logsumexp moves by at most the largest error of its arguments; its own rounding is a few
ulps of the result).  ``signal`` = bound - baseline, both within tol_g: 2 tol_g.  ``share`` = exp(log w - logsumexp) <= 1:
its relative error is the absolute error of the exponent, at most 2 tol_g, so 2 tol_g absolute.  ``ess`` = 1 / sum share^2:
squaring doubles the relative error of every share: 4 tol_g relative.  Gradients, coefficient x ce with |ce| <= 1: the
coefficient (share, beta share, signal - beta share) is within 3 tol_g (2 for the signal, 1 for beta share with beta <= 1 --
2 tol_g |share| <= 2 tol_g in absolute terms either way), and ce = softmax - onehot is within 1e-5 relative of itself, hence
|got - ref| <= 3 tol_g + 1e-5 |coefficient| per element.  -inf / finite patterns and ``support`` are compared exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from importance_bound_reference import importance_bound_reference  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)
GUARD = 64          # guard words on either side of every output buffer
SENTINEL = -777.0
G = 37
TX, TP, TQ = 5, 4, 3
SAMPLES = [1, 2, 3, 8, 9, 64]   # no baseline; a mean of one; odd; one row per wave; a wave with two rows; every lane
WIDTHS = [(3, 2), (64, 45), (65, 64), (130, 129), (257, 256), (513, 512), (1024, 1023)]  # the register counts of with_nper
UNSUPPORTED = [g for g in range(G) if g % 8 == 3]
LIFTED = [g for g in range(G) if g % 8 == 1]
PAD = 0


def make_inputs(K, Vx, Vq, seed=0, Tx=TX):
    """37 questions of K rows: logits x 3, a tenth of the rows x 8, a quarter of the tokens padding, some rows all padding.
    Questions g = 1 (mod 8): one sample's log w is lifted 30 nats and more above the others through its logits (its
    reconstruction made near certain, its program unlikely under the generator and free under the prior; the question's
    other rows are not scaled by 8).  Questions g = 3 (mod 8): exactly one row gets a token that is no index, or a -inf at
    a scored target, in one of the three terms.  No other row has either."""
    rng = np.random.default_rng(100000 * Vx + 1000 * K + 10 * Tx + seed)
    R = G * K
    calm = np.repeat(np.arange(G) % 8 == 1, K)          # (the lifted questions: their other rows stay in the usual range)

    def term(T, V):
        logits = (rng.standard_normal((R, T, V)) * 3).astype(np.float32)
        logits[(rng.random(R) < 0.1) & ~calm] *= 8
        tokens = rng.integers(1, V, (R, T)).astype(np.int64)
        tokens[rng.random((R, T)) < 0.25] = PAD
        tokens[rng.random(R) < 0.06] = PAD
        return [logits, tokens, PAD]

    x, p, q = term(Tx, Vx), term(TP, Vq), term(TQ, Vq)
    x[1][R - 1], q[1][0] = PAD, PAD                      # (rows that are all padding, whatever the draw)
    for g in LIFTED:
        r = g * K + int(rng.integers(0, K))
        x[1][r] = rng.integers(1, Vx, Tx)
        q[1][r] = rng.integers(1, Vq, TQ)
        p[1][r] = PAD
        for t in range(Tx):
            x[0][r, t, x[1][r, t]] = np.abs(x[0][r, t]).max() + 40.0
        for t in range(TQ):
            q[0][r, t, q[1][r, t]] = -np.abs(q[0][r, t]).max() - 12.0
    for i, g in enumerate(UNSUPPORTED):
        r = g * K + int(rng.integers(0, K))
        logits, tokens, _ = (x, p, q)[i % 3]
        t, V = int(rng.integers(0, tokens.shape[1])), logits.shape[2]
        if i % 2:
            tokens[r, t] = int(rng.integers(1, V))
            logits[r, t, tokens[r, t]] = -np.inf
        else:
            tokens[r, t] = V + 3 if i % 4 else -2
    return tuple(x), tuple(q), tuple(p)


def launch(x, q, p, beta, K, grad=(False, False, False), optional=True):
    """One ``pnmn_importance_bound`` launch on numpy inputs; every output lies between GUARD sentinel words, which must come
    back untouched, and is itself filled with the sentinel first.  The token rows are handed over with a stride wider than T.
    ``grad`` = which of d_x / d_p / d_q are asked for.  Returns the outputs as numpy."""
    from probnmn import _hip, _hip_importance

    dev = torch.device("cuda:0")
    R = len(x[0])
    n = R // K
    keep = []

    def term(t):
        if t is None:
            return [0, 0, 0, 0, 0, 0], 1
        logits, tokens, pad = t
        wide = torch.full((R, tokens.shape[1] + 2), 12345, dtype=torch.long)
        wide[:, :tokens.shape[1]] = torch.from_numpy(np.ascontiguousarray(tokens))
        d_logits, d_tokens = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev), wide.to(dev)
        keep.extend((d_logits, d_tokens))
        return [d_logits.data_ptr(), d_tokens.data_ptr(), wide.stride(0), pad, logits.shape[1], logits.shape[2]], logits[0].size

    (x_args, x_words), (p_args, p_words), (q_args, q_words) = term(x), term(p), term(q)
    f32 = lambda size: torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
    bufs = {name: f32(R) for name in ("log_px", "log_pz", "log_q", "log_weight", "share", "signal")}
    bufs.update(bound=f32(n), ess=f32(n), support=torch.full((n + 2 * GUARD,), int(SENTINEL), dtype=torch.int32, device=dev))
    for name, want, words in zip(("d_x", "d_p", "d_q"), grad, (x_words, p_words, q_words)):
        if want:
            bufs[name] = f32(R * words)
    ptr = lambda name: bufs[name][GUARD:].data_ptr() if name in bufs else 0  # noqa: E731
    opt = lambda name: ptr(name) if optional else 0  # noqa: E731
    rc = _hip_importance.lib().pnmn_importance_bound(
        *x_args, *p_args, *q_args, float(beta), n, K, opt("log_px"), opt("log_pz"), opt("log_q"), ptr("log_weight"), ptr("share"),
        ptr("signal"), ptr("bound"), opt("ess"), opt("support"), ptr("d_x"), ptr("d_p"), ptr("d_q"), _hip.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), name
        out[name] = host[GUARD:-GUARD]
    for name, t in (("d_x", x), ("d_p", p), ("d_q", q)):
        if name in out:
            out[name] = out[name].reshape(t[0].shape)
    return out


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def check_against_reference(got, ref, x, q, p, beta, K, label=""):
    tol_g = 1e-5 * (1.0 + ref["scale"])
    tol_r = np.repeat(tol_g, K)
    counts = ref["support"] == K
    rows = np.repeat(counts, K)
    for name in ("log_px", "log_pz", "log_q"):
        if ref[name] is None:
            assert (got[name] == SENTINEL).all(), name          # (a term that is left out is not written)
            continue
        inf = np.isneginf(ref[name])
        assert np.array_equal(np.isneginf(got[name]), inf) and not np.isnan(got[name]).any(), name
        np.testing.assert_allclose(got[name][~inf], ref[name][~inf], err_msg=name, **TOL)
    assert np.array_equal(got["support"], ref["support"])
    fin = np.isfinite(ref["log_weight"])
    assert np.array_equal(np.isfinite(got["log_weight"]), fin) and np.isneginf(got["log_weight"][~fin]).all()
    worst = {"log_weight": (np.abs(got["log_weight"][fin] - ref["log_weight"][fin]) / tol_r[fin]).max(),
             "bound": (np.abs(got["bound"][counts] - ref["bound"][counts]) / tol_g[counts]).max(),
             "signal": (np.abs(got["signal"] - ref["signal"]) / (2 * tol_r)).max(),
             "share": (np.abs(got["share"] - ref["share"]) / (2 * tol_r)).max(),
             "ess": (np.abs(got["ess"][counts] - ref["ess"][counts]) / (4 * tol_g[counts] * ref["ess"][counts])).max()}
    assert np.isneginf(got["bound"][~counts]).all() and (got["ess"][~counts] == 0).all()
    assert (got["share"][~rows] == 0).all() and (got["signal"][~rows] == 0).all()
    for name, term in (("d_x", x), ("d_p", p), ("d_q", q)):
        if name not in got:
            continue
        d, want, c = got[name], ref[name], np.abs(ref["coefficient_" + name[-1]])
        assert not (bits(d) == bits(np.float32(SENTINEL))).any(), name        # every word was written
        scored = (term[1] != term[2]) & (term[1] >= 0) & (term[1] < term[0].shape[2])
        assert (d[~scored] == 0).all() and (d[~rows] == 0).all(), name         # padding steps, unsupported questions: zeros
        bar = (3 * tol_r + 1e-5 * c)[:, None, None]
        worst[name] = (np.abs(d - want) / bar).max()
    print("%s largest error / tolerance: %s" % (label, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def run_case(K, Vx, Vq, beta=1.0, Tx=TX, prior=True):
    x, q, p = make_inputs(K, Vx, Vq, Tx=Tx)
    p = p if prior else None
    ref = importance_bound_reference(x, q, p, beta, K, gradients=True)
    # what the inputs are required to hold, on the reference alone: the comparison below leaves out no other question
    # (the marked row's term is x, p, q in turn: a term that is left out of log w rules nothing out)
    enters = (True, p is not None and beta != 0.0, beta != 0.0)
    ruled_out = [g for i, g in enumerate(UNSUPPORTED) if enters[i % 3]]
    assert ref["support"].tolist() == [K - 1 if g in ruled_out else K for g in range(G)]
    assert sum(g % 8 == 3 for g in range(G)) == 5 == -(-G // 8)
    assert all((t[1] == PAD).all(1).any() and (t[1] == PAD).mean() > 0.15 for t in (x, q))
    if K > 1 and beta == 1.0:
        lw = np.sort(ref["log_weight"].reshape(G, K)[LIFTED], axis=1)
        print("lifted questions: the largest log w leads the next by %.1f .. %.1f nats" % ((lw[:, -1] - lw[:, -2]).min(), (lw[:, -1] - lw[:, -2]).max()))
        assert (lw[:, -1] - lw[:, -2] >= 25.0).all()    # one sample dominates: totals minus the sample would cancel
    grads = (True, p is not None, True)
    got = launch(x, q, p, beta, K, grad=grads)
    check_against_reference(got, ref, x, q, p, beta, K, "K = %d, V = (%d, %d), beta = %g:" % (K, Vx, Vq, beta))
    # the plain launch: the outputs the two modes share are the same bits
    plain = launch(x, q, p, beta, K)
    for name in plain:
        assert np.array_equal(bits(plain[name]), bits(got[name])), name
    return x, q, p, got


@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("K", SAMPLES)
def test_kernel_against_fp64_reference(K, V):
    run_case(K, *V)


def test_second_block_of_steps():
    run_case(3, 3, 2, Tx=70)  # (take_steps reads the tokens 64 at a time: steps 64 .. 69 are the second block)


@pytest.mark.parametrize("beta,prior", [(0.1, True), (0.0, True), (1.0, False), (0.0, False)])
def test_terms_left_out(beta, prior):
    """beta = 0.1; beta = 0 (the prior's term is not read and not reported, its gradient is zeros; the generator's leaves
    log w but keeps its signal); no prior at all."""
    x, q, p, got = run_case(9, 65, 64, beta=beta, prior=prior)
    if beta == 0.0:
        assert np.array_equal(bits(got["log_weight"][np.isfinite(got["log_weight"])]), bits(got["log_px"][np.isfinite(got["log_weight"])]))
        if prior:
            assert (got["d_p"] == 0).all()
        # a null prior equals a zero beta, bit for bit
        other = launch(x, q, None if prior else make_inputs(9, 65, 64)[2], 0.0, 9, grad=(True, False, True))
        for name in ("log_weight", "share", "signal", "bound", "ess", "support", "d_x", "d_q"):
            assert np.array_equal(bits(other[name]), bits(got[name])), name


def test_log_px_is_the_posterior_kernels_bit_for_bit():
    from test_hypothesis_posterior_gpu import launch as posterior_launch

    for K, V in ((3, (3, 2)), (9, (65, 64)), (8, (257, 256)), (2, (1024, 1023))):
        x, q, p = make_inputs(K, *V)
        got = launch(x, q, p, 1.0, K)
        start = np.arange(G + 1) * K
        theirs = posterior_launch(x, p, None, start, (1.0, 1.0, 0.0))
        assert np.array_equal(bits(theirs["log_px"]), bits(got["log_px"])) and np.isneginf(got["log_px"]).any() == np.isneginf(theirs["log_px"]).any()
        assert np.array_equal(bits(theirs["log_pz"]), bits(got["log_pz"]))
        theirs = posterior_launch(q, None, None, start, (1.0, 0.0, 0.0))
        assert np.array_equal(bits(theirs["log_px"]), bits(got["log_q"]))


def test_a_question_is_the_same_bits_alone_and_in_a_batch():
    for K, V in ((9, (65, 64)), (64, (130, 129)), (1, (64, 45))):
        x, q, p = make_inputs(K, *V)
        whole = launch(x, q, p, 1.0, K, grad=(True, True, True))
        again = launch(x, q, p, 1.0, K, grad=(True, True, True))
        for name in whole:
            assert np.array_equal(bits(whole[name]), bits(again[name])), name
        for g in (0, 1, 3, 9, 11, 20, 36):
            lo, hi = g * K, (g + 1) * K
            cut = lambda t: (t[0][lo:hi], t[1][lo:hi], t[2])  # noqa: E731
            alone = launch(cut(x), cut(q), cut(p), 1.0, K, grad=(True, True, True))
            for name in ("log_px", "log_pz", "log_q", "log_weight", "share", "signal", "d_x", "d_p", "d_q"):
                assert np.array_equal(bits(alone[name]), bits(whole[name][lo:hi])), (K, g, name)
            for name in ("bound", "ess", "support"):
                assert bits(alone[name])[0] == bits(whole[name])[g], (K, g, name)


def test_a_wider_vocabulary_than_the_widest_kernel_holds_returns_without_a_launch():
    from probnmn import _hip, _hip_importance

    dev = torch.device("cuda:0")
    out = torch.full((2 * 3 * 1025,), SENTINEL, device=dev)
    a = out.data_ptr()
    for Vx, Vp, Vq in ((1025, 4, 4), (4, 1025, 4), (4, 4, 1025)):
        rc = _hip_importance.lib().pnmn_importance_bound(a, a, 3, 0, 3, Vx, a, a, 3, 0, 3, Vp, a, a, 3, 0, 3, Vq, 1.0, 1, 2, 0, 0, 0,
                                                         a, a, a, a, 0, 0, 0, 0, 0, _hip.stream_ptr(dev))
        assert rc == _hip.ESHAPE
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()  # nothing ran


# ---- under autograd ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prior_needs_grad", [True, False])
def test_importance_weighted_bound_under_autograd(prior_needs_grad):
    from probnmn.models.nmn import INVALID_PROGRAM_LOSS
    from probnmn.modules.importance_weighted import importance_weighted_bound

    dev = torch.device("cuda:0")
    K, beta = 3, 0.5
    x, q, p = make_inputs(K, 65, 64)
    ref = importance_bound_reference(x, q, p, beta, K, gradients=True)

    def on_device(t, needs_grad):
        return (torch.from_numpy(t[0]).to(dev).requires_grad_(needs_grad), torch.from_numpy(t[1]).to(dev), t[2])

    dx, dq, dp = on_device(x, True), on_device(q, True), on_device(p, prior_needs_grad)
    loss, stats = importance_weighted_bound(dx, dq, dp, samples=K, beta=beta)
    assert set(stats) == {"log_weight", "share", "signal", "ess", "support", "log_px", "log_pz", "log_q"}
    assert not any(v.requires_grad for v in stats.values()) and loss.requires_grad and loss.shape == (G,)
    saved = loss.grad_fn.saved_tensors
    assert saved[0] is not None and saved[2] is not None and (saved[1] is not None) == prior_needs_grad  # no buffer unasked
    counts = ref["support"] == K
    tol_g = 1e-5 * (1.0 + ref["scale"])
    host = loss.detach().cpu().numpy()
    assert (host[~counts] == np.float32(INVALID_PROGRAM_LOSS)).all()
    assert (np.abs(-host[counts] - ref["bound"][counts]) <= tol_g[counts]).all()
    assert np.array_equal(stats["support"].cpu().numpy(), ref["support"])
    loss.sum().backward(retain_graph=True)
    tol_r = np.repeat(tol_g, K)
    first = {}
    for name, t in (("x", dx), ("q", dq), ("p", dp)):
        if t[0].grad is None:
            assert name == "p" and not prior_needs_grad
            continue
        got = t[0].grad.cpu().numpy()
        bar = (3 * tol_r + 1e-5 * np.abs(ref["coefficient_" + name]))[:, None, None]
        assert (np.abs(got - ref["d_" + name]) <= bar).all(), name
        assert (got[np.repeat(~counts, K)] == 0).all()
        first[name], t[0].grad = t[0].grad.clone(), None
    # a dloss per question: one multiply per term backward
    weights = torch.linspace(0.5, 2.0, G, device=dev)
    (loss * weights).sum().backward()
    for name, t in (("x", dx), ("q", dq), ("p", dp)):
        if name in first:
            torch.testing.assert_close(t[0].grad, first[name] * weights.repeat_interleave(K).view(-1, 1, 1), rtol=1e-6, atol=0)
    # nothing requires a gradient: the plain launch, the same bits
    plain, plain_stats = importance_weighted_bound(on_device(x, False), on_device(q, False), on_device(p, False), samples=K, beta=beta)
    assert not plain.requires_grad and torch.equal(plain, loss.detach())
    for name in stats:
        assert torch.equal(plain_stats[name], stats[name]) or name == "log_pz" and torch.equal(plain_stats[name].isnan(), stats[name].isnan())
    # no prior: its statistic is NaN
    none = importance_weighted_bound(on_device(x, False), on_device(q, False), None, samples=K, beta=beta)[1]
    assert torch.isnan(none["log_pz"]).all()


# ---- the models ------------------------------------------------------------------------------------------------------------

def _models(dev, seed=0):
    from probnmn.models import ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    pg, qr = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev)
    return vocab, pg, qr, prior


def _constraint(vocab, pg):
    from probnmn.runtime.program_compiler import ProgramCompiler

    compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    exclude = [getattr(pg, n) for n in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
    return compiler, compiler.decoding_automaton(exclude=exclude)


@pytest.fixture(scope="module")
def models():
    from probnmn.data.synthetic import synthetic_batch

    dev = torch.device("cuda:0")
    vocab, pg, qr, prior = _models(dev)
    return vocab, pg, qr, prior, synthetic_batch(vocab, 8, seed=31), dev


def test_evaluate_question_evidence(models):
    from probnmn.evaluators import evaluate_question_evidence

    vocab, pg, qr, prior, batch, dev = models
    batches = [{"question": batch["question"][s].to(dev)} for s in (slice(0, 4), slice(4, 8))]
    # metrics on record, one model in each mode
    qr.eval(), prior.eval()
    with torch.no_grad():
        qr(batch["program"].to(dev), batch["question"].to(dev))
        prior(batch["program"].to(dev))
    qr.get_metrics(reset=False)
    before = (qr.get_metrics(reset=False), prior._log2_perplexity._count, qr._log2_perplexity._count, qr._sequence_accuracy._count)
    pg.train(), prior.train()
    params = [p.detach().clone() for m in (pg, qr, prior) for p in m.parameters()]

    torch.manual_seed(5)
    one = evaluate_question_evidence(pg, qr, prior, batches, num_samples=1)
    assert one["log_evidence_bound"] == one["elbo"] and one["questions"] == 8 and one["unsupported"] == 0
    assert one["effective_sample_size"] == 1.0 and one["bound"].shape == (8,)
    torch.manual_seed(6)
    four = evaluate_question_evidence(pg, qr, prior, batches, num_samples=4)
    log_w = four["log_weight"].double()
    assert log_w.shape == (8, 4) and four["questions"] == 8 and four["unsupported"] == 0
    tol = 1e-5 * (1 + log_w.abs().max(1).values)   # (at most tol_g: |log w| <= |lx| + |lp| + |lq|)
    assert (four["bound"].double() >= log_w.mean(1) - tol).all()
    assert four["log_evidence_bound"] >= four["elbo"] - float(tol.max()) and 1.0 <= four["effective_sample_size"] <= 4.0
    assert four["log_evidence_bound"] == pytest.approx(float(four["bound"].double().mean()), rel=1e-6)
    assert four["elbo"] == pytest.approx(float(log_w.mean()), rel=1e-6)
    torch.manual_seed(6)
    again = evaluate_question_evidence(pg, qr, prior, batches, num_samples=4)
    assert torch.equal(again["bound"], four["bound"]) and again["elbo"] == four["elbo"]          # reproducible under the seed
    # under the grammar: scored under the distribution the constrained draw came from
    _, automaton = _constraint(vocab, pg)
    torch.manual_seed(7)
    valid = evaluate_question_evidence(pg, qr, prior, batches, num_samples=2, constraint=automaton)
    assert valid["unsupported"] == 0 and torch.isfinite(valid["bound"]).all()

    assert pg.training and not qr.training and prior.training                                    # the modes are back
    assert (qr.get_metrics(reset=False), prior._log2_perplexity._count, qr._log2_perplexity._count, qr._sequence_accuracy._count) == before
    assert all(torch.equal(a, b) for a, b in zip(params, (p for m in (pg, qr, prior) for p in m.parameters())))
    qr.train()


@pytest.mark.parametrize("constrained", [False, True])
def test_one_importance_weighted_coding_step(constrained):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator
    from probnmn.trainers import ImportanceWeightedCodingStep

    dev = torch.device("cuda:0")
    vocab, pg, qr, prior = _models(dev, seed=1)
    compiler, automaton = _constraint(vocab, pg)
    batch = synthetic_batch(vocab, 8, seed=31)
    supervision = torch.tensor([1, 1, 0, 0, 0, 1, 0, 0])
    dbatch = {"question": batch["question"].to(dev), "program": batch["program"].to(dev), "supervision": supervision}
    before = [[p.detach().clone() for p in m.parameters()] for m in (pg, qr, prior)]
    K, alpha = 4, 100.0
    step = ImportanceWeightedCodingStep(pg, qr, prior, num_samples=K, beta=1.0, alpha=alpha, constraint=automaton if constrained else None)
    torch.manual_seed(3)
    out = step.step(dbatch)
    torch.cuda.synchronize()
    for key in ("objective", "bound", "effective_sample_size", "signal_variance", "unsupported", "programs",
                "samples_per_question", "loss"):
        assert key in out, key
    assert out["samples_per_question"] == K and out["programs"].shape[0] == 5 * K and int(out["unsupported"]) == 0
    values = [out["objective"], out["bound"], out["effective_sample_size"], out["signal_variance"], *out["loss"].values()]
    assert all(torch.isfinite(v).all() for v in values)
    assert 1.0 <= float(out["effective_sample_size"]) <= K and float(out["signal_variance"]) >= 0.0
    # the objective is the two terms it reports: alpha x the supervised cross entropies, minus the mean bound
    want = alpha * (float(out["loss"]["program_generation_gt"]) + float(out["loss"]["question_reconstruction_gt"])) - float(out["bound"])
    assert float(out["objective"]) == pytest.approx(want, rel=1e-5)
    moved = [[not torch.equal(a, b) for a, b in zip(old, m.parameters())] for old, m in zip(before, (pg, qr, prior))]
    assert any(moved[0]) and any(moved[1])                  # the generator and the reconstructor learn
    assert not any(moved[2]) and not prior.training        # the prior is frozen, bit for bit
    assert all(p.grad is None for p in prior.parameters())
    if constrained:
        assert all(c.valid for c in compiler.compile_batch(out["programs"].cpu().numpy()))
    with pytest.raises(ValueError):
        ImportanceWeightedCodingStep(ProgramGenerator(vocab, dropout=0.2).to(dev), qr, prior)
    step.close()
