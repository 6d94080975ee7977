"""Stochastic beam search on the device (``pnmn_attn_lstm_beam_stochastic``, ``decoding_strategy="stochastic_beam"``) against
the fp64 host statement of its rule (tests/stochastic_beam_ref.py), on the models and sources of tests/test_beam_gpu.py.

The main check REPLAYS the device's own prefixes in fp64 (tests/helpers/beam_reference.py runs the network) and recomputes
phi and G~ of every candidate from the helper's uniforms: per step (a) every chosen G~ >= every unchosen one - TOL_G,
(b) best first within TOL_G, (c) the traced phi within tol_t = 1e-4 (t + 1) of fp64 -- the project's beam bar --, (d) the
traced G within TOL_G of fp64.

TOL_G: G~ is steep in g near the arg-max child when the parent's G exceeds Z, so the bar comes from a measurement, not
from the format: the worst |G_device - G_fp64| of exactly these inputs on an MI355X was 6.68e-5 (trained model, K = 8), and TOL_G is
four times that, to cover other seeds.  The worst |phi_device - phi_fp64| of the same run was 0.056 tol_t; (a) and (b) were
never violated at all."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import beam_reference as br  # noqa: E402
import stochastic_beam_ref as ref  # noqa: E402

from oracle.seq2seq_oracle import END, PAD, START, UNK, trim_predictions  # noqa: E402

pytestmark = pytest.mark.gpu

NEG = float("-inf")
STEPS = 26
WORST_G = 6.68e-5  # worst |G_device - G_fp64| of the replay cases below, measured on an MI355X
TOL_G = 4 * WORST_G
SEED = 0x5EED5EED5EED
EXCLUDE = (PAD, UNK, START, END)


@pytest.fixture(scope="module")
def vocab():
    from probnmn.vocabulary import Vocabulary

    return Vocabulary.clevr()


@pytest.fixture(scope="module")
def models(vocab):
    """{"untrained" | "trained" | "peaked": host state_dict} of the ProgramGenerator fixture of tests/test_beam_gpu.py (seed
    0, 100 Adam steps on the host: its hypotheses end on at least four different steps); "peaked": the trained one with
    its output layer scaled by 8.  And a factory of device models from them."""
    from probnmn.models import ProgramGenerator

    v_src, v_tgt = vocab.get_vocab_size("questions"), vocab.get_vocab_size("programs")
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, max(1, threads)))
    try:
        torch.manual_seed(0)
        fresh = {k: v.detach().clone() for k, v in ProgramGenerator(vocab, max_decoding_steps=12).state_dict().items()}
        trained = br.train_on_host(fresh, v_src, v_tgt, steps=100, rows=64)
    finally:
        torch.set_num_threads(threads)
    src, _ = br.synthetic_task(v_src, v_tgt, 128, torch.Generator().manual_seed(99))
    ends = br.first_end_steps(br.beam_search(trained, src, 4, 12)["tokens"])
    assert len(set(ends.reshape(-1).tolist())) >= 4, "fixture: first @end@ on fewer than four different steps"
    peaked = {k: v.clone() for k, v in trained.items()}
    for name in ("_output_projection_layer.weight", "_output_projection_layer.bias"):
        peaked[name] = peaked[name] * 8.0
    sds = {"untrained": fresh, "trained": trained, "peaked": peaked}
    cache = {}

    def device_model(which, steps=STEPS):
        if (which, steps) not in cache:
            model = ProgramGenerator(vocab, max_decoding_steps=steps)
            model.load_state_dict(sds[which])
            cache[(which, steps)] = model.to("cuda:0").eval()
        return cache[(which, steps)]

    return sds, device_model, v_src, v_tgt


def _sources(v_src, v_tgt, rows, seed, long=False):
    gen = torch.Generator().manual_seed(seed)
    if not long:
        return br.synthetic_task(v_src, v_tgt, rows, gen)[0]
    src = torch.zeros(rows, 40, dtype=torch.long)
    for r in range(rows):
        n = int(torch.randint(3, 41, (1,), generator=gen))
        src[r, :n] = torch.randint(4, v_src, (n,), generator=gen)
    return src


def _decode(model, src, K, seed=SEED, offset=0, constraint=None, trace=True):
    model.sample_row_offset = offset
    try:
        out = model.decode_stochastic_beam(model.encode(src.to("cuda:0"), dropout=False), K, seed=seed, trace=trace,
                                           constraint=constraint)
    finally:
        model.sample_row_offset = 0
    torch.cuda.synchronize()
    flat = {k: v.cpu() for k, v in out.items() if k != "beam_trace"}
    if trace:
        flat.update({"trace_" + k: v.cpu() for k, v in out["beam_trace"].items()})
    return flat


def _replay_check(sd, src, out, K, V, seed, offset, tol_g):
    """The conditions of the replay check on one batch; returns (worst |G - G_fp64|, worst |phi - phi_fp64| / tol_t, worst
    (a) / (b) violation)."""
    tok, bp = out["trace_tokens"].long(), out["trace_backpointers"].long()
    sc, pg = out["trace_scores"], out["trace_perturbed"]
    B, T, _ = tok.shape
    assert int(tok.min()) >= 0 and int(tok.max()) < V and int(bp.min()) >= 0 and int(bp.max()) < K
    assert not bool(((tok == PAD) | (tok == UNK) | (tok == START)).any())
    sd = br._cast(sd, torch.float64)
    enc, fmask, h0 = br.encode(sd, src)
    h = h0.unsqueeze(1).expand(B, K, -1).contiguous()
    c = torch.zeros_like(h)
    last = torch.full((B, K), START, dtype=torch.long)
    phi = np.full((B, K), NEG)
    phi[:, 0] = 0.0
    G = phi.copy()
    question = offset + np.arange(B)
    worst_g = worst_phi = worst_order = 0.0
    for t in range(T):
        # log-softmax over the whole vocabulary with pad / unk / start removed (score 0: the table is the row itself); the
        # helper renormalises over what is offered, which is the softmax restricted to the offered tokens
        h2, c2, cand = br.candidates(sd, enc, fmask, h, c, last, torch.zeros(B, K, dtype=torch.float64))
        logp = cand.view(B, K, V).numpy()
        finished = (last == END).numpy()
        u = ref.uniforms(seed, question, K, V, t)
        phi_c, gt = ref.candidates(phi, G, finished, logp, np.isfinite(logp), u, END)
        tk, b_ = tok[:, t].numpy(), bp[:, t].numpy()
        live = (sc[:, t] > NEG).numpy()
        assert np.array_equal(live, (pg[:, t] > NEG).numpy())
        assert bool((tk[~live] == END).all()) and bool((b_[~live] == 0).all()) and bool((live[:, :-1] | ~live[:, 1:]).all())
        flat = b_ * V + tk
        chosen_g = np.where(live, np.take_along_axis(gt.reshape(B, -1), flat, 1), NEG)
        chosen_p = np.where(live, np.take_along_axis(phi_c.reshape(B, -1), flat, 1), NEG)
        assert bool(np.isfinite(chosen_g[live]).all()), "step %d: a chosen candidate the reference rules out" % t
        for b in range(B):
            f = flat[b][live[b]].tolist()
            assert len(set(f)) == len(f), (t, b, f)
        rest = gt.reshape(B, -1).copy()
        np.put_along_axis(rest, np.where(live, flat, flat[:, :1]), NEG, 1)
        best_rest = rest.max(1)
        worst_chosen = np.where(live, chosen_g, np.inf).min(1)
        gap = np.where(best_rest == NEG, 0.0, best_rest - worst_chosen)  # (a)
        assert bool((best_rest[~live.all(1)] == NEG).all())  # an empty slot: nothing finite was left
        with np.errstate(invalid="ignore"):
            order = np.where(live[:, 1:], chosen_g[:, 1:] - chosen_g[:, :-1], 0.0)  # (b)
        worst_order = max(worst_order, float(gap.max()), float(order.max()) if K > 1 else 0.0)
        err_p = np.abs(sc[:, t].double().numpy() - chosen_p)[live]  # (c)
        err_g = np.abs(pg[:, t].double().numpy() - chosen_g)[live]  # (d)
        worst_phi = max(worst_phi, float(err_p.max()) / (1e-4 * (t + 1)))
        worst_g = max(worst_g, float(err_g.max()))
        assert float(err_p.max()) <= 1e-4 * (t + 1), "step %d: (c) worst %g x tol_t" % (t, float(err_p.max()) / (1e-4 * (t + 1)))
        assert float(gap.max()) <= tol_g, "step %d: (a) %g" % (t, float(gap.max()))
        assert K == 1 or float(order.max()) <= tol_g, "step %d: (b) %g" % (t, float(order.max()))
        assert float(err_g.max()) <= tol_g, "step %d: (d) %g" % (t, float(err_g.max()))
        # a finished slot extends only by @end@ with phi and G unchanged, bit for bit
        if t > 0:
            parent_tok = np.take_along_axis(tok[:, t - 1].numpy(), b_, 1)
            ext = live & (parent_tok == END)
            assert bool((tk[ext] == END).all())
            assert np.array_equal(sc[:, t].numpy()[ext], np.take_along_axis(sc[:, t - 1].numpy(), b_, 1)[ext])
            assert np.array_equal(pg[:, t].numpy()[ext], np.take_along_axis(pg[:, t - 1].numpy(), b_, 1)[ext])
        phi, G = chosen_p, chosen_g
        h, c = br._advance(h2, c2, tok[:, t], bp[:, t])
        last = tok[:, t]
    raw = br.backtrack(tok, bp)
    assert torch.equal(out["beam_predictions"], trim_predictions(raw.view(B * K, T)).view(B, K, T))
    assert torch.equal(out["beam_log_probabilities"], sc[:, -1]) and torch.equal(out["beam_perturbed"], pg[:, -1])
    assert torch.equal(out["predictions"], out["beam_predictions"][:, 0])
    return worst_g, worst_phi, worst_order


REPLAY_CASES = [(which, K, B, STEPS) for which in ("untrained", "trained") for K, B in ((1, 17), (2, 9), (4, 5), (8, 3), (16, 3))]
REPLAY_CASES.append(("trained", 4, 5, 64))


@pytest.mark.parametrize("which,K,B,steps", REPLAY_CASES)
def test_replay_of_the_device_prefixes(models, which, K, B, steps):
    sds, device_model, v_src, v_tgt = models
    src = _sources(v_src, v_tgt, B, 7 + B + K, long=which == "untrained")
    out = _decode(device_model(which, steps), src, K, offset=3)
    assert out["trace_tokens"].shape == (B, steps, K)
    worst = _replay_check(sds[which], src, out, K, v_tgt, SEED, 3, TOL_G)
    print("replay %s K=%d B=%d T=%d: worst |G - G64| %.3g, worst phi error %.4f x tol_t, worst order violation %.3g"
          % ((which, K, B, steps) + worst))
    if which == "trained":
        assert int((br.first_end_steps(br.backtrack(out["trace_tokens"].long(), out["trace_backpointers"].long())) < steps).sum()) > 0


def _distinct(beams, finite):
    """Per question: how many of its finite hypotheses there are, and how many different token rows they are."""
    n, d = [], []
    for b in range(beams.size(0)):
        rows = [tuple(beams[b, k].tolist()) for k in range(beams.size(1)) if finite[b, k]]
        n.append(len(rows)), d.append(len(set(rows)))
    return n, d


def test_without_replacement_where_samples_repeat(models):
    sds, device_model, v_src, v_tgt = models
    model = device_model("peaked", 12)
    src = _sources(v_src, v_tgt, 32, 41)
    out = _decode(model, src, 8, trace=False)
    n, d = _distinct(out["beam_predictions"], torch.isfinite(out["beam_log_probabilities"]))
    assert n == d, "a question holds the same program twice"
    assert min(n) >= 2
    torch.manual_seed(17)
    with torch.no_grad():
        drawn = model(src.to("cuda:0").repeat_interleave(8, 0))["predictions"].cpu().view(32, 8, -1)
    _, d_with = _distinct(drawn, torch.ones(32, 8, dtype=torch.bool))
    print("peaked generator, 8 programs per question: distinct without replacement %s, with replacement %s" % (d, d_with))
    assert min(d_with) < 8, "fixture too flat: num_programs=8 never repeats a program"


def _chi_square(counts, expected, variance_scale=None):
    big = expected >= 50
    assert int(big.sum()) >= 10
    var = expected if variance_scale is None else expected * variance_scale
    z = (counts[big] - expected[big]) / np.sqrt(var[big])
    return float((z ** 2).sum()), ref.chi_square_quantile(int(big.sum())), float(np.abs(z).max())


def test_distribution_of_the_draws(models, vocab):
    """One source row 4096 times: the rows differ only by question_offset + b.  K = 2 at one step: a token is included with
    probability p_i + sum_{j != i} p_j p_i / (1 - p_j); K = 4 at three steps: the first token of hypothesis 0 follows p."""
    sds, device_model, v_src, v_tgt = models
    n = 4096
    one = _sources(v_src, v_tgt, 1, 5, long=True)
    sd = br._cast(sds["untrained"], torch.float64)
    enc, fmask, h0 = br.encode(sd, one)
    _, _, cand = br.candidates(sd, enc, fmask, h0.unsqueeze(1), torch.zeros(1, 1, h0.size(1), dtype=torch.float64),
                               torch.full((1, 1), START), torch.zeros(1, 1, dtype=torch.float64))
    logp = cand.view(-1).numpy()
    p = np.where(np.isfinite(logp), np.exp(logp), 0.0)
    p = p / p.sum()  # the softmax restricted to the offered tokens
    src = one.repeat(n, 1)
    out = _decode(device_model("untrained", 1), src, 2, seed=99, offset=1000, trace=False)
    first = out["beam_predictions"][:, :, 0].numpy()
    first = np.where(first == PAD, END, first)  # (trimmed: a hypothesis that ends at once is all padding)
    assert bool((first[:, 0] != first[:, 1]).all())
    pi = p + np.array([sum(p[j] * p[i] / (1.0 - p[j]) for j in range(v_tgt) if j != i) for i in range(v_tgt)])
    counts = np.bincount(first.reshape(-1), minlength=v_tgt).astype(np.float64)
    assert bool((counts[p == 0] == 0).all())
    stat, bar, worst = _chi_square(counts, n * pi, variance_scale=1.0 - pi)
    print("inclusion at K=2: chi-square %.1f (bar %.1f), largest |z| %.2f" % (stat, bar, worst))
    assert stat < bar
    out = _decode(device_model("untrained", 3), src, 4, seed=100, offset=77, trace=False)
    first = out["beam_predictions"][:, 0, 0].numpy()
    counts = np.bincount(np.where(first == PAD, END, first), minlength=v_tgt).astype(np.float64)
    stat, bar, worst = _chi_square(counts, n * p)
    print("first token of hypothesis 0 at K=4: chi-square %.1f (bar %.1f), largest |z| %.2f" % (stat, bar, worst))
    assert stat < bar


KEYS = ("beam_predictions", "beam_log_probabilities", "beam_perturbed", "predictions", "loss")


def test_same_bits_alone_or_in_a_batch(models):
    sds, device_model, v_src, v_tgt = models
    model = device_model("trained")
    src = _sources(v_src, v_tgt, 12, 3)
    for K in (2, 8):
        whole = _decode(model, src, K, trace=False)
        part = _decode(model, src[5:10], K, offset=5, trace=False)
        for key in KEYS:
            assert torch.equal(whole[key][5:10], part[key]), (K, key)
        again = _decode(model, src, K, trace=False)
        other = _decode(model, src, K, seed=SEED + 1, trace=False)
        assert all(torch.equal(whole[key], again[key]) for key in KEYS)
        assert not torch.equal(whole["beam_perturbed"], other["beam_perturbed"])
        assert not torch.equal(whole["beam_predictions"], other["beam_predictions"])
    # seed=None: one draw from torch's CPU generator, as the sampling decode
    state = model.encode(src.to("cuda:0"), dropout=False)
    torch.manual_seed(5)
    a = model.decode_stochastic_beam(state, 4)["beam_predictions"]
    after = torch.get_rng_state()
    torch.manual_seed(5)
    want = int(torch.randint(0, 2 ** 62, (1,)))
    assert torch.equal(torch.get_rng_state(), after)
    assert torch.equal(model.decode_stochastic_beam(state, 4, seed=want)["beam_predictions"], a)
    via_forward = model(src.to("cuda:0"), decoding_strategy="stochastic_beam", beam_size=4)
    assert set(via_forward) == {"predictions", "loss", "beam_predictions", "beam_log_probabilities", "beam_perturbed"}


def test_under_the_program_automaton_every_hypothesis_is_valid(models, vocab):
    from probnmn.runtime.program_compiler import DecodingAutomaton, ProgramCompiler

    sds, device_model, v_src, v_tgt = models
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    auto = comp.decoding_automaton(exclude=EXCLUDE)
    src = _sources(v_src, v_tgt, 20, 23, long=True)
    out = _decode(device_model("untrained"), src, 4, constraint=auto, trace=False)
    finite = torch.isfinite(out["beam_log_probabilities"])
    assert bool(finite[:, 0].all()) and bool((finite == torch.isfinite(out["beam_perturbed"])).all())
    rows = out["beam_predictions"][finite]
    assert rows.size(0) >= 40 and all(c.valid for c in comp.compile_batch(rows.numpy()))
    n, d = _distinct(out["beam_predictions"], finite)
    assert n == d
    # one state, one class, min_left = {0}: the call without tables, bit for bit
    trivial = DecodingAutomaton(np.zeros(v_tgt, np.uint8), [[0]], [0])
    for K in (1, 4, 16):
        free = _decode(device_model("trained"), src[:7], K)
        same = _decode(device_model("trained"), src[:7], K, constraint=trivial)
        assert set(free) == set(same) and all(torch.equal(free[k], same[k]) for k in free), K


def test_the_plain_kernel_and_the_sampler_do_not_notice(models):
    sds, device_model, v_src, v_tgt = models
    model = device_model("untrained")
    src = _sources(v_src, v_tgt, 19, 3, long=True).to("cuda:0")
    state = model.encode(src, dropout=False)

    def plain():
        out = model.decode_beam(state, 8, trace=True)
        return [out[k].clone() for k in ("beam_predictions", "beam_log_probabilities", "loss")] + [v.clone() for v in out["beam_trace"].values()]

    def sampled(with_call):
        torch.manual_seed(11)
        with torch.no_grad():
            if with_call:
                model.decode_stochastic_beam(state, 8, seed=3)
            a = model(src, decoding_strategy="sampling")
        return a["predictions"].clone(), a["loss"].clone()

    before = plain()
    model.decode_stochastic_beam(state, 8, seed=3, trace=True)
    for x, y in zip(before, plain()):
        assert torch.equal(x, y)
    for x, y in zip(sampled(False), sampled(True)):
        assert torch.equal(x, y)


def test_c_abi_refuses_bad_arguments():
    from probnmn import _hip

    lib = _hip.lib()
    f = torch.zeros(64, device="cuda:0")
    tokens = torch.full((64,), -7, dtype=torch.long, device="cuda:0")
    scores, perturbed = torch.full((16,), 123.0, device="cuda:0"), torch.full((16,), 321.0, device="cuda:0")
    traces = [torch.full((64,), -9, dtype=torch.int32, device="cuda:0") for _ in range(2)] + [torch.full((64,), 5.0, device="cuda:0") for _ in range(2)]
    p = f.data_ptr()

    def call(B=1, T=4, hidden=256, beam=4, perturbed_ptr=perturbed.data_ptr(), trace=(None, None, None, None), offset=0):
        return lib.pnmn_attn_lstm_beam_stochastic(p, p, p, p, p, p, p, p, tokens.data_ptr(), scores.data_ptr(), trace[0], trace[1],
                                                  trace[2], B, T, 8, 44, hidden, beam, 0, 1, 2, 3, None, None, None, 0, 0,
                                                  perturbed_ptr, trace[3], 5, offset, None)

    t = [x.data_ptr() for x in traces]
    for kwargs in (dict(perturbed_ptr=None), dict(trace=(t[0], t[1], t[2], None)), dict(trace=(None, None, None, t[3])),
                   dict(trace=(t[0], None, t[2], t[3])), dict(offset=-1), dict(beam=3), dict(hidden=128)):
        assert call(**kwargs) == _hip.EINVAL, kwargs
    assert call(B=0) == 0 and call(B=0, trace=tuple(t)) == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()) and bool((scores == 123.0).all()) and bool((perturbed == 321.0).all())
    assert all(bool((x == v).all()) for x, v in zip(traces, (-9, -9, 5.0, 5.0)))


def test_answers_from_a_sample_without_replacement(models, vocab):
    """predict_answers(num_programs=8, without_replacement=True) on the peaked generator: ``support`` is the number of distinct
    valid hypotheses, the weights sum to 1, "importance" gives the K-th hypothesis weight 0, rerank accepts the proposals, and
    the answers with without_replacement=False are what they are without the arguments."""
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import evaluate_marginal_answer_accuracy, predict_answers
    from probnmn.models import NeuralModuleNetwork, ProgramPrior, QuestionReconstructor

    sds, device_model, v_src, v_tgt = models
    dev = torch.device("cuda:0")
    pg = device_model("peaked", 12)
    torch.manual_seed(0)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64).to(dev)
    qr, prior = QuestionReconstructor(vocab).to(dev), ProgramPrior(vocab, hidden_size=256).to(dev)
    batches = [{k: v.to(dev) for k, v in synthetic_batch(vocab, 6, seed=11).items()}]
    itos = vocab.get_index_to_token_vocabulary("programs")

    def strings(row):
        return [itos[int(x)] for x in row if int(x) != PAD]

    for constrained in (False, True):
        extra = dict(constrained_sampling=True) if constrained else {}
        torch.manual_seed(3)
        records = predict_answers(pg, nmn, batches, vocab, num_programs=8, without_replacement=True, **extra)
        torch.manual_seed(3)
        again = predict_answers(pg, nmn, batches, vocab, num_programs=8, without_replacement=True, sample_weights="importance", **extra)
        # the hypotheses of the same seed, straight from the decoder
        torch.manual_seed(3)
        auto = nmn.engine.compiler.decoding_automaton(exclude=[PAD, UNK, START, END]) if constrained else None
        with torch.no_grad():
            out = pg(batches[0]["question"], decoding_strategy="stochastic_beam", beam_size=8, constraint=auto)
        beams, phi, G = out["beam_predictions"].cpu(), out["beam_log_probabilities"].cpu(), out["beam_perturbed"].cpu()
        for i, (r, s) in enumerate(zip(records, again)):
            ok = [c.valid for c in nmn.engine.compiler.compile_batch(beams[i].numpy())]
            want = [k for k in range(8) if ok[k] and bool(torch.isfinite(phi[i, k]))]
            assert r["support"] == len(want) == len(r["hypotheses"]), (i, r["support"], want)
            assert [h["program"] for h in r["hypotheses"]] == [strings(beams[i, k]) for k in want]
            assert [h["perturbed"] for h in r["hypotheses"]] == [float(G[i, k]) for k in want]
            if constrained:
                assert r["support"] >= 2
            if want:
                assert abs(sum(h["weight"] for h in r["hypotheses"]) - 1.0) < 1e-5
                share = torch.softmax(phi[i, want].double(), 0)
                assert np.allclose([h["weight"] for h in r["hypotheses"]], share.numpy(), atol=1e-5)
            # "importance": the K-th hypothesis sets the threshold and weighs nothing
            kept = [k for k in want if k != 7 or not bool(torch.isfinite(G[i, 7]))]
            assert [h["program"] for h in s["hypotheses"]] == [strings(beams[i, k]) for k in kept]
            if kept:
                assert abs(sum(h["weight"] for h in s["hypotheses"]) - 1.0) < 1e-5
    torch.manual_seed(3)
    reranked = predict_answers(pg, nmn, batches, vocab, num_programs=8, without_replacement=True, constrained_sampling=True,
                               rerank=True, question_reconstructor=qr, program_prior=prior)
    assert [r["support"] for r in reranked] == [r["support"] for r in records]
    assert all("map_answer" in r and all("log_prior" in h and "perturbed" in h for h in r["hypotheses"]) for r in reranked)
    torch.manual_seed(3)
    got = evaluate_marginal_answer_accuracy(pg, nmn, batches, num_programs=8, without_replacement=True, constrained_sampling=True)
    assert got["average_support"] == sum(r["support"] for r in records) / 6
    # the defaults leave every existing call as it is
    torch.manual_seed(9)
    base = predict_answers(pg, nmn, batches, vocab, num_programs=8)
    torch.manual_seed(9)
    assert predict_answers(pg, nmn, batches, vocab, num_programs=8, without_replacement=False, sample_weights="probability") == base
    assert all("perturbed" not in h for r in base for h in r["hypotheses"])
