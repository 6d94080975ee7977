"""Beam-search decoding on the device (``pnmn_attn_lstm_beam``, ``decoding_strategy="beam"``) against the fp64 host
reference of tests/helpers/beam_reference.py.

The main check REPLAYS the device's own prefixes in fp64 (every step of every question: the chosen candidates beat the
ones not chosen, are ordered, and carry the right running score, all within tol_t = 1e-4 * (t + 1) -- the project's
fp32 loss bar per decoded token), so a near-tie decided the other way passes and a wrong gather does not.  The tests
run on an untrained model and on one trained on the host until its hypotheses finish at different steps.

Worst ratios to tol_t measured on an MI355X: see DESIGN.md section 5."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import beam_reference as br  # noqa: E402

from oracle.seq2seq_oracle import END, PAD, START, UNK, trim_predictions  # noqa: E402

pytestmark = pytest.mark.gpu

BEAMS = (1, 2, 4, 8, 16)
STEPS = 12
NEG = float("-inf")


def _spec(kind):
    from probnmn.models import ProgramGenerator, QuestionReconstructor

    return {"pg": (ProgramGenerator, "questions", "programs"), "qr": (QuestionReconstructor, "programs", "questions")}[kind]


@pytest.fixture(scope="module")
def vocab():
    from probnmn.vocabulary import Vocabulary

    return Vocabulary.clevr()


@pytest.fixture(scope="module", params=["pg", "qr"])
def models(request, vocab):
    """(kind, {"untrained" | "trained": (device model, host state_dict)}, source vocabulary size, target vocabulary size).
    The trained one: 100 Adam steps of the oracle's teacher-forced loss on the host; on the REFERENCE alone, at K = 4
    and T = 12, every hypothesis must finish and the first @end@ must fall on at least four different steps."""
    cls, src_ns, tgt_ns = _spec(request.param)
    v_src, v_tgt = vocab.get_vocab_size(src_ns), vocab.get_vocab_size(tgt_ns)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, max(1, threads)))
    try:
        torch.manual_seed(0)
        fresh = {k: v.detach().clone() for k, v in cls(vocab, max_decoding_steps=STEPS).state_dict().items()}
        trained = br.train_on_host(fresh, v_src, v_tgt, steps=100, rows=64)
    finally:
        torch.set_num_threads(threads)
    src, _ = br.synthetic_task(v_src, v_tgt, 128, torch.Generator().manual_seed(99))
    ends = br.first_end_steps(br.beam_search(trained, src, 4, STEPS)["tokens"])
    assert int(ends.max()) < STEPS, "fixture: a reference hypothesis does not finish"
    assert len(set(ends.reshape(-1).tolist())) >= 4, "fixture: first @end@ on fewer than four different steps"
    out = {}
    for name, sd in (("untrained", fresh), ("trained", trained)):
        model = cls(vocab, max_decoding_steps=STEPS)
        model.load_state_dict(sd)
        out[name] = (model.to("cuda:0"), sd)
    return request.param, out, v_src, v_tgt


def _sources(v_src, v_tgt, rows, seed, long=False):
    """Sources of the synthetic task; ``long``: random tokens, 3-40 of them per row (several chunks of encoder positions)."""
    gen = torch.Generator().manual_seed(seed)
    if not long:
        return br.synthetic_task(v_src, v_tgt, rows, gen)[0]
    src = torch.zeros(rows, 40, dtype=torch.long)
    for r in range(rows):
        n = int(torch.randint(3, 41, (1,), generator=gen))
        src[r, :n] = torch.randint(4, v_src, (n,), generator=gen)
    return src


def _device_beam(model, src, K):
    out = model.decode_beam(model.encode(src.to("cuda:0")), K, trace=True)
    torch.cuda.synchronize()
    tr = out["beam_trace"]
    return ({k: v.cpu() for k, v in out.items() if k != "beam_trace"},
            tr["tokens"].cpu().long(), tr["backpointers"].cpu().long(), tr["scores"].cpu())


def _replay_check(sd, src, out, tok, bp, sc, K, V):
    """The four conditions of the replay check on one batch; returns the worst ratio to tol_t seen in (a), (b), (c)."""
    B, T, _ = tok.shape
    # (d) exact: tokens in range, never pad / unk / start
    assert int(tok.min()) >= 0 and int(tok.max()) < V and int(bp.min()) >= 0 and int(bp.max()) < K
    assert not bool(((tok == PAD) | (tok == UNK) | (tok == START)).any())
    tables = br.replay(sd, src, tok, bp)
    worst = 0.0
    prev_tok = torch.full((B, K), START, dtype=torch.long)
    prev_sc = torch.full((B, K), NEG)
    prev_sc[:, 0] = 0.0
    for t in range(T):
        tol = 1e-4 * (t + 1)
        cand = tables[t]
        live = sc[:, t] > NEG  # slots that hold a hypothesis
        flat = bp[:, t] * V + tok[:, t]
        chosen = torch.where(live, cand.gather(1, flat), torch.full((B, K), NEG, dtype=cand.dtype))
        # a slot without a hypothesis: token @end@, back-pointer 0 -- and live slots first
        assert bool((tok[:, t][~live] == END).all()) and bool((bp[:, t][~live] == 0).all())
        assert bool((live[:, :-1] | ~live[:, 1:]).all())
        # live slots chose distinct, finite candidates
        assert bool(torch.isfinite(chosen[live]).all()), "step %d: a chosen candidate the reference rules out" % t
        for b in range(B):
            f = flat[b][live[b]].tolist()
            assert len(set(f)) == len(f), (t, b, f)
        rest = cand.clone()
        rest.scatter_(1, torch.where(live, flat, flat[:, :1].expand(B, K)), NEG)  # (slot 0 is live from step 0 on)
        best_rest = rest.max(1)[0]
        worst_chosen = chosen.min(1)[0]
        # (a) each chosen candidate >= every candidate not chosen - tol_t  (a -inf slot: nothing finite may be left)
        gap = best_rest - worst_chosen
        gap = torch.where(best_rest == NEG, torch.zeros_like(gap), gap)
        assert bool((gap <= tol).all()), "step %d: (a) worst %g x tol_t" % (t, float(gap.max()) / tol)
        worst = max(worst, float(gap.max()) / tol)
        # (b) best first within tol_t
        order = chosen[:, 1:] - chosen[:, :-1]
        order = torch.where(torch.isnan(order) | (chosen[:, 1:] == NEG), torch.zeros_like(order), order)
        if K > 1:
            assert bool((order <= tol).all()), "step %d: (b) worst %g x tol_t" % (t, float(order.max()) / tol)
            worst = max(worst, float(order.max()) / tol)
        # (c) the device's running score = the fp64 candidate within tol_t
        err = (sc[:, t].double() - chosen)[live].abs()
        assert bool((err <= tol).all()), "step %d: (c) worst %g x tol_t" % (t, float(err.max()) / tol)
        worst = max(worst, float(err.max()) / tol) if err.numel() else worst
        # (d) a finished slot extends only by @end@ with an unchanged score
        parent_tok, parent_sc = prev_tok.gather(1, bp[:, t]), prev_sc.gather(1, bp[:, t])
        ext = live & (parent_tok == END)
        assert bool((tok[:, t][ext] == END).all()) and bool((sc[:, t][ext] == parent_sc[ext]).all())
        prev_tok, prev_sc = tok[:, t], sc[:, t]
    # (d) the back-tracked outputs agree with the trace
    raw = br.backtrack(tok, bp)
    assert torch.equal(out["beam_predictions"], trim_predictions(raw.view(B * K, T)).view(B, K, T))
    assert torch.equal(out["beam_log_probabilities"], sc[:, -1])
    return worst


@pytest.mark.parametrize("which", ["untrained", "trained"])
@pytest.mark.parametrize("rows", [37, 128])
@pytest.mark.parametrize("K", BEAMS)
def test_replay_of_the_device_prefixes(models, which, rows, K):
    kind, pair, v_src, v_tgt = models
    model, sd = pair[which]
    src = _sources(v_src, v_tgt, rows, 7 + rows, long=which == "untrained")
    out, tok, bp, sc = _device_beam(model, src, K)
    worst = _replay_check(sd, src, out, tok, bp, sc, K, v_tgt)
    if which == "trained" and K >= 4:  # the finished-hypothesis path is exercised
        ends = br.first_end_steps(br.backtrack(tok, bp))
        assert int((ends < STEPS).sum()) > 0
    print("replay %s %s B=%d K=%d: worst ratio to tol_t %.4f" % (kind, which, rows, K, worst))


@pytest.mark.parametrize("which,K,rows", [("untrained", 16, 3), ("trained", 16, 5), ("trained", 2, 19)])
def test_replay_at_the_longest_decode(models, vocab, which, K, rows):
    """T = 64, the most steps the kernel keeps a history for (the trained model: most of them after every hypothesis has
    finished, i.e. filled in after the early stop)."""
    kind, pair, v_src, v_tgt = models
    _, sd = pair[which]
    model = _spec(kind)[0](vocab, max_decoding_steps=64)
    model.load_state_dict(sd)
    model.to("cuda:0")
    src = _sources(v_src, v_tgt, rows, 31, long=which == "untrained")
    out, tok, bp, sc = _device_beam(model, src, K)
    assert tok.shape == (rows, 64, K)
    worst = _replay_check(sd, src, out, tok, bp, sc, K, v_tgt)
    print("replay %s %s B=%d K=%d T=64: worst ratio to tol_t %.4f" % (kind, which, rows, K, worst))


@pytest.mark.parametrize("K", BEAMS)
def test_agreement_with_the_reference_search(models, K):
    """Every question whose reference margin (smallest gap between adjacent ranks 1..K+1 over all steps) is >= tol_T has
    the reference's K-best list token for token; the share below the margin and the overall agreement are printed."""
    kind, pair, v_src, v_tgt = models
    model, sd = pair["trained"]
    src = _sources(v_src, v_tgt, 128, 1234)
    out, tok, bp, sc = _device_beam(model, src, K)
    ref = br.beam_search(sd, src, K, STEPS)
    want = trim_predictions(ref["tokens"].view(128 * K, STEPS)).view(128, K, STEPS)
    same = (out["beam_predictions"] == want).all(-1).all(-1)
    clear = ref["margin"] >= 1e-4 * STEPS
    print("agreement %s K=%d: %d/128 questions equal the reference's K-best list; %d/128 below the margin"
          % (kind, K, int(same.sum()), int((~clear).sum())))
    assert bool(same[clear].all()), (torch.nonzero(clear & ~same).reshape(-1).tolist())
    assert torch.allclose(out["beam_log_probabilities"][same].double(), ref["scores"][same], atol=1e-4 * STEPS)


def test_surface(models, vocab):
    kind, pair, v_src, v_tgt = models
    model, sd = pair["trained"]
    src = _sources(v_src, v_tgt, 21, 5).to("cuda:0")
    B, K, T = 21, 4, STEPS
    model.train()
    state = torch.get_rng_state()
    out = model(src, decoding_strategy="beam", beam_size=K)
    assert torch.equal(torch.get_rng_state(), state), "a beam call must not draw from the torch generator"
    assert set(out) == {"predictions", "loss", "beam_predictions", "beam_log_probabilities"}
    assert out["beam_predictions"].shape == (B, K, T) and out["beam_predictions"].dtype == torch.long
    assert out["beam_log_probabilities"].shape == (B, K) and out["beam_log_probabilities"].dtype == torch.float32
    assert out["predictions"].shape == (B, T) and out["loss"].shape == (B,)
    assert all(not v.requires_grad for v in out.values())
    assert torch.equal(out["predictions"], out["beam_predictions"][:, 0])
    beams = out["beam_predictions"].cpu()
    assert torch.equal(beams.view(B * K, T), trim_predictions(beams.view(B * K, T)))  # trimmed: a fixed point of the rule
    model.eval()
    again = model(src, decoding_strategy="beam", beam_size=K)
    model.train()
    assert torch.equal(again["beam_predictions"], out["beam_predictions"])  # the same in train() and eval() mode
    via_decode = model.decode(model.encode(src), decoding_strategy="beam", beam_size=K)
    assert torch.equal(via_decode["beam_predictions"], out["beam_predictions"])
    # loss = -score / (n + 1e-12) of the best hypothesis, for EVERY row: the score is the fp64 one of the device's own best
    # hypothesis (the replay tables' entry for slot 0 at the last step), n its non-padding tokens
    traced = model.decode_beam(model.encode(src, dropout=False), K, trace=True)
    assert torch.equal(traced["beam_predictions"], out["beam_predictions"]) and torch.equal(traced["loss"], out["loss"])
    tr = traced["beam_trace"]
    tok, bp = tr["tokens"].cpu().long(), tr["backpointers"].cpu().long()
    tables = br.replay(sd, src.cpu(), tok, bp)
    score64 = tables[-1].gather(1, (bp[:, -1, :1] * v_tgt + tok[:, -1, :1])).squeeze(1)
    n = (out["predictions"].cpu() != PAD).sum(-1).double()
    want = torch.where(n > 0, -score64 / (n + 1e-12), torch.zeros_like(n))
    assert bool(torch.isfinite(want).all())
    assert torch.allclose(out["loss"].cpu().double(), want, atol=1e-4, rtol=0)
    # default width, and the arguments that are refused
    assert model(src, decoding_strategy="beam")["beam_predictions"].shape == (B, 4, T)
    for bad in (3, 0, 32, 2.0, None):
        with pytest.raises(ValueError):
            model(src, decoding_strategy="beam", beam_size=bad)
    with pytest.raises(ValueError):
        model(src, src, decoding_strategy="beam")
    with pytest.raises(ValueError):
        model.decode(model.encode(src), src, decoding_strategy="beam")
    with pytest.raises(ValueError):
        model(src, decoding_strategy="beams")


def test_shapes_outside_the_kernel_are_refused(vocab):
    cls, _, _ = _spec("pg")
    torch.manual_seed(0)
    src = torch.randint(4, 40, (5, 9), device="cuda:0")
    small = cls(vocab, input_size=128, hidden_size=128).to("cuda:0")
    with pytest.raises(NotImplementedError, match="256"):
        small(src, decoding_strategy="beam", beam_size=4)
    long_steps = cls(vocab, max_decoding_steps=65).to("cuda:0")
    with pytest.raises(NotImplementedError, match="64"):
        long_steps(src, decoding_strategy="beam", beam_size=4)
    with pytest.raises(NotImplementedError, match="64"):
        long_steps(torch.randint(4, 40, (2, 70), device="cuda:0"), decoding_strategy="beam", beam_size=2)


def test_c_abi_refuses_bad_arguments():
    from probnmn import _hip

    lib = _hip.lib()
    f = torch.zeros(16, device="cuda:0")
    i = torch.zeros(16, dtype=torch.long, device="cuda:0")
    p = f.data_ptr()

    def call(B=1, T=4, S=8, V=44, hidden=256, beam=4, tokens=i.data_ptr(), trace=(None, None, None), start=2, end=3):
        return lib.pnmn_attn_lstm_beam(p, p, p, p, p, p, p, p, tokens, p, trace[0], trace[1], trace[2], B, T, S, V, hidden, beam,
                                       0, 1, start, end, None, None, None, 0, 0, None)

    for kwargs in (dict(beam=3), dict(beam=32), dict(hidden=128), dict(S=65), dict(S=0), dict(V=129), dict(T=65), dict(tokens=None),
                   dict(trace=(p, None, None)), dict(end=44), dict(start=-1), dict(B=-1)):
        assert call(**kwargs) == _hip.EINVAL, kwargs
    assert call(B=0) == 0  # nothing to do


def test_sampling_and_greedy_do_not_notice_a_beam_call(models):
    kind, pair, v_src, v_tgt = models
    model, _ = pair["untrained"]
    src = _sources(v_src, v_tgt, 19, 3).to("cuda:0")

    def passes(with_beam):
        torch.manual_seed(11)
        with torch.no_grad():
            a = model(src)
            if with_beam:
                model(src, decoding_strategy="beam", beam_size=8)
            b = model(src)
            c = model(src, decoding_strategy="greedy")
        return [x[k].clone() for x in (a, b, c) for k in ("predictions", "loss")]

    for x, y in zip(passes(False), passes(True)):
        assert torch.equal(x, y)


def test_beam_ignores_encoder_dropout_in_train_mode(vocab):
    """A generator with LSTM dropout between its encoder layers, in train() mode: a beam call draws nothing from the torch
    generator, searches the encoding WITHOUT dropout (the eval() result), and the seeded sampled passes around it -- which
    do drop -- are what they are without it."""
    cls, _, _ = _spec("pg")
    torch.manual_seed(3)
    model = cls(vocab, dropout=0.3, max_decoding_steps=STEPS).to("cuda:0")
    src = _sources(vocab.get_vocab_size("questions"), vocab.get_vocab_size("programs"), 23, 9, long=True).to("cuda:0")
    model.train()
    torch.manual_seed(21)
    with torch.no_grad():
        one, two = model(src), model(src)
    assert not torch.equal(one["loss"], two["loss"])  # (dropout and sampling are live in this mode)

    state = torch.get_rng_state()
    in_train = model(src, decoding_strategy="beam", beam_size=4)
    assert torch.equal(torch.get_rng_state(), state), "a beam call must not draw from the torch generator"
    again = model(src, decoding_strategy="beam", beam_size=4)
    model.eval()
    in_eval = model(src, decoding_strategy="beam", beam_size=4)
    model.train()
    for key in ("beam_predictions", "beam_log_probabilities", "predictions", "loss"):
        assert torch.equal(in_train[key], in_eval[key]) and torch.equal(in_train[key], again[key]), key
    via_state = model.decode(model.encode(src, dropout=False), decoding_strategy="beam", beam_size=4)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(via_state["beam_predictions"], in_eval["beam_predictions"])

    def passes(with_beam):
        torch.manual_seed(21)
        with torch.no_grad():
            a = model(src)
            if with_beam:
                model(src, decoding_strategy="beam", beam_size=8)
            b = model(src)
            c = model(src, decoding_strategy="greedy")
        return [x[k].clone() for x in (a, b, c) for k in ("predictions", "loss")]

    for x, y in zip(passes(False), passes(True)):
        assert torch.equal(x, y)


def test_inference_with_a_beam(vocab):
    """predict_answers(beam_size=4): the answers are the oracle NMN's on the programs the records name; with
    prefer_valid a record whose beam holds a valid program names the best-ranked valid one; beam_size=None is unchanged."""
    from oracle import nmn_oracle
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import predict_answers
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.optim import ClampAdam
    from probnmn.runtime.program_compiler import ProgramCompiler

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64)
    nmn_sd = {k: v.detach().clone() for k, v in nmn.state_dict().items()}
    pg.to(dev), nmn.to(dev)
    host = [synthetic_batch(vocab, 6, seed=s) for s in (11, 12)]
    batches = [{k: v.to(dev) for k, v in b.items()} for b in host]
    # teach the generator these programs for a few iterations, so that its beams hold valid programs
    opt = ClampAdam(list(pg.parameters()), lr=2e-3, clamp=5.0)
    q = torch.cat([b["question"] for b in batches])
    p = torch.cat([b["program"] for b in batches])
    for _ in range(120):
        opt.zero_grad()
        pg(q, p, decoding_strategy="sampling")["loss"].mean().backward()
        opt.step()

    torch.manual_seed(5)
    before = predict_answers(pg, nmn, batches, vocab)
    torch.manual_seed(5)
    assert predict_answers(pg, nmn, batches, vocab, beam_size=None) == before
    assert all(set(r) == {"question_index", "answer"} for r in before)

    itos = vocab.get_index_to_token_vocabulary("programs")
    stoi = vocab.get_token_to_index_vocabulary("programs")
    reference = ProgramCompiler(itos)  # its Python rules: pinned to tests/golden/nmn_validity.json by test_program_compiler
    for prefer in (True, False):
        records = predict_answers(pg, nmn, batches, vocab, beam_size=4, prefer_valid=prefer)
        assert len(records) == 12 and [r["question_index"] for r in records] == list(range(12))
        assert pg.training and nmn.training
        pg.eval()
        with torch.no_grad():
            beams = torch.cat([pg(b["question"], decoding_strategy="beam", beam_size=4)["beam_predictions"].cpu() for b in batches])
        pg.train()
        T = beams.size(-1)
        named = torch.zeros(12, T, dtype=torch.long)
        n_valid = 0
        for i, r in enumerate(records):
            assert set(r) == {"question_index", "answer", "program", "beam_rank", "program_valid"}
            ids = [stoi[t] for t in r["program"]]
            named[i, : len(ids)] = torch.tensor(ids, dtype=torch.long)
            assert torch.equal(named[i], beams[i, r["beam_rank"]])
            ok = [reference.compile(beams[i, k].tolist()).valid for k in range(4)]
            want_rank = ok.index(True) if (prefer and True in ok) else 0
            assert r["beam_rank"] == want_rank and r["program_valid"] == ok[want_rank], (i, r, ok)
            n_valid += r["program_valid"]
        assert n_valid >= 3, "fixture: the fitted generator's beams should hold valid programs"
        k = 0
        for b in host:
            out = nmn_oracle.nmn_forward(nmn_sd, itos, b["image"], named[k:k + 6], None)
            for a in out["predictions"].tolist():
                assert records[k]["answer"] == vocab.get_token_from_index(a, "answers")
                k += 1
