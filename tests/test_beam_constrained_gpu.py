"""Grammar-constrained beam search on the device (the tables of ``pnmn_attn_lstm_beam``, ``decode_beam(constraint=...)``,
``predict_answers(constrained=True)``) against the fp64 host reference of tests/helpers/constrained_beam_reference.py.

As in tests/test_beam_gpu.py the main check REPLAYS the device's own prefixes in fp64, here against the CONSTRAINED
candidate table: the chosen candidates beat the ones not chosen, are ordered and carry the right running score, all
within tol_t = 1e-4 * (t + 1); a candidate the automaton rules out is -inf in that table, so a device that chose one
fails.  On top of that every device hypothesis with a finite score must compile as a valid program and slot 0 of every
question must be finite.  The models are ProgramGenerators: untrained, and trained on the host on the synthetic task of
beam_reference.py -- whose unconstrained best program is invalid on every question (tests/test_decoding_automaton.py).

Worst ratios to tol_t measured on an MI355X: see DESIGN.md section 5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import beam_reference as br  # noqa: E402
import constrained_beam_reference as cbr  # noqa: E402

from oracle.seq2seq_oracle import END, PAD, START, UNK, trim_predictions  # noqa: E402

pytestmark = pytest.mark.gpu

BEAMS = (1, 2, 4, 8, 16)
STEPS = 12
NEG = float("-inf")
EXCLUDE = (PAD, UNK, START, END)


@pytest.fixture(scope="module")
def vocab():
    from probnmn.vocabulary import Vocabulary

    return Vocabulary.clevr()


@pytest.fixture(scope="module")
def grammar(vocab):
    """(compiler, automaton of the CLEVR program vocabulary)."""
    from probnmn.runtime.program_compiler import ProgramCompiler

    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    return comp, comp.decoding_automaton(exclude=EXCLUDE)


@pytest.fixture(scope="module")
def models(vocab):
    """({"untrained" | "trained": (device model, host state_dict)}, source vocabulary size, target vocabulary size): the
    ProgramGenerator fixture of tests/test_beam_gpu.py (seed 0, 100 Adam steps on the host)."""
    from probnmn.models import ProgramGenerator

    v_src, v_tgt = vocab.get_vocab_size("questions"), vocab.get_vocab_size("programs")
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, max(1, threads)))
    try:
        torch.manual_seed(0)
        fresh = {k: v.detach().clone() for k, v in ProgramGenerator(vocab, max_decoding_steps=STEPS).state_dict().items()}
        trained = br.train_on_host(fresh, v_src, v_tgt, steps=100, rows=64)
    finally:
        torch.set_num_threads(threads)
    out = {}
    for name, sd in (("untrained", fresh), ("trained", trained)):
        model = ProgramGenerator(vocab, max_decoding_steps=STEPS)
        model.load_state_dict(sd)
        out[name] = (model.to("cuda:0"), sd)
    return out, v_src, v_tgt


def _with_steps(vocab, sd, steps):
    from probnmn.models import ProgramGenerator

    model = ProgramGenerator(vocab, max_decoding_steps=steps)
    model.load_state_dict(sd)
    return model.to("cuda:0")


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


def _device_beam(model, src, K, constraint):
    out = model.decode_beam(model.encode(src.to("cuda:0")), K, trace=True, constraint=constraint)
    torch.cuda.synchronize()
    tr = out["beam_trace"]
    return ({k: v.cpu() for k, v in out.items() if k != "beam_trace"},
            tr["tokens"].cpu().long(), tr["backpointers"].cpu().long(), tr["scores"].cpu())


def _replay_check(sd, src, out, tok, bp, sc, K, V, auto):
    """The four conditions of the replay check of tests/test_beam_gpu.py on one batch, against the constrained candidate
    tables; returns the worst ratio to tol_t seen in (a), (b), (c)."""
    B, T, _ = tok.shape
    # (d) exact: tokens in range, never pad / unk / start
    assert int(tok.min()) >= 0 and int(tok.max()) < V and int(bp.min()) >= 0 and int(bp.max()) < K
    assert not bool(((tok == PAD) | (tok == UNK) | (tok == START)).any())
    # (the slots the device leaves without a hypothesis stay empty in the replay; that nothing finite was left for them is (a))
    tables = cbr.replay(sd, src, tok, bp, auto.token_class, auto.next_state, auto.min_left, live=sc > NEG)
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
        assert bool(live[:, 0].all()), "step %d: slot 0 of a question holds no hypothesis" % t
        # live slots chose distinct, finite candidates: none that the automaton (or the base rule) rules out
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


def _all_valid(comp, out):
    """Every device hypothesis with a finite score compiles as valid (Python rules and the native host compiler); slot 0 of
    every question is finite.  Returns the number of finite hypotheses."""
    beams, scores = out["beam_predictions"], out["beam_log_probabilities"]
    B, K, T = beams.shape
    finite = torch.isfinite(scores)
    assert bool(finite[:, 0].all()), "slot 0 of a question is not finite"
    assert bool((scores[~finite] == NEG).all())
    rows = beams.view(B * K, T)[finite.view(-1)]
    assert all(comp.compile(r).valid for r in rows.tolist())
    assert all(p.valid for p in comp.compile_batch(rows.numpy()))
    return int(finite.sum())


@pytest.mark.parametrize("which", ["untrained", "trained"])
@pytest.mark.parametrize("rows", [37, 128])
@pytest.mark.parametrize("K", BEAMS)
def test_replay_of_the_device_prefixes(models, grammar, which, rows, K):
    pair, v_src, v_tgt = models
    comp, auto = grammar
    model, sd = pair[which]
    src = _sources(v_src, v_tgt, rows, 7 + rows, long=which == "untrained")
    out, tok, bp, sc = _device_beam(model, src, K, auto)
    worst = _replay_check(sd, src, out, tok, bp, sc, K, v_tgt, auto)
    n_finite = _all_valid(comp, out)
    assert n_finite == rows * K  # (T = 12: far more valid programs than slots)
    print("constrained replay %s B=%d K=%d: worst ratio to tol_t %.4f" % (which, rows, K, worst))


@pytest.mark.parametrize("which,K,rows", [("untrained", 16, 3), ("trained", 16, 5), ("trained", 2, 19)])
def test_replay_at_the_longest_decode(models, grammar, vocab, which, K, rows):
    """T = 64, the most steps the kernel keeps a history for."""
    pair, v_src, v_tgt = models
    comp, auto = grammar
    _, sd = pair[which]
    model = _with_steps(vocab, sd, 64)
    src = _sources(v_src, v_tgt, rows, 31, long=which == "untrained")
    out, tok, bp, sc = _device_beam(model, src, K, auto)
    assert tok.shape == (rows, 64, K)
    worst = _replay_check(sd, src, out, tok, bp, sc, K, v_tgt, auto)
    assert _all_valid(comp, out) == rows * K
    print("constrained replay %s B=%d K=%d T=64: worst ratio to tol_t %.4f" % (which, rows, K, worst))


@pytest.mark.parametrize("which", ["untrained", "trained"])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_replay_at_the_shortest_decodes(models, grammar, vocab, which, T):
    """T = 1, 2, 3: the step budget decides almost every token, and a wide beam runs out of valid programs (T = 1: the
    empty program and `unique`), so slots without a hypothesis occur."""
    pair, v_src, v_tgt = models
    comp, auto = grammar
    _, sd = pair[which]
    model = _with_steps(vocab, sd, T)
    src = _sources(v_src, v_tgt, 37, 41 + T, long=which == "untrained")
    for K in BEAMS:
        out, tok, bp, sc = _device_beam(model, src, K, auto)
        assert tok.shape == (37, T, K)
        worst = _replay_check(sd, src, out, tok, bp, sc, K, v_tgt, auto)
        n_finite = _all_valid(comp, out)
        if T == 1:
            assert n_finite == 37 * min(K, 2)
        print("constrained replay %s B=37 K=%d T=%d: worst ratio to tol_t %.4f, %d finite hypotheses"
              % (which, K, T, worst, n_finite))


@pytest.mark.parametrize("K", [1, 2, 4])
def test_agreement_with_the_reference_search(models, grammar, K):
    """Every question whose reference margin (smallest gap between adjacent ranks 1..K+1 of the constrained candidates over
    all steps) is >= 1e-4 * T has the reference's K-best list token for token and its scores within 1e-4 * T; at most 16 of
    the 128 questions may fall below the margin (the fp64 reference alone: 0 / 10 / 11 at K = 1 / 2 / 4; 43 and 84 at
    K = 8 and 16, which the replay check covers)."""
    pair, v_src, v_tgt = models
    comp, auto = grammar
    model, sd = pair["trained"]
    src = _sources(v_src, v_tgt, 128, 1234)
    out, tok, bp, sc = _device_beam(model, src, K, auto)
    ref = cbr.beam_search(sd, src, K, STEPS, auto.token_class, auto.next_state, auto.min_left)
    want = trim_predictions(ref["tokens"].view(128 * K, STEPS)).view(128, K, STEPS)
    same = (out["beam_predictions"] == want).all(-1).all(-1)
    clear = ref["margin"] >= 1e-4 * STEPS
    print("constrained agreement K=%d: %d/128 questions equal the reference's K-best list; %d/128 below the margin"
          % (K, int(same.sum()), int((~clear).sum())))
    assert int((~clear).sum()) <= 16
    assert bool(same[clear].all()), (torch.nonzero(clear & ~same).reshape(-1).tolist())
    err = (out["beam_log_probabilities"][clear].double() - ref["scores"][clear]).abs()
    assert bool((err <= 1e-4 * STEPS).all()), float(err.max())
    # the premise: the unconstrained device search names no valid best program here
    free = model.decode_beam(model.encode(src.to("cuda:0")), K)["predictions"].cpu()
    assert not any(comp.compile(r).valid for r in free.tolist())


@pytest.mark.parametrize("which", ["untrained", "trained"])
def test_a_trivial_automaton_changes_nothing(models, which):
    """One state, one class, min_left = [0]: tokens, scores and trace are bit-identical to the unconstrained search."""
    from probnmn.runtime.program_compiler import DecodingAutomaton

    pair, v_src, v_tgt = models
    model, _ = pair[which]
    trivial = DecodingAutomaton(np.zeros(v_tgt, np.uint8), [[0]], [0])
    src = _sources(v_src, v_tgt, 37, 77, long=which == "untrained")
    for K in BEAMS:
        free = _device_beam(model, src, K, None)
        same = _device_beam(model, src, K, trivial)
        for key in ("predictions", "loss", "beam_predictions", "beam_log_probabilities"):
            assert torch.equal(free[0][key], same[0][key]), (K, key)
        for a, b in zip(free[1:], same[1:]):
            assert torch.equal(a, b), K


def test_c_abi_refuses_bad_tables():
    """Every refusal comes before any launch; the accepted call has nothing to do (B = 0)."""
    from probnmn import _hip

    lib = _hip.lib()
    f = torch.zeros(16, device="cuda:0")
    i = torch.zeros(16, dtype=torch.long, device="cuda:0")
    p = f.data_ptr()
    V = 44
    good = dict(token_class=np.zeros(V, np.uint8), next_state=np.zeros((2, 3), np.uint8), min_left=np.zeros(2, np.uint8))

    def call(B=0, n_states=2, n_classes=3, beam=4, drop=None, **tables):
        t = dict(good, **tables)
        ptr = {k: (None if k == drop else np.ascontiguousarray(v).ctypes.data) for k, v in t.items()}
        code = lib.pnmn_attn_lstm_beam(p, p, p, p, p, p, p, p, i.data_ptr(), p, None, None, None, B, 4, 8, V, 256, beam,
                                       0, 1, 2, 3, ptr["token_class"], ptr["next_state"], ptr["min_left"],
                                       n_states, n_classes, None)
        del t
        return code

    assert call() == 0
    assert call(n_states=32, n_classes=16, next_state=np.full((32, 16), 31, np.uint8), min_left=np.full(32, 255, np.uint8),
                token_class=np.full(V, 15, np.uint8)) == 0
    bad_class, bad_state, bad_last = good["token_class"].copy(), good["next_state"].copy(), good["next_state"].copy()
    bad_class[V - 1] = 3
    bad_state[0, 1] = 2
    bad_last[1, 2] = 200
    big = np.zeros((33, 17), np.uint8)
    for kwargs in (dict(drop="token_class"), dict(drop="next_state"), dict(drop="min_left"),
                   dict(n_states=0), dict(n_states=33, next_state=big, min_left=np.zeros(33, np.uint8)),
                   dict(n_classes=0), dict(n_classes=17, next_state=big), dict(n_states=-1), dict(n_classes=-1),
                   dict(token_class=bad_class), dict(next_state=bad_state), dict(next_state=bad_last),
                   dict(beam=3), dict(B=-1)):
        assert call(**kwargs) == _hip.EINVAL, sorted(kwargs)
    # with work to do the tables are checked before anything is launched
    for kwargs in (dict(B=1, drop="min_left"), dict(B=1, n_states=33, next_state=big, min_left=np.zeros(33, np.uint8)),
                   dict(B=1, token_class=bad_class), dict(B=1, next_state=bad_state)):
        assert call(**kwargs) == _hip.EINVAL, sorted(kwargs)
    torch.cuda.synchronize()


def test_surface_and_refusals(models, grammar):
    from probnmn.evaluators import predict_answers
    from probnmn.runtime.program_compiler import DecodingAutomaton

    pair, v_src, v_tgt = models
    comp, auto = grammar
    model, _ = pair["trained"]
    src = _sources(v_src, v_tgt, 21, 5).to("cuda:0")
    B, K, T = 21, 4, STEPS
    model.train()
    state = torch.get_rng_state()
    out = model(src, decoding_strategy="beam", beam_size=K, constraint=auto)
    assert torch.equal(torch.get_rng_state(), state), "a beam call must not draw from the torch generator"
    assert model.training
    assert set(out) == {"predictions", "loss", "beam_predictions", "beam_log_probabilities"}
    assert out["beam_predictions"].shape == (B, K, T) and out["beam_predictions"].dtype == torch.long
    assert out["beam_log_probabilities"].shape == (B, K) and out["beam_log_probabilities"].dtype == torch.float32
    assert out["predictions"].shape == (B, T) and out["loss"].shape == (B,)
    assert all(not v.requires_grad for v in out.values())
    assert torch.equal(out["predictions"], out["beam_predictions"][:, 0])
    assert all(comp.compile(r).valid for r in out["beam_predictions"].view(B * K, T).cpu().tolist())
    unconstrained = model(src, decoding_strategy="beam", beam_size=K)
    assert not torch.equal(unconstrained["predictions"], out["predictions"])
    assert torch.equal(model(src, decoding_strategy="beam", beam_size=K, constraint=None)["beam_predictions"],
                       unconstrained["beam_predictions"])
    model.eval()
    again = model(src, decoding_strategy="beam", beam_size=K, constraint=auto)
    assert not model.training
    model.train()
    assert torch.equal(again["beam_predictions"], out["beam_predictions"])  # the same in train() and eval() mode
    via_decode = model.decode(model.encode(src, dropout=False), decoding_strategy="beam", beam_size=K, constraint=auto)
    assert torch.equal(via_decode["beam_predictions"], out["beam_predictions"])
    assert torch.equal(via_decode["beam_log_probabilities"], out["beam_log_probabilities"])
    traced = model.decode_beam(model.encode(src, dropout=False), K, trace=True, constraint=auto)
    assert set(traced) == set(out) | {"beam_trace"} and torch.equal(traced["loss"], out["loss"])
    # plain arrays behind any object with the three attributes will do
    class Plain:
        token_class, next_state, min_left = auto.token_class.tolist(), auto.next_state.tolist(), auto.min_left.tolist()

    assert torch.equal(model(src, decoding_strategy="beam", beam_size=K, constraint=Plain())["beam_predictions"], out["beam_predictions"])
    assert torch.equal(torch.get_rng_state(), state)
    # refused: a constraint with another strategy, or of another vocabulary
    for strategy in ("sampling", "greedy"):
        with pytest.raises(ValueError):
            model(src, decoding_strategy=strategy, constraint=auto)
        with pytest.raises(ValueError):
            model.decode(model.encode(src), decoding_strategy=strategy, constraint=auto)
    with pytest.raises(ValueError):
        model(src, constraint=auto)
    wrong = DecodingAutomaton(auto.token_class[:-1], auto.next_state, auto.min_left)
    with pytest.raises(ValueError):
        model(src, decoding_strategy="beam", beam_size=K, constraint=wrong)
    with pytest.raises(ValueError):
        model.decode_beam(model.encode(src, dropout=False), K, constraint=wrong)
    with pytest.raises(ValueError):
        predict_answers(model, None, [], None, constrained=True)
    with pytest.raises(ValueError):
        predict_answers(model, None, [], None, beam_size=None, constrained=True)
    assert torch.equal(torch.get_rng_state(), state) and model.training


def test_inference_under_the_constraint(vocab):
    """predict_answers(beam_size=4, constrained=True) with an UNTRAINED generator: every record names a valid program of
    rank 0, no answer is @@UNKNOWN@@, the answers are the oracle NMN's on the named programs; without the constraint the
    same call names invalid programs; beam_size=None is unchanged."""
    from oracle import nmn_oracle
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import predict_answers
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.runtime.program_compiler import ProgramCompiler

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64)
    nmn_sd = {k: v.detach().clone() for k, v in nmn.state_dict().items()}
    pg.to(dev), nmn.to(dev)
    host = [synthetic_batch(vocab, 6, seed=s) for s in (11, 12)]
    batches = [{k: v.to(dev) for k, v in b.items()} for b in host]

    torch.manual_seed(5)
    before = predict_answers(pg, nmn, batches, vocab)
    torch.manual_seed(5)
    assert predict_answers(pg, nmn, batches, vocab, beam_size=None, constrained=False) == before
    assert all(set(r) == {"question_index", "answer"} for r in before)

    itos = vocab.get_index_to_token_vocabulary("programs")
    stoi = vocab.get_token_to_index_vocabulary("programs")
    reference = ProgramCompiler(itos)  # its Python rules: pinned to tests/golden/nmn_validity.json by test_program_compiler
    auto = reference.decoding_automaton(exclude=EXCLUDE)
    state = torch.get_rng_state()
    for prefer in (True, False):
        records = predict_answers(pg, nmn, batches, vocab, beam_size=4, prefer_valid=prefer, constrained=True)
        assert torch.equal(torch.get_rng_state(), state)
        assert len(records) == 12 and [r["question_index"] for r in records] == list(range(12))
        assert pg.training and nmn.training
        pg.eval()
        with torch.no_grad():
            beams = torch.cat([pg(b["question"], decoding_strategy="beam", beam_size=4, constraint=auto)["beam_predictions"].cpu()
                               for b in batches])
        pg.train()
        T = beams.size(-1)
        named = torch.zeros(12, T, dtype=torch.long)
        for i, r in enumerate(records):
            assert set(r) == {"question_index", "answer", "program", "beam_rank", "program_valid"}
            ids = [stoi[t] for t in r["program"]]
            named[i, : len(ids)] = torch.tensor(ids, dtype=torch.long)
            assert r["beam_rank"] == 0 and r["program_valid"] is True, (i, r)
            assert torch.equal(named[i], beams[i, 0])
            assert reference.compile(ids).valid
            assert r["answer"] != "@@UNKNOWN@@"
        k = 0
        for b in host:
            out = nmn_oracle.nmn_forward(nmn_sd, itos, b["image"], named[k:k + 6], None)
            for a in out["predictions"].tolist():
                assert records[k]["answer"] == vocab.get_token_from_index(a, "answers")
                k += 1
    # the same call without the constraint: the untrained generator names invalid programs
    free = predict_answers(pg, nmn, batches, vocab, beam_size=4, constrained=False)
    assert free == predict_answers(pg, nmn, batches, vocab, beam_size=4)
    assert sum(not r["program_valid"] for r in free) >= 1
