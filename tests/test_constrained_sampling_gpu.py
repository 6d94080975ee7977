"""Sampling and greedy decoding under the grammar automaton inside the persistent decoder kernels
(the tables of ``pnmn_attn_lstm_fwd`` and ``pnmn_attn_lstm_fwd_group``; ``Seq2SeqBase.decode_constrained``,
``predict_answers(constrained_sampling=True)``), token for token against the fp64 host reference of
tests/helpers/constrained_choice.py: one workgroup per tile and multi-CU, the identity filter, every filter of
tests/helpers/filtered_inputs.py and the greedy mode, the paired launch, a row that is not finite, the argument checks of the C
entry points and the model surface.

The check REPLAYS the device: for every (row, t) the row's automaton state is rebuilt from the kernel's OWN earlier tokens,
the logits come from the kernel's own h_t in fp64 and the uniform from ``kernel_uniform``; the kernel's token must be the
reference's.  The excuse rule is that of tests/test_filtered_sampling_gpu.py: a sampled row within ``fi.DECODER_DELTA`` of one
of the rule's decisions (the reference's margin) may differ, but must still be in A_c and inside the kept set widened by one
rank, and at most ``fi.excused_cap(rows)`` rows of a case are so marked -- twice what tests/test_constrained_choice_ref.py
allows the reference itself.  A greedy row has no such excuse: it matches exactly (an exact tie takes the first index on both
sides)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import constrained_choice as cc  # noqa: E402
import filtered_inputs as fi  # noqa: E402
from filtered_choice import kernel_uniform, ranks_within_allowed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, UNK, START, END = fi.PAD, fi.UNK, fi.START, 3
H, V = 256, 44
IDENTITY = (1.0, 0, 1.0)
SHAPES = [(1, 1, 1), (7, 5, 3), (17, 12, 20), (64, 12, 20), (130, 9, 27), (33, 2, 5), (33, 30, 40)]  # (B, T, S)
CASES = [(IDENTITY, 99, 16)] + fi.decoder_filter_cases()  # (filter, seed, row offset)


@pytest.fixture(scope="module")
def grammar():
    """(compiler, automaton, reference tables, ``meta["constraint"]``) of the CLEVR program vocabulary."""
    from probnmn.modules.seq2seq_base import constraint_tables
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    assert vocab.get_vocab_size("programs") == V and vocab.get_token_index("@end@", namespace="programs") == END
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    auto = comp.decoding_automaton(exclude=(PAD, UNK, START, END))
    return comp, auto, cc.Tables(auto, END), constraint_tables(auto, V, END)


def _decoder_inputs(B, S, seed):
    return {k: v.to(DEV) for k, v in fi.decoder_inputs(B, S, V, seed).items()}


def _decode(d, mode, T, seed, row_offset, filt=None, constraint=None, h0=None, in_tokens=None):
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoder

    with torch.no_grad():
        hs, tok = _AttnLSTMDecoder.apply(None, d["etable"], d["enc"], d["mask"], d["h0"] if h0 is None else h0, d["w_c"],
                                         d["w_hh"], d["w_p"] if mode else None, d["b_p"] if mode else None, mode, T, seed,
                                         row_offset, PAD, UNK, START, None, in_tokens, filt, constraint)
    torch.cuda.synchronize()
    return hs, tok


def _teacher_forced(d, tok):
    B, T = tok.shape
    return _decode(d, 0, T, 0, 0, in_tokens=torch.cat((tok.new_full((B, 1), START), tok[:, :-1]), 1))[0]


def _masks(tab, tok):
    """A_c [B * T, V] of every (row, step), the states rebuilt from the rows' own tokens; and which (row, step) are live."""
    B, T = tok.shape
    state, finished = cc.states_of(tab, tok)
    masks = np.stack([cc.allowed_mask(tab, state[:, t], finished[:, t], t, T, V, PAD, UNK, START) for t in range(T)], 1)
    return masks.reshape(B * T, V), ~finished.reshape(-1)


def _check_tokens(tab, hs, tok, w_p, b_p, seed, row_offset, filt, greedy, what):
    """Check (1) of the module docstring on one decode; returns how many rows the reference marked."""
    B, T, _ = hs.shape
    assert tok.shape == (B, T)
    tok = tok.cpu().numpy()
    assert tok.min() >= 0 and tok.max() < V, what
    logits = (hs.double() @ w_p.double().t() + b_p.double()).cpu().numpy().reshape(B * T, V)
    masks, live = _masks(tab, tok)
    flat = tok.reshape(-1)
    assert masks[np.arange(B * T), flat].all(), "%s: a token outside A_c" % what
    if greedy:
        ref, gap = cc.constrained_greedy_ref(logits, masks)
        with np.errstate(invalid="ignore"):
            print("%s: greedy, smallest gap between the two largest logits of a set %g" % (what, np.nanmin(gap)))
        bad = np.flatnonzero(flat != ref)
        assert bad.size == 0, "%s: %d of %d greedy tokens differ; rows %s got %s want %s (gaps %s)" % (
            what, bad.size, B * T, bad[:8].tolist(), flat[bad[:8]].tolist(), ref[bad[:8]].tolist(), gap[bad[:8]].tolist())
        return 0
    rows = row_offset + np.arange(B, dtype=np.uint64)[:, None]
    u = kernel_uniform(seed, rows, np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
    ref, margin, kept = cc.constrained_sample_ref(logits, u, masks, PAD, UNK, START, *filt)
    marked = margin < fi.DECODER_DELTA
    print("%s: %d of %d rows (%d live) within %g of a decision, %d of them differ" % (
        what, int(marked.sum()), B * T, int(live.sum()), fi.DECODER_DELTA, int((flat != ref)[marked].sum())))
    bad = np.flatnonzero((flat != ref) & ~marked)
    assert bad.size == 0, "%s: %d of %d draws differ from the reference; rows %s got %s want %s (margins %s)" % (
        what, bad.size, B * T, bad[:8].tolist(), flat[bad[:8]].tolist(), ref[bad[:8]].tolist(), margin[bad[:8]].tolist())
    differ = np.flatnonzero((flat != ref) & marked)
    if differ.size:  # still inside the kept set widened by one rank (the ranking is that within A_c)
        inside = np.where(masks[differ], logits[differ], -np.inf)
        rank = ranks_within_allowed(inside, PAD, UNK, START, filt[0])[np.arange(differ.size), flat[differ]]
        assert (rank <= kept[differ].sum(1)).all(), (what, differ[:8].tolist(), flat[differ[:8]].tolist())
    assert int(marked.sum()) <= fi.excused_cap(B * T), (what, int(marked.sum()), B * T)
    return int(marked.sum())


def _assert_valid(comp, auto, tok, what):
    """Check (2): every row, cut at its first end, is accepted by the automaton and by the compiler; all end behind it."""
    for r, row in enumerate(tok.cpu().tolist()):
        program = cc.cut_at_end(row, END)
        assert auto.accepts(program) and comp.compile(program).valid, (what, r, row)
        assert set(row[len(program):]) <= {END}, (what, r, row)


def _count_invalid(comp, tok):
    return sum(not comp.compile(cc.cut_at_end(row, END)).valid for row in tok.cpu().tolist())


# ---- 1-3. token for token, validity, replay ---------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", ["0", "1"])
@pytest.mark.parametrize("B,T,S", SHAPES)
def test_constrained_decoder_chooses_the_reference_token(grammar, B, T, S, cluster, monkeypatch):
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    comp, auto, tab, constraint = grammar
    d = _decoder_inputs(B, S, B + T + S + V)
    invalid_unconstrained = 0
    for filt, seed, row_offset in CASES + [(None, 0, 0)]:
        greedy = filt is None
        what = "cluster=%s B=%d T=%d S=%d %s seed=%d offset=%d" % (cluster, B, T, S, "greedy" if greedy else "filter=%s" % (filt,),
                                                                    seed, row_offset)
        hs, tok = _decode(d, 2 if greedy else 1, T, seed, row_offset, None if greedy else filt, constraint)
        _check_tokens(tab, hs, tok, d["w_p"], d["b_p"], seed, row_offset, filt, greedy, what)
        _assert_valid(comp, auto, tok, what)
        torch.testing.assert_close(_teacher_forced(d, tok), hs, rtol=1e-6, atol=1e-7, msg=lambda m: "%s: %s" % (what, m))
        if not greedy:
            invalid_unconstrained += _count_invalid(comp, _decode(d, 1, T, seed, row_offset, filt)[1])
    if B >= 7:  # (one row of one step may be valid by chance)
        assert invalid_unconstrained > 0, "the same seeds unconstrained leave no invalid row: the inputs do not discriminate"


# ---- 4. the trivial automaton -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", ["0", "1"])
@pytest.mark.parametrize("B,T,S", [(17, 12, 20), (130, 9, 27), (33, 30, 40)])
def test_trivial_automaton_is_the_unconstrained_sampling_decode(B, T, S, cluster, monkeypatch):
    """One state, one class, min_left = {0}: A_c is "all but pad / unk / start" until the row's first end."""
    from probnmn.modules.seq2seq_base import constraint_tables

    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    trivial = constraint_tables(cc.trivial_tables(V, END)[1], V, END)
    d = _decoder_inputs(B, S, 3 * B + T)
    ended = 0
    for filt, seed, row_offset in CASES[:3]:
        hs, tok = _decode(d, 1, T, seed, row_offset, filt)
        hs_c, tok_c = _decode(d, 1, T, seed, row_offset, filt, trivial)
        is_end = (tok == END).long()
        upto = (torch.cumsum(is_end, 1) - is_end) == 0  # steps up to and including the row's first end
        ended += int((~upto).any(1).sum())
        assert torch.equal(tok_c[upto], tok[upto]), (filt, seed)
        assert torch.equal(hs_c[upto], hs[upto]), (filt, seed)
        assert bool((tok_c[~upto] == END).all())
    assert ended > 0  # (some rows did end early: the frozen tail was exercised)


# ---- 5. the paired launch ---------------------------------------------------------------------------------------------
def test_paired_launch_constrains_the_free_running_side_only(grammar):
    """7 constrained-sampling rows beside 20 teacher-forced rows in one launch, in either order."""
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoderGroup

    comp, auto, tab, constraint = grammar
    T, S = 12, 20
    a, b = _decoder_inputs(7, S, 8), _decoder_inputs(20, S, 22)
    tf_tokens = torch.randint(3, V, (20, T), generator=torch.Generator().manual_seed(20)).to(DEV)
    alone = _decode(b, 0, T, 0, 0, in_tokens=tf_tokens)[0]
    for order, (filt, seed, row_offset) in enumerate(((IDENTITY, 2 ** 62 - 1, 0), (fi.FILTERS[2], 77, 2 ** 32 - 5))):
        meta_a = dict(packs=None, mode=1, T=T, start=START, pad=PAD, unk=UNK, seed=seed, row_offset=row_offset, w_p=a["w_p"],
                      b_p=a["b_p"], filter=filt, constraint=constraint)
        meta_b = dict(packs=None, mode=0, T=T, start=START, in_tokens=tf_tokens)
        ta = (a["etable"], a["enc"], a["mask"], a["h0"], a["w_c"], a["w_hh"])
        tb = (b["etable"], b["enc"], b["mask"], b["h0"], b["w_c"], b["w_hh"])
        with torch.no_grad():
            if order == 0:
                hs_a, tok_a, hs_b, _ = _AttnLSTMDecoderGroup.apply(*ta, *tb, (meta_a, meta_b), None)
            else:
                hs_b, _, hs_a, tok_a = _AttnLSTMDecoderGroup.apply(*tb, *ta, (meta_b, meta_a), None)
        torch.cuda.synchronize()
        what = "pair 7 + 20 filter=%s seed=%d offset=%d order=%d" % (filt, seed, row_offset, order)
        _check_tokens(tab, hs_a, tok_a, a["w_p"], a["b_p"], seed, row_offset, filt, False, what)
        _assert_valid(comp, auto, tok_a, what)
        torch.testing.assert_close(_teacher_forced(a, tok_a), hs_a, rtol=1e-6, atol=1e-7)
        assert torch.equal(hs_b, alone)  # (the teacher-forced side: bit for bit its run alone)


# ---- 6. a row that is not finite --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("cluster", ["0", "1"])
def test_nonfinite_row_takes_the_lowest_allowed_index_and_stays_to_itself(grammar, cluster, mode, monkeypatch):
    """h0 = NaN in one row: every logit of it is NaN, so at every step it emits the lowest index of A_c -- still a valid
    program -- and every other row is bit for bit that of a run without the NaN."""
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    comp, auto, tab, constraint = grammar
    B, T, S = 33, 12, 20
    d = _decoder_inputs(B, S, 31 + B)
    bad = 17
    h0 = d["h0"].clone()
    h0[bad] = float("nan")
    good = torch.ones(B, dtype=torch.bool, device=DEV)
    good[bad] = False
    for filt in (None, fi.FILTERS[0]) if mode == 1 else (None,):
        hs_ref, tok_ref = _decode(d, mode, T, 99, 16, filt, constraint)
        hs, tok = _decode(d, mode, T, 99, 16, filt, constraint, h0=h0)
        assert bool(torch.isnan(hs[bad]).all())
        masks, _ = _masks(tab, tok[bad:bad + 1].cpu().numpy())
        assert tok[bad].cpu().tolist() == masks.argmax(1).tolist(), (mode, filt)
        _assert_valid(comp, auto, tok, "NaN row")
        assert torch.equal(hs[good], hs_ref[good]) and torch.equal(tok[good], tok_ref[good])


# ---- 7. PNMN_EINVAL ---------------------------------------------------------------------------------------------------
def test_constrained_entry_points_refuse_bad_arguments_and_launch_nothing(grammar):
    from probnmn import _hip
    from probnmn.modules.seq2seq_base import _decoder_workspace, _prepare_decoder_side

    comp, auto, tab, (tc, ns, ml, _) = grammar
    lib, dev = _hip.lib(), torch.device(DEV)
    B, T, S = 20, 4, 5
    d = _decoder_inputs(B, S, 5)
    meta = dict(packs=None, mode=1, T=T, start=START, pad=PAD, unk=UNK, seed=1, row_offset=0, w_p=d["w_p"], b_p=d["b_p"])
    jobs = np.zeros(2, _hip.DECODER_FWD_JOB)
    sides = [_prepare_decoder_side(jobs, k, d["etable"], d["enc"], d["mask"], d["h0"], d["w_c"], d["w_hh"], meta) for k in (0, 1)]
    ws = _decoder_workspace([B, B], False, dev)
    n_states, n_classes = ns.shape
    good_filter = np.array([(1.0, 0, 1.0, 0), (0.7, 5, 0.9, 0)], _hip.SAMPLING_FILTER)

    def with_entry(table, index, value):
        out = table.copy()
        out.reshape(-1)[index] = value
        return out

    long_left = with_entry(ml, 0, T + 1)  # the shortest accepted string does not fit the steps
    ok = dict(filt=good_filter, end=END, tc=tc, ns=ns, ml=ml, n_states=n_states, n_classes=n_classes)
    bad_calls = [dict(tc=None), dict(ns=None), dict(ml=None),
                 dict(tc=with_entry(tc, V - 1, n_classes)), dict(tc=with_entry(tc, 0, 255)),
                 dict(ns=with_entry(ns, n_states * n_classes - 1, n_states)), dict(ns=with_entry(ns, 0, 255)),
                 dict(n_states=0), dict(n_states=_hip.BEAM_MAX_STATES + 1), dict(n_classes=0), dict(n_classes=_hip.BEAM_MAX_CLASSES + 1),
                 dict(end=-1), dict(end=V), dict(ml=long_left),
                 dict(filt=np.array([(0.0, 0, 1.0, 0)] * 2, _hip.SAMPLING_FILTER)),
                 dict(filt=np.array([(1.0, -1, 1.0, 0)] * 2, _hip.SAMPLING_FILTER)),
                 dict(filt=np.array([(1.0, 0, float("nan"), 0)] * 2, _hip.SAMPLING_FILTER))]
    ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731

    def calls(c):
        tail = (c["end"], ptr(c["tc"]), ptr(c["ns"]), ptr(c["ml"]), c["n_states"], c["n_classes"])
        return fi.decoder_entry_calls(jobs, sides, ws, c["filt"], tail)

    for change in [{}] + bad_calls:
        for entry, rc, outputs in calls({**ok, **change}):
            assert rc == (_hip.EINVAL if change else 0), (change, entry)
            tokens = outputs[2::3] if entry == "group n=2" else outputs[2:3]  # (of the jobs the call covers)
            if change:
                assert all(bool((t == -7).all()) for t in outputs), (change, entry)
            else:
                assert all(bool((t >= 0).all()) for t in tokens), entry
    # a null filter under the automaton is not an error: the identity for every job, bit for bit
    identity = np.array([(1.0, 0, 1.0, 0)] * 2, _hip.SAMPLING_FILTER)
    for (entry, rc_n, out_n), (_, rc_r, out_r) in zip(calls({**ok, "filt": None}), calls({**ok, "filt": identity})):
        assert rc_n == 0 and rc_r == 0, entry
        assert bool((out_n[2] >= 0).all()), entry
        assert all(torch.equal(a, b) for a, b in zip(out_n, out_r)), entry  # (hs, cs and tokens of every job)


# ---- 8. the model surface ---------------------------------------------------------------------------------------------
def _generator(steps=12, **kw):
    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(3)
    return vocab, ProgramGenerator(vocab, max_decoding_steps=steps, **kw).to(DEV)


def test_decode_constrained_surface(grammar):
    comp, auto, tab, _ = grammar
    vocab, pg = _generator()
    B, T = 21, 12
    q = torch.randint(4, vocab.get_vocab_size("questions"), (B, 9), generator=torch.Generator().manual_seed(1)).to(DEV)
    outs = {}
    for mode in ("eval", "train"):
        getattr(pg, mode)()
        for strategy in ("constrained_sampling", "constrained_greedy"):
            torch.manual_seed(11)
            out = pg(q, decoding_strategy=strategy, constraint=auto)
            assert sorted(out) == ["loss", "predictions"]
            assert out["predictions"].shape == (B, T) and out["predictions"].dtype == torch.long
            assert out["loss"].shape == (B,) and out["loss"].dtype == torch.float32
            assert not out["predictions"].requires_grad and not out["loss"].requires_grad and out["loss"].grad_fn is None
            assert bool(torch.isfinite(out["loss"]).all())
            for row in out["predictions"].cpu().tolist():  # trimmed: padding behind the first end
                program = cc.cut_at_end(row, END)
                assert comp.compile(program).valid and auto.accepts(program), row
                assert set(row[len(program) + 1:]) <= {PAD}
            outs[mode, strategy] = out
    for strategy in ("constrained_sampling", "constrained_greedy"):  # the same in train() and eval() mode
        assert torch.equal(outs["eval", strategy]["predictions"], outs["train", strategy]["predictions"])
        assert torch.equal(outs["eval", strategy]["loss"], outs["train", strategy]["loss"])
    pg.eval()
    with torch.no_grad():
        # loss: as the sampling decode reports it, under the UNMODIFIED distribution -- under the trivial automaton, which
        # changes no token before a row's end, predictions and loss are those of the sampling decode from the same seed
        state = pg.encode(q, dropout=False)
        trivial = cc.trivial_tables(V, END)[1]
        for kw in ({}, dict(temperature=0.7, top_k=8)):
            sampled = pg.decode(state, seed=77, **kw)
            under = pg.decode_constrained(state, trivial, seed=77, **kw)
            assert torch.equal(under["predictions"], sampled["predictions"]) and torch.equal(under["loss"], sampled["loss"])
        # the generator advances as one sampling call advances it; a greedy constrained call draws nothing
        torch.manual_seed(5)
        pg(q)
        after_sampling = torch.get_rng_state()
        torch.manual_seed(5)
        first = pg(q, decoding_strategy="constrained_sampling", constraint=auto, top_k=10)
        assert torch.equal(torch.get_rng_state(), after_sampling)
        torch.manual_seed(5)
        before = torch.get_rng_state()
        pg(q, decoding_strategy="constrained_greedy", constraint=auto)
        assert torch.equal(torch.get_rng_state(), before)
        torch.manual_seed(5)
        again = pg.decode(pg.encode(q, dropout=False), decoding_strategy="constrained_sampling", constraint=auto, top_k=10)
        assert torch.equal(again["predictions"], first["predictions"]) and torch.equal(again["loss"], first["loss"])
        torch.manual_seed(6)
        other = pg(q, decoding_strategy="constrained_sampling", constraint=auto, top_k=10)
        assert not torch.equal(other["predictions"], first["predictions"])
        same = pg.decode_constrained(pg.encode(q, dropout=False), auto, seed=1234)
        assert torch.equal(pg.decode_constrained(pg.encode(q, dropout=False), auto, seed=1234)["predictions"], same["predictions"])
    # refusals
    for strategy in ("constrained_sampling", "constrained_greedy"):
        with pytest.raises(ValueError):
            pg(q, decoding_strategy=strategy)
        with pytest.raises(ValueError):
            pg(q, q[:, :5], decoding_strategy=strategy, constraint=auto)
        with pytest.raises(ValueError):
            pg(q, decoding_strategy=strategy, constraint=SimpleNamespace(token_class=auto.token_class[:-1], next_state=auto.next_state,
                                                                        min_left=auto.min_left))
    with pytest.raises(ValueError):
        pg(q, decoding_strategy="constrained_greedy", constraint=auto, temperature=0.7)
    long_left = np.array(auto.min_left)
    long_left[0] = T + 1
    with pytest.raises(ValueError):
        pg(q, decoding_strategy="constrained_sampling",
           constraint=SimpleNamespace(token_class=auto.token_class, next_state=auto.next_state, min_left=long_left))
    for strategy in ("sampling", "greedy"):  # (the old refusals still hold)
        with pytest.raises(ValueError):
            pg(q, decoding_strategy=strategy, constraint=auto)
        with pytest.raises(ValueError):
            pg.decode(pg.encode(q), decoding_strategy=strategy, constraint=auto)
    with pytest.raises(ValueError):
        pg(q, decoding_strategy="nonsense")
    _, small = _generator(input_size=128, hidden_size=128)
    small.eval()
    with torch.no_grad():
        small(q)  # (the step-by-step path still samples)
    for strategy in ("constrained_sampling", "constrained_greedy"):
        with pytest.raises(NotImplementedError):
            small(q, decoding_strategy=strategy, constraint=auto)


# ---- 9. predict_answers -----------------------------------------------------------------------------------------------
def test_predict_answers_samples_valid_programs_only(grammar):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import predict_answers
    from probnmn.models import NeuralModuleNetwork

    vocab, pg = _generator(steps=26)
    pg.eval()
    nmn = NeuralModuleNetwork(vocab).to(DEV).eval()
    batches = [{k: v.to(DEV) for k, v in synthetic_batch(vocab, 6, seed=s).items()} for s in (8, 9)]
    comp = nmn.engine.compiler
    torch.manual_seed(21)
    records = predict_answers(pg, nmn, batches, vocab, constrained_sampling=True, temperature=0.9, top_k=20)
    assert len(records) == 12
    for i, r in enumerate(records):
        assert sorted(r) == ["answer", "program", "program_valid", "question_index"]
        assert r["program_valid"] is True
        tokens = [vocab.get_token_index(t, namespace="programs") for t in r["program"]]
        assert comp.compile(cc.cut_at_end(tokens, END)).valid, r
        # the answer is the NMN's on the named program
        batch = batches[i // 6]
        program = torch.zeros(1, 26, dtype=torch.long, device=DEV)
        program[0, :len(tokens)] = torch.tensor(tokens, device=DEV)
        with torch.no_grad():
            answer = int(nmn(batch["image"][i % 6: i % 6 + 1], program)["predictions"][0])
        assert r["answer"] == vocab.get_token_from_index(answer, namespace="answers"), (i, r)
    # without the flag: the sampled pipeline as it was, from the same torch seed
    torch.manual_seed(21)
    plain = predict_answers(pg, nmn, batches, vocab)
    torch.manual_seed(21)
    want = []
    with torch.no_grad():
        programs = [pg(b["question"])["predictions"] for b in batches]  # (the loop queues every generator pass first)
        for b, p in zip(batches, programs):
            want += nmn(b["image"], p)["predictions"].cpu().tolist()
    assert all(sorted(r) == ["answer", "question_index"] for r in plain)
    assert [r["answer"] for r in plain] == [vocab.get_token_from_index(int(a), namespace="answers") for a in want]
    with pytest.raises(ValueError):
        predict_answers(pg, nmn, batches, vocab, beam_size=4, constrained_sampling=True)
    with pytest.raises(ValueError):
        predict_answers(pg, nmn, batches, vocab, constrained=True)  # (pinned: needs beam_size)
