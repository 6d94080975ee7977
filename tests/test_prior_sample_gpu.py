"""``pnmn_prior_sample``: free-running samples from the program prior in one persistent launch, and ``ProgramPrior.sample`` /
``sample_programs`` on top of it.  Forced tokens against the oracle; the draws token for token against the fp64 host
reference of tests/helpers/filtered_choice.py on logits taken from the kernel's OWN projection; self-consistency, row
independence, the identity filter and the greedy mode, the grammar automaton, rows that are not finite, the argument checks
of the C entry point, and the model surface.

The excusing rule of a sampled row is that of tests/test_filtered_sampling_gpu.py (``_check_filtered``, used as it is): a row
within ``fi.DECODER_DELTA`` of one of the rule's decisions may differ but stays inside the kept set widened by one rank, at
most ``fi.excused_cap(rows)`` rows of a case are so marked -- twice what tests/test_prior_sample_ref.py allows the reference
itself -- and every other row matches exactly."""
import os
import sys

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.join(_HERE, "helpers"))
import constrained_choice as cc  # noqa: E402
import filtered_inputs as fi  # noqa: E402
import prior_inputs as pi  # noqa: E402
from test_filtered_sampling_gpu import _check_filtered  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, UNK, START, END = pi.PAD, pi.UNK, pi.START, pi.END
H = 256


def _device_weights(w):
    from probnmn.models.program_prior import PriorSampleWeights
    from probnmn.modules.seq2seq_base import pack_fragments

    d = {k: v.to(DEV).contiguous() for k, v in w.items()}
    return PriorSampleWeights(d["table0"], *(pack_fragments(d[k]) for k in ("w_hh0", "w_ih1", "w_hh1")), d["b1"],
                              pack_fragments(d["w_proj"]), d["w_out"], PAD, UNK, START)


def _run(dw, B, T, mode, seed=0, row_offset=0, forced=None, filt=None, constraint=None, want_proj=True):
    from probnmn.models.program_prior import prior_sample_call

    out = prior_sample_call(dw, B, T, mode, seed, row_offset, forced, filt, constraint, want_proj)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def cases():
    """{(B, T, V): (host weights, device weights)}: built once, shared, never modified."""
    out = {}
    for B, T, V in pi.SHAPES:
        w = pi.prior_weights(B, T, V)
        out[(B, T, V)] = (w, _device_weights(w))
    return out


@pytest.fixture(scope="module")
def grammar():
    from probnmn.modules.seq2seq_base import constraint_tables
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    assert vocab.get_vocab_size("programs") == 44 and vocab.get_token_index("@end@", namespace="programs") == END
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    auto = comp.decoding_automaton(exclude=(PAD, UNK, START, END))
    return vocab, comp, auto, constraint_tables(auto, 44, END)


def _prior(vocab, seed=4):
    from probnmn.models import ProgramPrior

    torch.manual_seed(seed)
    return ProgramPrior(vocab, hidden_size=256).to(DEV).eval()


def _logits64(proj, w_out):
    B, T, _ = proj.shape
    return (proj.double() @ w_out.double().t()).cpu().numpy().reshape(B * T, -1)


def _check_logprobs(tok, lp_vocab, lp_proj, proj, z64, what):
    """Both log-probabilities against fp64 log_softmax of the kernel's own projection / of the logits made from it."""
    flat = tok.cpu().numpy().reshape(-1)
    n = np.arange(flat.size)
    want_v = torch.log_softmax(torch.from_numpy(z64), 1).numpy()[n, flat]
    want_p = torch.log_softmax(proj.double().reshape(flat.size, H), 1).cpu().numpy()[n, flat]
    np.testing.assert_allclose(lp_vocab.cpu().numpy().reshape(-1), want_v, rtol=1e-5, atol=1e-5, err_msg=what)
    np.testing.assert_allclose(lp_proj.cpu().numpy().reshape(-1), want_p, rtol=1e-5, atol=1e-5, err_msg=what)


# ---- 1. forced tokens against the oracle ------------------------------------------------------------------------------
def test_forced_tokens_match_the_oracle(grammar):
    from oracle import seq2seq_oracle as so
    from probnmn.models.program_prior import prior_sample_launch

    torch.manual_seed(4)
    from probnmn.models import ProgramPrior

    prior = ProgramPrior(grammar[0], hidden_size=256)
    sd = {k: v.detach().clone() for k, v in prior.state_dict().items() if k != "_output_layer.weight"}
    prior.to(DEV).eval()
    g = torch.Generator().manual_seed(12)
    forced = torch.randint(3, 44, (9, 27), generator=g)
    forced[0, 0] = END   # starts with @end@ -> all padding
    forced[1] = 9        # never ends -> kept whole
    raw, lp_vocab, lp_proj, _ = prior_sample_launch(prior, 9, 27, 0, 0, forced=forced.to(DEV))
    assert torch.equal(raw.cpu(), forced)
    got = prior._trim_and_sort(raw, lp_proj, lp_vocab)
    want = so.program_prior_sample(sd, forced, 28)
    assert torch.equal(got["predictions"].cpu(), want["predictions"])
    torch.testing.assert_close(got["loss"].cpu(), want["loss"], rtol=1e-4, atol=1e-5)
    # the torch loop behind ``_forced`` is still there and agrees
    loop = prior.sample(9, 28, _forced=forced)
    assert torch.equal(loop["predictions"], got["predictions"])
    torch.testing.assert_close(loop["loss"], got["loss"], rtol=1e-4, atol=1e-5)


# ---- 2 / 3. the draws token for token; mode 0 reproduces a mode 1 run ---------------------------------------------------
@pytest.mark.parametrize("B,T,V", pi.SHAPES)
def test_draws_are_the_reference_tokens(cases, B, T, V):
    w, dw = cases[(B, T, V)]
    for filt, seed, row_offset in pi.prior_filter_cases(V):
        what = "B=%d T=%d V=%d filter=%s seed=%d offset=%d" % (B, T, V, filt, seed, row_offset)
        tok, lp_vocab, lp_proj, proj = _run(dw, B, T, 1, seed, row_offset, filt=None if filt == pi.IDENTITY else filt)
        z64 = _logits64(proj, dw.w_out)
        _check_filtered(tok.cpu().numpy().reshape(-1), z64, pi.uniforms(seed, row_offset, B, T), filt, fi.DECODER_DELTA, what)
        _check_logprobs(tok, lp_vocab, lp_proj, proj, z64, what)
        # self-consistency: the same tokens forced give the same projection
        tok0, lp_vocab0, lp_proj0, proj0 = _run(dw, B, T, 0, forced=tok)
        assert torch.equal(tok0, tok), what
        torch.testing.assert_close(proj0, proj, rtol=1e-6, atol=1e-7, msg=lambda m: "%s: %s" % (what, m))
        torch.testing.assert_close(lp_vocab0, lp_vocab, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(lp_proj0, lp_proj, rtol=1e-6, atol=1e-6)


def test_the_kernel_runs_the_stated_arithmetic(cases):
    """The projection of a forced run against the fp64 host emulation of the step arithmetic (fp32 round-off through 12
    steps of two LSTM layers: 1e-4 of the projection's scale)."""
    B, T, V = 17, 12, 100
    w, dw = cases[(B, T, V)]
    forced = torch.randint(3, V, (B, T), generator=torch.Generator().manual_seed(1))
    _, p64, _ = pi.emulate_prior_logits(w, B, T, lambda z, t: forced[:, t].numpy())
    proj = _run(dw, B, T, 0, forced=forced.to(DEV))[3]
    err = float((proj.double().cpu().reshape(B * T, H) - torch.from_numpy(p64)).abs().max())
    assert err < 1e-4 * float(np.abs(p64).max()), (err, float(np.abs(p64).max()))


# ---- 4. row independence ----------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_they_run_in(cases):
    _, dw = cases[(130, 9, 44)]
    for filt, seed, row_offset in ((None, 2 ** 62 - 1, 2 ** 32 - 5), (fi.FILTERS[2], 12345, 16)):
        big = _run(dw, 130, 9, 1, seed, row_offset, filt=filt)
        small = _run(dw, 17, 9, 1, seed, row_offset, filt=filt)
        for a, b in zip(big, small):
            assert torch.equal(a[:17], b)


# ---- 5. the identity filter and the greedy mode ------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,V", [(17, 12, 100), (64, 27, 128)])
def test_identity_filter_is_no_filter_and_greedy_is_the_first_argmax(cases, B, T, V):
    _, dw = cases[(B, T, V)]
    plain = _run(dw, B, T, 1, 99, 16)
    ident = _run(dw, B, T, 1, 99, 16, filt=pi.IDENTITY)
    for a, b in zip(plain, ident):
        assert torch.equal(a, b)
    greedy = _run(dw, B, T, 2)
    greedy_f = _run(dw, B, T, 2, filt=(0.5, 3, 0.5))
    for a, b in zip(greedy, greedy_f):
        assert torch.equal(a, b)
    tok, lp_vocab, lp_proj, proj = greedy
    z64 = _logits64(proj, dw.w_out)
    want = z64.argmax(1)  # (numpy: the first maximum)
    top2 = -np.sort(-z64, 1)[:, :2]
    close = (top2[:, 0] - top2[:, 1]) < fi.DECODER_DELTA
    flat = tok.cpu().numpy().reshape(-1)
    assert ((flat == want) | close).all(), np.flatnonzero((flat != want) & ~close)[:8]
    assert int(close.sum()) <= fi.excused_cap(B * T)
    _check_logprobs(tok, lp_vocab, lp_proj, proj, z64, "greedy")


# ---- 6. the grammar automaton -----------------------------------------------------------------------------------------
def test_constrained_rows_are_valid_programs(grammar):
    from probnmn.models.program_prior import prior_sample_launch

    vocab, comp, auto, tables = grammar
    prior = _prior(vocab)
    invalid_unconstrained = 0
    for B, T in pi.CONSTRAINED_SHAPES:
        T = pi.shortest_steps(auto.min_left) if T is None else T
        for filt, seed, row_offset in pi.constrained_cases():
            greedy = filt is None
            tok = prior_sample_launch(prior, B, T, 2 if greedy else 1, seed, row_offset, None,
                                      None if greedy or filt == pi.IDENTITY else filt, tables)[0]
            for r, row in enumerate(tok.cpu().tolist()):
                program = cc.cut_at_end(row, END)
                assert auto.accepts(program) and comp.compile(program).valid, (B, T, filt, r, row)
                assert set(row[len(program):]) <= {END}, (B, T, filt, r, row)
            if not greedy and T > 1:
                free = prior_sample_launch(prior, B, T, 1, seed, row_offset)[0]
                invalid_unconstrained += sum(not comp.compile(cc.cut_at_end(row, END)).valid for row in free.cpu().tolist())
    assert invalid_unconstrained > 0, "the same seeds unconstrained leave no invalid row: the inputs do not discriminate"


def test_trivial_automaton_is_the_unconstrained_run_up_to_the_first_end(cases):
    from probnmn.modules.seq2seq_base import constraint_tables

    ended = 0
    for (B, T, V), filt, seed, row_offset in (((130, 9, 44), None, 99, 16), ((16, 64, 4), None, 7, 0),
                                              ((64, 27, 128), fi.FILTERS[0], 2 ** 62 - 1, 0)):
        _, dw = cases[(B, T, V)]
        trivial = constraint_tables(cc.trivial_tables(V, END)[1], V, END)
        tok = _run(dw, B, T, 1, seed, row_offset, filt=filt)[0]
        tok_c = _run(dw, B, T, 1, seed, row_offset, filt=filt, constraint=trivial)[0]
        is_end = (tok == END).long()
        upto = (torch.cumsum(is_end, 1) - is_end) == 0  # steps up to and including the row's first end
        ended += int((~upto).any(1).sum())
        assert torch.equal(tok_c[upto], tok[upto]), (B, T, V)
        assert bool((tok_c[~upto] == END).all())
    assert ended > 0  # (some rows did end early: the frozen tail was exercised)


def test_log_probability_is_what_forward_scores(grammar):
    """``forward`` returns the MEAN negative log-likelihood over the program's tokens and its closing @end@ (allennlp's
    ``sequence_cross_entropy_with_logits(average=None)``); ``log_probability`` is the SUM over the same tokens.  So
    loss x token count == -log_probability, on the rows that closed with @end@ inside the steps (a row that fills all
    27 steps has no @end@ among its kept tokens, and ``forward`` scores one more token than ``sample`` kept)."""
    vocab, comp, auto, _ = grammar
    prior = _prior(vocab)
    out = prior.sample(256, 28, seed=11, constraint=auto)
    pred = out["predictions"]
    closed = (pred == END).any(1)
    assert int(closed.sum()) >= 8, int(closed.sum())
    programs = (pred * (pred != END))[closed]  # as the trainers hand them over: no boundary tokens, right-padded
    with torch.no_grad():
        loss = prior(programs, need_predictions=False)["loss"]
    n_tokens = (pred[closed] != PAD).sum(1).float()
    torch.testing.assert_close(loss * n_tokens, -out["log_probability"][closed], rtol=1e-4, atol=1e-4)


# ---- 7. rows that are not finite --------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["inf_w_out", "nan_table0"])
def test_nonfinite_weights_keep_every_token_in_range(cases, what):
    B, T, V = 17, 12, 100
    w, _ = cases[(B, T, V)]
    w = {k: v.clone() for k, v in w.items()}
    if what == "inf_w_out":
        w["w_out"][7] = float("inf")
    else:
        w["table0"][START, 5] = float("nan")  # (the row every sample reads at step 0)
    dw = _device_weights(w)
    trivial = (np.zeros(V, np.uint8), np.zeros((1, 1), np.uint8), np.zeros(1, np.uint8), END)
    for mode, filt, constraint in ((1, None, None), (1, fi.FILTERS[0], None), (2, None, None), (1, fi.FILTERS[2], trivial),
                                   (2, None, trivial)):
        tok = _run(dw, B, T, mode, 5, 0, filt=filt, constraint=constraint)[0]  # (a non-zero return code raises)
        assert int(tok.min()) >= 0 and int(tok.max()) < V, (what, mode, filt)


# ---- 8. PNMN_EINVAL ---------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_and_launches_nothing(cases):
    from probnmn import _hip

    B, T, V = 7, 5, 44
    _, dw = cases[(B, T, V)]
    lib, stream = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    tok = torch.full((B, T), -7, dtype=torch.long, device=DEV)
    lpv, lpp = torch.full((B, T), -7.0, device=DEV), torch.full((B, T), -7.0, device=DEV)
    proj = torch.full((B, T, H), -7.0, device=DEV)
    forced = torch.full((B, T), 5, dtype=torch.long, device=DEV)
    ok_filter = np.array([(0.7, 5, 1.0, 0)], _hip.SAMPLING_FILTER)
    tc, ns, ml = np.zeros(V, np.uint8), np.zeros((1, 1), np.uint8), np.zeros(1, np.uint8)
    weights = ["table0", "w_hh0", "w_ih1", "w_hh1", "b1", "w_proj", "w_out"]

    def call(**kw):
        a = dict(B=B, T=T, V=V, hidden=H, mode=1, in_tokens=None, filter=None, end=END, tc=None, ns=None, ml=None, n_states=0,
                 n_classes=0, tokens=tok.data_ptr(), lpv=lpv.data_ptr(), lpp=lpp.data_ptr(), proj=proj.data_ptr())
        a.update({k: getattr(dw, k).data_ptr() for k in weights})
        a.update(kw)
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.pnmn_prior_sample(*(a[k] for k in weights), a["tokens"], a["lpv"], a["lpp"], a["proj"], a["B"], a["T"], a["V"],
                                     a["hidden"], a["mode"], PAD, UNK, START, 1, 0, a["in_tokens"], T, ptr(a["filter"]), a["end"],
                                     ptr(a["tc"]), ptr(a["ns"]), ptr(a["ml"]), a["n_states"], a["n_classes"], stream)

    full = dict(tc=tc, ns=ns, ml=ml, n_states=1, n_classes=1)
    bad = [dict(hidden=128), dict(V=0), dict(V=129), dict(T=0), dict(B=-1), dict(mode=-1), dict(mode=3), dict(mode=0),
           dict(tokens=None), dict(lpv=None), dict(lpp=None)]
    bad += [{k: None} for k in weights]
    for f in ((0.0, 0, 1.0), (float("nan"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5)):
        bad.append(dict(filter=np.array([(*f, 0)], _hip.SAMPLING_FILTER)))
        bad.append(dict(filter=np.array([(*f, 0)], _hip.SAMPLING_FILTER), mode=2))
    for missing in ("tc", "ns", "ml"):  # some but not all of the tables
        bad.append({**full, missing: None})
    bad += [{**full, "n_states": 0}, {**full, "n_states": 33}, {**full, "n_classes": 0}, {**full, "n_classes": 17},
            {**full, "end": V}, {**full, "end": -1}, {**full, "tc": np.full(V, 1, np.uint8)}, {**full, "ns": np.ones((1, 1), np.uint8)},
            {**full, "ml": np.array([T + 1], np.uint8)}, {**full, "ml": np.array([T + 1], np.uint8), "mode": 2}]
    for kw in bad:
        assert call(**kw) == _hip.EINVAL, kw
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool((lpv == -7.0).all()) and bool((lpp == -7.0).all()) and bool((proj == -7.0).all())
    assert call(B=0) == 0 and call(B=0, tokens=None, lpv=None, lpp=None, proj=None) == 0
    torch.cuda.synchronize()
    assert bool((tok == -7).all())
    # and the same block of arguments is accepted when nothing is wrong with it
    assert call() == 0 and call(filter=ok_filter, **full) == 0 and call(mode=0, in_tokens=forced.data_ptr(), proj=None) == 0
    torch.cuda.synchronize()
    assert bool((tok == 5).all())


# ---- 9. the model surface ---------------------------------------------------------------------------------------------
def test_sample_surface(grammar):
    from probnmn.evaluators import sample_programs

    vocab, comp, auto, _ = grammar
    prior = _prior(vocab)
    a, b, c = prior.sample(64, 28, seed=5), prior.sample(64, 28, seed=5), prior.sample(64, 28, seed=6)
    assert sorted(a) == ["log_probability", "loss", "predictions"]
    assert a["predictions"].shape == (64, 27) and a["loss"].shape == (64,) and a["log_probability"].shape == (64,)
    assert a["predictions"].dtype == torch.long
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["predictions"], c["predictions"])
    torch.manual_seed(21)
    d = prior.sample(64, 28)
    torch.manual_seed(21)
    e = prior.sample(64, 28)
    assert torch.equal(d["predictions"], e["predictions"]) and torch.equal(d["loss"], e["loss"])
    assert not torch.equal(d["predictions"], prior.sample(64, 28)["predictions"])  # (the generator moved on)
    pred = a["predictions"]
    assert not torch.isin(pred, torch.tensor([UNK, START], device=DEV)).any()
    kept = pred != PAD
    assert bool((kept.long().cumsum(1) == torch.arange(1, 28, device=DEV)[None, :])[kept].all())  # no pad inside a kept program
    assert bool(((pred == END).sum(1) <= 1).all())
    assert bool((a["loss"][1:] >= a["loss"][:-1]).all())  # most likely (smallest loss) first
    assert bool((a["log_probability"] <= 0).all())
    # the row key: a shard that starts at row 16 draws what rows 16.. of the whole batch draw (before the sort: by content)
    prior.sample_row_offset = 16
    shard = prior.sample(16, 28, seed=5)
    prior.sample_row_offset = 0
    whole = {tuple(r) for r in prior.sample(32, 28, seed=5)["predictions"].tolist()}
    assert {tuple(r) for r in shard["predictions"].tolist()} <= whole
    # training mode without dropout still takes the kernel; greedy draws nothing
    prior.train()
    assert torch.equal(prior.sample(64, 28, seed=5)["predictions"], a["predictions"])
    prior.eval()
    g = prior.sample(4, 28, greedy=True)
    assert bool((g["predictions"] == g["predictions"][0]).all())
    records = sample_programs(prior, vocab, 48, seed=3, temperature=0.8, top_k=20, constrained=True, compiler=comp)
    assert len(records) == 48 and all(sorted(r) == ["log_probability", "program", "program_valid"] for r in records)
    assert all(r["program_valid"] for r in records)
    assert all(isinstance(t, str) for r in records for t in r["program"])
    plain = sample_programs(prior, vocab, 8, seed=3)
    assert all(sorted(r) == ["log_probability", "program"] for r in plain)


def test_shapes_outside_the_kernel_keep_the_torch_loop(grammar):
    from probnmn.models import ProgramPrior

    torch.manual_seed(0)
    prior = ProgramPrior(grammar[0], hidden_size=128).to(DEV).eval()
    out = prior.sample(5, 10)
    assert sorted(out) == ["loss", "predictions"] and out["predictions"].shape == (5, 9)
    for kw in (dict(seed=1), dict(top_k=3), dict(constraint=grammar[2]), dict(greedy=True)):
        with pytest.raises(NotImplementedError):
            prior.sample(5, 10, **kw)
