"""Sampling under a filter (temperature, top-k, top-p), token for token against the host reference of
tests/helpers/filtered_choice.py: the standalone ``pnmn_sample_tokens`` under a filter (through ``choose_tokens``), the draws
inside the persistent decoder kernels (one workgroup per tile, multi-CU, paired launch), the identity filter, a known
distribution, rows that are not all finite, the argument checks of the C entry points, and the model surface.

The kernels work in fp32 and the reference in fp64, so a row within ``delta`` of one of the rule's decisions (a CDF
boundary, the top-k cut, the top-p boundary: the reference's margin) may come out differently.  Such a row must still get
an allowed token inside the kept set widened by one rank; the rows the reference marks are at most 5 % of a case + 5,
twice what tests/test_filtered_choice_ref.py allows the reference itself; every other row matches exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filtered_inputs as fi  # noqa: E402
from filtered_choice import filtered_sample_ref, kernel_uniform, ranks_within_allowed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, UNK, START = fi.PAD, fi.UNK, fi.START
H = 256


def _check_filtered(tok, logits64, u, filt, delta, what):
    """The excusing rule of the module docstring; returns how many rows the reference marked."""
    N, V = logits64.shape
    ref, margin, kept = filtered_sample_ref(logits64, u, PAD, UNK, START, *filt)
    marked = margin < delta
    print("%s: %d of %d rows within %g of a decision, %d of them differ" % (what, int(marked.sum()), N, delta,
                                                                           int((tok != ref)[marked].sum())))
    assert tok.min() >= 0 and tok.max() < V, what
    bad = np.flatnonzero((tok != ref) & ~marked)
    assert bad.size == 0, "%s: %d of %d draws differ from the reference; rows %s got %s want %s (margins %s)" % (
        what, bad.size, N, bad[:8].tolist(), tok[bad[:8]].tolist(), ref[bad[:8]].tolist(), margin[bad[:8]].tolist())
    differ = np.flatnonzero((tok != ref) & marked)
    if differ.size:
        rank = ranks_within_allowed(logits64[differ], PAD, UNK, START, filt[0])[np.arange(differ.size), tok[differ]]
        allowed = (tok[differ] != PAD) & (tok[differ] != UNK) & (tok[differ] != START)
        assert (allowed & (rank <= kept[differ].sum(1))).all(), (what, differ[:8].tolist(), tok[differ[:8]].tolist())
    assert int(marked.sum()) <= fi.excused_cap(N), (what, int(marked.sum()), N)
    return int(marked.sum())


# ---- a. the standalone kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", fi.STANDALONE_V)
def test_filtered_sample_tokens_kernel_draws_the_reference_token(V):
    from probnmn.modules.seq2seq_base import choose_tokens

    for logits, seed, step, row_offset in fi.standalone_inputs(V):
        B = logits.size(0)
        z64 = logits.double().numpy()
        u = kernel_uniform(seed, row_offset + np.arange(B, dtype=np.uint64), step)
        want_lp = torch.log_softmax(logits.double(), 1).numpy()
        dlogits = logits.to(DEV)
        for filt in fi.FILTERS:
            tok, lp = choose_tokens(dlogits, False, seed, row_offset, step, PAD, UNK, START, *filt)
            tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
            what = "V=%d B=%d seed=%d step=%d offset=%d filter=%s" % (V, B, seed, step, row_offset, filt)
            _check_filtered(tok, z64, u, filt, fi.STANDALONE_DELTA, what)
            np.testing.assert_allclose(lp, want_lp[np.arange(B), tok], rtol=1e-5, atol=1e-5, err_msg=what)


# ---- b. draws inside the decoder kernels ------------------------------------------------------------------------------
def _decoder_inputs(B, S, V, seed):
    return {k: v.to(DEV) for k, v in fi.decoder_inputs(B, S, V, seed).items()}


def _decode(d, mode, T, seed, row_offset, filt=None, h0=None, in_tokens=None):
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoder

    with torch.no_grad():
        hs, tok = _AttnLSTMDecoder.apply(None, d["etable"], d["enc"], d["mask"], d["h0"] if h0 is None else h0, d["w_c"],
                                         d["w_hh"], d["w_p"] if mode else None, d["b_p"] if mode else None, mode, T, seed,
                                         row_offset, PAD, UNK, START, None, in_tokens, filt)
    torch.cuda.synchronize()
    return hs, tok


def _teacher_forced(d, tok):
    B, T = tok.shape
    return _decode(d, 0, T, 0, 0, in_tokens=torch.cat((tok.new_full((B, 1), START), tok[:, :-1]), 1))[0]


def _check_decoder_tokens(hs, tok, w_p, b_p, seed, row_offset, filt, what):
    """Every (row, t) on its own: logits from the kernel's own h_t in fp64, counter (seed, row_offset + row, t)."""
    B, T, _ = hs.shape
    assert tok.shape == (B, T)
    logits = (hs.double() @ w_p.double().t() + b_p.double()).cpu().numpy().reshape(B * T, -1)
    rows = row_offset + np.arange(B, dtype=np.uint64)[:, None]
    u = kernel_uniform(seed, rows, np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
    return _check_filtered(tok.cpu().numpy().reshape(-1), logits, u, filt, fi.DECODER_DELTA, what)


@pytest.mark.parametrize("cluster", ["0", "1"])
@pytest.mark.parametrize("B,T,S,V", fi.DECODER_SHAPES)
def test_decoder_draws_the_filtered_reference_token(B, T, S, V, cluster, monkeypatch):
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    d = _decoder_inputs(B, S, V, B + T + S + V)
    for filt, seed, row_offset in fi.decoder_filter_cases():
        what = "cluster=%s B=%d T=%d S=%d V=%d filter=%s seed=%d offset=%d" % (cluster, B, T, S, V, filt, seed, row_offset)
        hs, tok = _decode(d, 1, T, seed, row_offset, filt)
        _check_decoder_tokens(hs, tok, d["w_p"], d["b_p"], seed, row_offset, filt, what)
        torch.testing.assert_close(_teacher_forced(d, tok), hs, rtol=1e-6, atol=1e-7, msg=lambda m: "%s: %s" % (what, m))


def test_paired_launch_draws_the_filtered_reference_token():
    """A filtered sampling pass (7 rows) beside a teacher-forced one (20 rows) in one launch."""
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoderGroup

    T, S, V = 12, 20, 44
    a, b = _decoder_inputs(7, S, V, 8), _decoder_inputs(20, S, V, 22)
    tf_tokens = torch.randint(3, V, (20, T), generator=torch.Generator().manual_seed(20)).to(DEV)
    alone = _decode(b, 0, T, 0, 0, in_tokens=tf_tokens)[0]
    for filt, seed, row_offset in ((fi.FILTERS[0], 2 ** 62 - 1, 0), (fi.FILTERS[2], 77, 2 ** 32 - 5)):
        meta_a = dict(packs=None, mode=1, T=T, start=START, pad=PAD, unk=UNK, seed=seed, row_offset=row_offset, w_p=a["w_p"],
                      b_p=a["b_p"], filter=filt)
        meta_b = dict(packs=None, mode=0, T=T, start=START, in_tokens=tf_tokens)
        with torch.no_grad():
            hs_a, tok_a, hs_b, _ = _AttnLSTMDecoderGroup.apply(
                a["etable"], a["enc"], a["mask"], a["h0"], a["w_c"], a["w_hh"],
                b["etable"], b["enc"], b["mask"], b["h0"], b["w_c"], b["w_hh"], (meta_a, meta_b), None)
        torch.cuda.synchronize()
        what = "pair 7 + 20 filter=%s seed=%d offset=%d" % (filt, seed, row_offset)
        _check_decoder_tokens(hs_a, tok_a, a["w_p"], a["b_p"], seed, row_offset, filt, what)
        torch.testing.assert_close(_teacher_forced(a, tok_a), hs_a, rtol=1e-6, atol=1e-7)
        assert torch.equal(hs_b, alone)  # (the teacher-forced side ignores its neighbour's filter)


# ---- c. the identity filter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", ["0", "1"])
@pytest.mark.parametrize("B,T,S,V", [s for s in fi.DECODER_SHAPES if s[0] >= 17])
def test_identity_filter_in_the_decoders_is_the_unfiltered_entry(B, T, S, V, cluster, monkeypatch):
    """``meta["filter"] = (1, 0, 1)`` reaches the one entry point of the path as a filter record, no filter as a null
    pointer; either way the unfiltered kernels run."""
    from probnmn import _hip

    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    d = _decoder_inputs(B, S, V, 3 * B + V)
    called = []  # (entry point, its filter argument) of every decoder forward call
    lib = _hip.lib()
    for name, at in (("pnmn_attn_lstm_fwd", 2), ("pnmn_attn_lstm_fwd_group", 1)):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name, _at=at: (called.append((_name, a[_at])), _real(*a))[1])
    hs, tok = _decode(d, 1, T, 99, 16)
    assert len(called) == 1 and called[0][1] == 0
    hs_f, tok_f = _decode(d, 1, T, 99, 16, (1.0, 0, 1.0))
    assert len(called) == 2 and called[1][0] == called[0][0] and called[1][1] != 0
    assert torch.equal(tok_f, tok) and torch.equal(hs_f, hs)
    # greedy ignores a filter
    hs_g, tok_g = _decode(d, 2, T, 99, 16)
    hs_gf, tok_gf = _decode(d, 2, T, 99, 16, (0.5, 3, 0.5))
    assert torch.equal(tok_gf, tok_g) and torch.equal(hs_gf, hs_g)


@pytest.mark.parametrize("V", [44, 512])
def test_identity_filter_standalone_is_the_unfiltered_entry(V):
    from probnmn import _hip
    from probnmn.modules.seq2seq_base import choose_tokens

    B = 1000
    logits = fi.standalone_logits(B, V, V).to(DEV)
    tok, lp = choose_tokens(logits, False, 2 ** 62 - 1, 2 ** 32 - 5, 7, PAD, UNK, START)
    out_tok = torch.full((B,), -7, dtype=torch.long, device=DEV)
    out_lp = torch.full((B,), -7.0, device=DEV)
    rec = np.array([(1.0, 0, 1.0, 0)], _hip.SAMPLING_FILTER)
    for greedy in (0, 1):
        rc = _hip.lib().pnmn_sample_tokens(logits.data_ptr(), out_tok.data_ptr(), out_lp.data_ptr(), B, V, greedy,
                                           2 ** 62 - 1, 2 ** 32 - 5, 7, PAD, UNK, START, rec.ctypes.data,
                                           _hip.stream_ptr(torch.device(DEV)))
        assert rc == 0
        want_tok, want_lp = (tok, lp) if not greedy else choose_tokens(logits, True, 0, 0, 0, PAD, UNK, START)
        assert torch.equal(out_tok, want_tok) and torch.equal(out_lp, want_lp)
        rec["temperature"], rec["top_k"] = 0.5, 2  # (the greedy round: a filter it must ignore)


# ---- d. a known distribution ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", ["0", "1"])
def test_filtered_decoder_draws_follow_the_truncated_distribution(cluster, monkeypatch):
    """W_p = 0: every (row, t) draws from softmax(b_p) without pad / unk / start, cut by the filter and renormalised."""
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    B, T, S, V = 1024, 8, 20, 100
    d = _decoder_inputs(B, S, V, 9)
    g = torch.Generator().manual_seed(4)
    b_p = torch.randn(V, generator=g, dtype=torch.float64)
    b_p[65:] += 1.5
    b_p[[PAD, UNK, START]] = 6.0
    d["w_p"], d["b_p"] = torch.zeros(V, H, device=DEV), b_p.float().to(DEV)
    p = torch.softmax(b_p.float().double(), 0)
    p[[PAD, UNK, START]] = 0
    order = torch.argsort(-p)
    for filt in ((1.0, 5, 1.0), (1.0, 0, 0.6)):
        if filt[1]:
            keep = order[:filt[1]]
        else:
            mass = torch.cumsum(p[order], 0) / p.sum()
            keep = order[:int((mass - p[order] / p.sum() < filt[2]).sum())]  # mass before < top_p
        q = torch.zeros_like(p)
        q[keep] = p[keep] / p[keep].sum()
        _, tok2d = _decode(d, 1, T, 2 ** 40 + 3, 0, filt)
        tok = tok2d.cpu().reshape(-1)
        outside = sorted(set(tok.tolist()) - set(keep.tolist()))
        assert not outside, (filt, outside)
        freq = torch.bincount(tok, minlength=V).double() / tok.numel()
        sigma = torch.sqrt(q * (1 - q) / tok.numel())
        worst = int(torch.argmax((freq - q).abs() / (6 * sigma + 1e-5)))
        assert torch.all((freq - q).abs() <= 6 * sigma + 1e-5), (filt, worst, float(freq[worst]), float(q[worst]))


# ---- e. rows that are not all finite ----------------------------------------------------------------------------------
def _nonfinite_rows(V, seed):
    """One NaN; all NaN; +inf; every allowed logit -inf -- each kind in several rows."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for rep in range(8):
        z = torch.randn(V, generator=g) * 3
        z[int(torch.randint(0, V, (1,), generator=g))] = float("nan")
        rows.append(z)
        rows.append(torch.full((V,), float("nan")))
        z = torch.randn(V, generator=g)
        z[torch.randint(0, V, (1 + rep % 3,), generator=g)] = float("inf")
        rows.append(z)
        z = torch.full((V,), float("-inf"))
        z[:3] = torch.randn(min(V, 3), generator=g)
        rows.append(z)
    return torch.stack(rows)


@pytest.mark.parametrize("V", [4, 44, 129])
def test_nonfinite_rows_ignore_the_filter_standalone(V):
    from probnmn.modules.seq2seq_base import choose_tokens

    logits = _nonfinite_rows(V, V).to(DEV)
    for seed, offset, step in ((1, 0, 0), (2 ** 62 - 1, 2 ** 32 - 5, 39)):
        want, want_lp = choose_tokens(logits, False, seed, offset, step, PAD, UNK, START)
        for filt in fi.FILTERS:
            tok, lp = choose_tokens(logits, False, seed, offset, step, PAD, UNK, START, *filt)
            assert int(tok.min()) >= 0 and int(tok.max()) < V
            assert torch.equal(tok, want), filt
            assert torch.equal(torch.nan_to_num(lp, nan=-7.0), torch.nan_to_num(want_lp, nan=-7.0))


@pytest.mark.parametrize("cluster", ["0", "1"])
def test_nonfinite_decoder_rows_stay_in_range_and_to_themselves(cluster, monkeypatch):
    """h0 = NaN in rows {0, 15, 16, B - 1}: every token in range, those rows get what the unfiltered entry gives them, and
    every other row's hidden states and tokens are bit for bit those of a run with those rows finite."""
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    B, T, S, V = 64, 12, 20, 100
    d = _decoder_inputs(B, S, V, 31 + B)
    bad = torch.tensor([0, 15, 16, B - 1], device=DEV)
    h0 = d["h0"].clone()
    h0[bad] = float("nan")
    good = torch.ones(B, dtype=torch.bool, device=DEV)
    good[bad] = False
    _, tok_plain = _decode(d, 1, T, 99, 16, h0=h0)
    for filt in (fi.FILTERS[0], fi.FILTERS[3]):
        hs_ref, tok_ref = _decode(d, 1, T, 99, 16, filt)
        hs, tok = _decode(d, 1, T, 99, 16, filt, h0=h0)
        assert int(tok.min()) >= 0 and int(tok.max()) < V
        assert bool(torch.isnan(hs[bad]).all())
        assert torch.equal(tok[bad], tok_plain[bad])
        assert torch.equal(hs[good], hs_ref[good]) and torch.equal(tok[good], tok_ref[good])


# ---- f. PNMN_EINVAL ---------------------------------------------------------------------------------------------------
_BAD_FILTERS = [(0.0, 0, 1.0), (-1.0, 0, 1.0), (float("inf"), 0, 1.0), (float("nan"), 0, 1.0), (1.0, -1, 1.0),
                (1.0, 0, 0.0), (1.0, 0, -0.5), (1.0, 0, 1.5), (1.0, 0, float("nan"))]


def _sample_tokens(logits, filters, greedy=0):
    """``pnmn_sample_tokens`` into outputs preset to -7: (return code, tokens, logprobs)."""
    from probnmn import _hip

    B, V = logits.shape
    tok = torch.full((B,), -7, dtype=torch.long, device=DEV)
    lp = torch.full((B,), -7.0, device=DEV)
    rc = _hip.lib().pnmn_sample_tokens(logits.data_ptr(), tok.data_ptr(), lp.data_ptr(), B, V, greedy, 5, 3, 2, PAD, UNK, START,
                                       0 if filters is None else filters.ctypes.data, _hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, tok, lp


def _two_jobs(B, T, S, V, modes, seed=5):
    """(job records, sides, workspace or None) of two decoder passes over one set of inputs, pass k in ``modes[k]``."""
    from probnmn import _hip
    from probnmn.modules.seq2seq_base import _decoder_workspace, _prepare_decoder_side

    d = _decoder_inputs(B, S, V, seed)
    tf_tokens = torch.randint(3, V, (B, T), generator=torch.Generator().manual_seed(seed)).to(DEV)
    jobs = np.zeros(2, _hip.DECODER_FWD_JOB)
    sides = []
    for k, mode in enumerate(modes):
        meta = dict(packs=None, mode=mode, T=T, start=START, pad=PAD, unk=UNK, seed=1, row_offset=0, w_p=d["w_p"], b_p=d["b_p"])
        if mode == 0:
            meta = dict(packs=None, mode=0, T=T, start=START, in_tokens=tf_tokens)
        sides.append(_prepare_decoder_side(jobs, k, d["etable"], d["enc"], d["mask"], d["h0"], d["w_c"], d["w_hh"], meta))
    return jobs, sides, _decoder_workspace([B, B], False, torch.device(DEV))


def test_filtered_entry_points_refuse_a_bad_filter_and_launch_nothing():
    from probnmn import _hip

    B, T, S, V = 20, 4, 5, 44
    logits = fi.standalone_logits(B, V, 1).to(DEV)
    jobs, sides, ws = _two_jobs(B, T, S, V, (1, 1))
    greedy = jobs.copy()
    greedy["sample"] = 2
    for bad in _BAD_FILTERS:
        rec = np.array([(*bad, 0), (1.0, 0, 1.0, 0)], _hip.SAMPLING_FILTER)
        rc, tok, lp = _sample_tokens(logits, rec)
        assert rc == _hip.EINVAL, bad
        assert bool((tok == -7).all()) and bool((lp == -7.0).all())
        # the bad filter first; second: checked although the first is fine; and beside a greedy job
        for records, filters in ((jobs, rec), (jobs, rec[::-1].copy()), (greedy, rec)):
            for entry, rc, outputs in fi.decoder_entry_calls(records, sides, ws, filters):
                if filters is rec or entry == "group n=2":
                    assert rc == _hip.EINVAL, (bad, entry)
                    assert all(bool((t == -7).all()) for t in outputs), (bad, entry)


def test_null_options_are_the_identity_options():
    """A null filter is the identity filter and null tables are no automaton: what an entry point returns and writes
    with a null option is, bit for bit, what it does with the identity record (beam: with the automaton that accepts
    every string).  This is what the null filter of the argument tests, once PNMN_EINVAL, now means."""
    from probnmn import _hip
    from probnmn.modules.seq2seq_base import constraint_tables
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    B, T, S, V, END = 20, 4, 5, 44, 3
    vocab = Vocabulary.clevr()
    assert vocab.get_vocab_size("programs") == V and vocab.get_token_index("@end@", namespace="programs") == END
    auto = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs")).decoding_automaton(exclude=(PAD, UNK, START, END))
    tc, ns, ml, _ = constraint_tables(auto, V, END)
    grammar = (END, tc.ctypes.data, ns.ctypes.data, ml.ctypes.data, *ns.shape)
    identity = np.array([(1.0, 0, 1.0, 0)] * 2, _hip.SAMPLING_FILTER)
    # the decoders: one workgroup per tile, and the group entry with one job and with a teacher-forced second one
    for mode in (1, 2):
        jobs, sides, ws = _two_jobs(B, T, S, V, (mode, 0))
        for tail in (fi.NO_TABLES, grammar):
            null = fi.decoder_entry_calls(jobs, sides, ws, None, tail)
            record = fi.decoder_entry_calls(jobs, sides, ws, identity, tail)
            assert [e for e, _, _ in null] == ["fwd"] + (["group n=1", "group n=2"] if ws is not None else [])
            for (entry, rc_n, out_n), (_, rc_r, out_r) in zip(null, record):
                what = (mode, tail is grammar, entry)
                assert rc_n == 0 and rc_r == 0, what
                assert bool((out_n[2] >= 0).all()) and bool((out_n[2] < V).all()), what  # (job 0's tokens were written)
                assert all(torch.equal(a, b) for a, b in zip(out_n, out_r)), what
    # one step's token choice
    for Vs in (44, 512):
        logits = fi.standalone_logits(B, Vs, Vs).to(DEV)
        rc_n, tok_n, lp_n = _sample_tokens(logits, None)
        rc_r, tok_r, lp_r = _sample_tokens(logits, identity)
        assert rc_n == 0 and rc_r == 0 and bool((tok_n >= 0).all())
        assert torch.equal(tok_n, tok_r) and torch.equal(lp_n, lp_r)
    # beam search: null tables against one state, one class, min_left = {0}
    Bq, Sq, beam = 3, 8, 4
    d = _decoder_inputs(Bq, Sq, V, 7)
    one = np.zeros(V, np.uint8), np.zeros((1, 1), np.uint8), np.zeros(1, np.uint8)
    got = []
    for tables in ((0, 0, 0, 0, 0), (one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, 1, 1)):
        tok = torch.full((Bq, beam, T), -7, dtype=torch.long, device=DEV)
        scores = torch.full((Bq, beam), -7.0, device=DEV)
        rc = _hip.lib().pnmn_attn_lstm_beam(d["etable"].data_ptr(), d["enc"].data_ptr(), d["mask"].data_ptr(), d["h0"].data_ptr(),
                                            d["w_c"].data_ptr(), d["w_hh"].data_ptr(), d["w_p"].data_ptr(), d["b_p"].data_ptr(),
                                            tok.data_ptr(), scores.data_ptr(), None, None, None, Bq, T, Sq, V, H, beam, PAD, UNK,
                                            START, END, *tables, _hip.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == 0 and bool((tok >= 0).all())
        got.append((tok, scores))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---- g. Seq2SeqBase and predict_answers -------------------------------------------------------------------------------
def _models():
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(3)
    pg = ProgramGenerator(vocab).to(DEV).eval()
    nmn = NeuralModuleNetwork(vocab).to(DEV).eval()
    batch = {k: v.to(DEV) for k, v in synthetic_batch(vocab, 50, seed=8).items()}
    return vocab, pg, nmn, batch


def test_program_generator_top_k_one_is_the_greedy_decode():
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoderGroup, _prep_tensors

    vocab, pg, _, batch = _models()
    q = batch["question"]
    with torch.no_grad():
        # an untrained generator's arg-max lands on pad / unk / start now and then; with their bias lowered it never does,
        # which is asserted on the data below: top_k = 1 then keeps the greedy token, whatever the uniform
        pg._output_projection_layer.bias[[PAD, UNK, pg._start_index]] -= 10.0
        state = pg.encode(q)
        greedy = pg.decode(state, decoding_strategy="greedy")
        prep = pg._fused_prep(state, None, True, 0, pg._derived())
        _, raw = _AttnLSTMDecoderGroup.apply(*_prep_tensors(prep), [prep["meta"]], None)
        assert not bool(((raw == PAD) | (raw == UNK) | (raw == pg._start_index)).any())
        for seed in (1, 2):
            torch.manual_seed(seed)
            out = pg(q, top_k=1)
            assert torch.equal(out["predictions"], greedy["predictions"])
            torch.testing.assert_close(out["loss"], greedy["loss"], rtol=1e-6, atol=1e-6)
        torch.manual_seed(5)
        assert not torch.equal(pg(q)["predictions"], greedy["predictions"])  # (unfiltered sampling is not the arg-max)
        # teacher forced, evaluation mode: the predictions drawn from the teacher-forced distributions honour the filter
        tf_greedy = pg(q, batch["program"], decoding_strategy="greedy")
        tf_top1 = pg(q, batch["program"], top_k=1)
        assert torch.equal(tf_top1["predictions"], tf_greedy["predictions"])
        torch.testing.assert_close(tf_top1["loss"], tf_greedy["loss"])
    for strategy in ("greedy", "beam"):
        with pytest.raises(ValueError):
            pg(q, decoding_strategy=strategy, top_k=5)
        with pytest.raises(ValueError):
            pg.decode(pg.encode(q), decoding_strategy=strategy, temperature=0.7)


def test_predict_answers_takes_a_filter():
    from probnmn.evaluators import predict_answers

    vocab, pg, nmn, batch = _models()
    records = predict_answers(pg, nmn, [batch], vocab, temperature=0.7, top_p=0.9)
    assert len(records) == 50
    assert all(sorted(r) == ["answer", "question_index"] for r in records)
    plain = predict_answers(pg, nmn, [batch], vocab)
    assert [sorted(r) for r in plain] == [sorted(r) for r in records]
    with pytest.raises(ValueError):
        predict_answers(pg, nmn, [batch], vocab, beam_size=4, top_k=3)
    with pytest.raises(ValueError):
        predict_answers(pg, nmn, [batch], vocab, top_p=0.0)


def test_shapes_outside_the_persistent_kernels_have_no_filtered_path():
    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab, input_size=128, hidden_size=128).to(DEV).eval()
    q = torch.randint(3, 40, (4, 9), device=DEV)
    with torch.no_grad():
        pg(q)  # (the step-by-step path still samples)
        with pytest.raises(NotImplementedError):
            pg(q, top_k=5)
