"""Which token the kernels choose, row by row, against the host reference of tests/token_choice.py: the standalone
``pnmn_sample_tokens`` (through ``choose_tokens``), the draws inside the persistent decoder kernels (one workgroup per
tile, multi-CU, paired launch), the teacher-forced predictions of ``Seq2SeqBase.decode``, and rows that are not all
finite (``-k nonfinite``).

The kernels work in fp32 and the reference in fp64, so a draw whose uniform lies within ``delta`` of a CDF boundary
(or a greedy choice between two logits within ``delta``) may take either neighbour; how many rows do is bounded by
3 x the expected 2 delta V N (+ 5), so that the allowance cannot hide a wrong kernel."""
import os
import sys

import numpy as np
import pytest
import torch

from token_choice import greedy_ref, kernel_uniform, sample_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, UNK, START = 0, 1, 2
H = 256
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_choice_draws.npz")


def _sample_ref(logits64, u, chunk=4096):
    out = [sample_ref(logits64[i:i + chunk], u[i:i + chunk], PAD, UNK, START) for i in range(0, len(u), chunk)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _check_sampled(tok, logits64, u, delta, what):
    """Every token equals the reference draw, or -- within ``delta`` of a CDF boundary -- the draw on the other side."""
    N, V = logits64.shape
    ref, margin = _sample_ref(logits64, u)
    ok = tok == ref
    amb = np.flatnonzero(margin < delta)
    if amb.size:
        lo, _ = _sample_ref(logits64[amb], np.maximum(u[amb] - delta, 0.0))
        hi, _ = _sample_ref(logits64[amb], np.minimum(u[amb] + delta, 1.0 - 2.0 ** -24))
        ok[amb] |= (tok[amb] == lo) | (tok[amb] == hi)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d draws differ from the reference; rows %s got %s want %s (margins %s)" % (
        what, bad.size, N, bad[:8].tolist(), tok[bad[:8]].tolist(), ref[bad[:8]].tolist(), margin[bad[:8]].tolist())
    assert amb.size <= 3 * 2 * delta * V * N + 5, (what, amb.size, N, V)
    return ref


def _check_greedy(tok, logits64, delta, what):
    N, V = logits64.shape
    ref, gap = greedy_ref(logits64)
    ok = tok == ref
    amb = np.flatnonzero(gap < delta)
    if amb.size:
        second = np.argsort(-logits64[amb], 1, kind="stable")[:, 1]
        ok[amb] |= tok[amb] == second
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d greedy tokens differ; rows %s got %s want %s" % (
        what, bad.size, N, bad[:8].tolist(), tok[bad[:8]].tolist(), ref[bad[:8]].tolist())
    assert amb.size <= 3 * 2 * delta * V * N + 5, (what, amb.size, N, V)


# ---- a. the standalone kernel -----------------------------------------------------------------------------------------
# (B, seed, step, row_offset): a row offset of 2**32 - 5 puts the batch across the counter's 32-bit word
_CASES = [(1, 0, 0, 0), (3, 2 ** 32 + 7, 39, 2 ** 32 - 5), (5, 2 ** 62 - 1, 2 ** 31, 0), (1000, 0, 39, 2 ** 32 - 5),
          (40960, 2 ** 62 - 1, 2 ** 31, 2 ** 32 - 5)]


def _standalone_logits(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.1, 1.0, 5.0, 20.0])[torch.arange(B) % 4]  # a different scale and vector in every row
    return torch.randn(B, V, generator=g) * scale[:, None]


@pytest.mark.parametrize("V", [1, 2, 3, 4, 44, 63, 64, 65, 100, 127, 128, 129, 500, 512])
def test_sample_tokens_kernel_draws_the_reference_token(V):
    from probnmn.modules.seq2seq_base import choose_tokens

    for case, (B, seed, step, row_offset) in enumerate(_CASES):
        logits = _standalone_logits(B, V, 100 * V + case)
        tok, lp = choose_tokens(logits.to(DEV), False, seed, row_offset, step, PAD, UNK, START)
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        z64 = logits.double().numpy()
        u = kernel_uniform(seed, row_offset + np.arange(B, dtype=np.uint64), step)
        what = "V=%d B=%d seed=%d step=%d offset=%d" % (V, B, seed, step, row_offset)
        _check_sampled(tok, z64, u, 1e-5, what)
        want_lp = torch.log_softmax(logits.double(), 1).numpy()[np.arange(B), tok]
        np.testing.assert_allclose(lp, want_lp, rtol=1e-5, atol=1e-5, err_msg=what)


@pytest.mark.parametrize("V", [1, 2, 3, 4, 44, 63, 64, 65, 100, 127, 128, 129, 500, 512])
def test_sample_tokens_kernel_greedy_is_argmax(V):
    from probnmn.modules.seq2seq_base import choose_tokens

    B = 5000
    logits = _standalone_logits(B, V, 7 * V)
    g = torch.Generator().manual_seed(V)
    # exact ties: the row's maximum copied to another index (before or after it) in every third row
    rows = torch.arange(0, B, 3)
    logits[rows, torch.randint(0, V, (rows.numel(),), generator=g)] = logits[rows].max(1).values
    tok, lp = choose_tokens(logits.to(DEV), True, 0, 0, 0, PAD, UNK, START)
    assert torch.equal(tok.cpu(), torch.argmax(logits, 1))
    want_lp = torch.log_softmax(logits.double(), 1)[torch.arange(B), tok.cpu()]
    np.testing.assert_allclose(lp.cpu().numpy(), want_lp.numpy(), rtol=1e-5, atol=1e-5)


def test_sample_tokens_kernel_rejects_a_wider_vocabulary():
    from probnmn import _hip

    x = torch.zeros(2, 513, device=DEV)
    tok = torch.full((2,), -7, dtype=torch.long, device=DEV)
    lp = torch.empty(2, device=DEV)
    rc = _hip.lib().pnmn_sample_tokens(x.data_ptr(), tok.data_ptr(), lp.data_ptr(), 2, 513, 0, 0, 0, 0, PAD, UNK, START,
                                       None, _hip.stream_ptr(torch.device(DEV)))
    assert rc == _hip.ESHAPE
    assert tok.cpu().tolist() == [-7, -7]  # nothing launched


# ---- b. draws inside the decoder kernels ------------------------------------------------------------------------------
def _decoder_inputs(B, S, V, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(DEV)  # noqa: E731
    enc, h0 = r(B, S, H), r(B, H)
    lens = torch.randint(1, S + 1, (B,), generator=g).to(DEV)
    mask = (torch.arange(S, device=DEV)[None, :] < lens[:, None]).float()
    return dict(etable=r(V, 4 * H), enc=enc, mask=mask, h0=h0, w_c=r(4 * H, H, scale=0.05), w_hh=r(4 * H, H, scale=0.05),
                w_p=r(V, H, scale=0.3), b_p=r(V))


def _decode(d, mode, T, seed, row_offset, h0=None):
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoder

    with torch.no_grad():
        hs, tok = _AttnLSTMDecoder.apply(None, d["etable"], d["enc"], d["mask"], d["h0"] if h0 is None else h0, d["w_c"],
                                         d["w_hh"], d["w_p"], d["b_p"], mode, T, seed, row_offset, PAD, UNK, START)
    torch.cuda.synchronize()
    return hs, tok


def _teacher_forced(d, tok):
    """The decoder re-run teacher forced on [start; tok[:, :-1]]: the hidden states of the free-running pass if every
    token it wrote is the token it fed to its next step."""
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoder

    B, T = tok.shape
    inp = torch.cat((tok.new_full((B, 1), START), tok[:, :-1]), 1)
    with torch.no_grad():
        hs, _ = _AttnLSTMDecoder.apply(None, d["etable"], d["enc"], d["mask"], d["h0"], d["w_c"], d["w_hh"], None, None, 0, T,
                                       0, 0, PAD, UNK, START, None, inp)
    torch.cuda.synchronize()
    return hs


def _check_decoder_tokens(hs, tok, w_p, b_p, mode, seed, row_offset, what):
    """Every (row, t) on its own: logits from the kernel's own h_t in fp64, counter (seed, row_offset + row, t)."""
    B, T, _ = hs.shape
    assert tok.shape == (B, T)
    logits = (hs.double() @ w_p.double().t() + b_p.double()).cpu().numpy().reshape(B * T, -1)
    tok = tok.cpu().numpy().reshape(-1)
    if mode == 1:
        rows = row_offset + np.arange(B, dtype=np.uint64)[:, None]
        u = kernel_uniform(seed, rows, np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
        _check_sampled(tok, logits, u, 1e-4, what)
    else:
        _check_greedy(tok, logits, 1e-4, what)


_DECODER_SHAPES = [(1, 1, 1, 44), (7, 5, 3, 44), (17, 12, 20, 100), (64, 12, 20, 128), (128, 27, 46, 44), (530, 9, 27, 100),
                   (1024, 40, 64, 44)]  # (B, T, S, V); the last = the 40 steps of config 5


@pytest.mark.parametrize("cluster", ["0", "1"])
@pytest.mark.parametrize("B,T,S,V", _DECODER_SHAPES)
def test_decoder_draws_the_reference_token(B, T, S, V, cluster, monkeypatch):
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    d = _decoder_inputs(B, S, V, B + T + S + V)
    for mode, seed, row_offset in ((1, 2 ** 62 - 1, 0), (1, 2 ** 32 + 7, 16), (1, 12345, 2 ** 32 - 5), (2, 3, 0)):
        what = "cluster=%s B=%d T=%d S=%d V=%d mode=%d seed=%d offset=%d" % (cluster, B, T, S, V, mode, seed, row_offset)
        hs, tok = _decode(d, mode, T, seed, row_offset)
        _check_decoder_tokens(hs, tok, d["w_p"], d["b_p"], mode, seed, row_offset, what)
        torch.testing.assert_close(_teacher_forced(d, tok), hs, rtol=1e-6, atol=1e-7, msg=lambda m: "%s: %s" % (what, m))


@pytest.mark.parametrize("rows_s,rows_t", [(7, 20), (130, 64), (530, 100)])
def test_paired_decoder_draws_the_reference_token(rows_s, rows_t):
    """The paired launch (a sampling side beside a teacher-forced one) draws what the reference draws from its own
    hidden states."""
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoderGroup

    T, S, V = 26, 30, 44
    a, b = _decoder_inputs(rows_s, S, V, 1 + rows_s), _decoder_inputs(rows_t, S, V, 2 + rows_t)
    tf_tokens = torch.randint(3, V, (rows_t, T), generator=torch.Generator().manual_seed(rows_t)).to(DEV)
    for seed, row_offset in ((2 ** 62 - 1, 0), (77, 2 ** 32 - 5)):
        meta_a = dict(packs=None, mode=1, T=T, start=START, pad=PAD, unk=UNK, seed=seed, row_offset=row_offset, w_p=a["w_p"],
                      b_p=a["b_p"])
        meta_b = dict(packs=None, mode=0, T=T, start=START, in_tokens=tf_tokens)
        with torch.no_grad():
            hs_a, tok_a, hs_b, _ = _AttnLSTMDecoderGroup.apply(
                a["etable"], a["enc"], a["mask"], a["h0"], a["w_c"], a["w_hh"],
                b["etable"], b["enc"], b["mask"], b["h0"], b["w_c"], b["w_hh"], (meta_a, meta_b), None)
        torch.cuda.synchronize()
        what = "pair rows %d + %d seed=%d offset=%d" % (rows_s, rows_t, seed, row_offset)
        _check_decoder_tokens(hs_a, tok_a, a["w_p"], a["b_p"], 1, seed, row_offset, what)
        torch.testing.assert_close(_teacher_forced(a, tok_a), hs_a, rtol=1e-6, atol=1e-7)


# ---- c. the decoder's draws against a known distribution, without the host reference ---------------------------------
@pytest.mark.parametrize("cluster", ["0", "1"])
def test_decoder_draws_follow_a_known_distribution(cluster, monkeypatch):
    """W_p = 0: every (row, t) draws from softmax(b_p) without pad / unk / start.  Those three carry the largest logits
    and most of the allowed mass lies above index 64."""
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    B, T, S, V = 1024, 40, 20, 100
    d = _decoder_inputs(B, S, V, 9)
    g = torch.Generator().manual_seed(4)
    b_p = torch.randn(V, generator=g, dtype=torch.float64)
    b_p[65:] += 1.5
    b_p[[PAD, UNK, START]] = 6.0
    d["w_p"], d["b_p"] = torch.zeros(V, H, device=DEV), b_p.float().to(DEV)
    seed = 2 ** 40 + 3
    _, tok2d = _decode(d, 1, T, seed, 0)
    # the logits are exactly b_p, so every step's draws are the standalone kernel's at the same (seed, row, step)
    from probnmn.modules.seq2seq_base import choose_tokens

    for t in range(T):
        want, _ = choose_tokens(d["b_p"].expand(B, V), False, seed, 0, t, PAD, UNK, START)
        assert torch.equal(tok2d[:, t], want), t
    tok = tok2d.cpu().reshape(-1)
    assert int(tok.min()) >= 3 and int(tok.max()) < V
    p = torch.softmax(b_p.float().double(), 0)
    p[[PAD, UNK, START]] = 0
    p = p / p.sum()
    assert float(p[64:].sum()) > 0.5
    freq = torch.bincount(tok, minlength=V).double() / tok.numel()
    sigma = torch.sqrt(p * (1 - p) / tok.numel())
    worst = int(torch.argmax((freq - p).abs() / (6 * sigma + 1e-5)))
    assert torch.all((freq - p).abs() <= 6 * sigma + 1e-5), (worst, float(freq[worst]), float(p[worst]))
    # greedy with an exact tie for the largest logit: always the lower index
    tied = b_p.float().clone()
    tied[70] = tied[90] = 9.0
    d["b_p"] = tied.to(DEV)
    _, tok = _decode(d, 2, T, 0, 0)
    assert bool((tok == 70).all())


# ---- d. teacher-forced predictions of Seq2SeqBase.decode --------------------------------------------------------------
@pytest.mark.parametrize("which", ["pg", "qr"])
@pytest.mark.parametrize("offset", [0, 16, 2 ** 32 - 5])
def test_teacher_forced_predictions_draw_the_reference_token(which, offset, monkeypatch):
    """Predictions drawn from the teacher-forced distributions (reference seq2seq_base.py:196-220): step t of row b is
    drawn at counter row (sample_row_offset + b) * steps + t, step 0, then trimmed after the first @end@."""
    from oracle.seq2seq_oracle import trim_predictions
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator, QuestionReconstructor
    from probnmn.modules import seq2seq_base
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(3)
    model = (ProgramGenerator if which == "pg" else QuestionReconstructor)(vocab).to(DEV).eval()
    model.sample_row_offset = offset
    batch = synthetic_batch(vocab, 50, seed=8, with_image=False)
    src, tgt = (batch["question"], batch["program"]) if which == "pg" else (batch["program"], batch["question"])
    seen = []
    real = seq2seq_base.choose_tokens

    def capture(logits, *args):
        out = real(logits, *args)
        seen.append((logits.detach().clone(), out[0].clone()))
        return out

    monkeypatch.setattr(seq2seq_base, "choose_tokens", capture)
    for strategy, seed in (("sampling", 2 ** 62 - 1), ("sampling", 5), ("greedy", 0)):
        seen.clear()
        with torch.no_grad():
            out = model.decode(model.encode(src.to(DEV)), tgt.to(DEV), strategy, seed=seed)
        assert len(seen) == 1
        logits, raw = seen[0]
        B = src.size(0)
        steps = logits.size(0) // B
        z64, tok = logits.double().cpu().numpy(), raw.cpu().numpy()
        what = "%s offset=%d %s seed=%d" % (which, offset, strategy, seed)
        if strategy == "sampling":
            rows = (offset + np.arange(B, dtype=np.uint64)[:, None]) * steps + np.arange(steps, dtype=np.uint64)[None, :]
            _check_sampled(tok, z64, kernel_uniform(seed, rows.reshape(-1), 0), 1e-5, what)
        else:
            assert np.array_equal(tok, torch.argmax(logits.cpu(), 1).numpy()), what
        want = trim_predictions(raw.cpu().view(B, steps), model._end_index)
        assert torch.equal(out["predictions"].cpu(), want), what


# ---- e. rows that are not all finite ----------------------------------------------------------------------------------
def _nonfinite_rows(V, seed):
    """One NaN; all NaN; +inf; every allowed logit -inf; allowed weights that underflow (excluded at +100, allowed
    about -10) -- each kind in several rows."""
    g = torch.Generator().manual_seed(seed)
    kinds, rows = [], []
    for rep in range(8):
        z = torch.randn(V, generator=g) * 3
        z[int(torch.randint(0, V, (1,), generator=g))] = float("nan")
        rows.append(z), kinds.append("one NaN")
        rows.append(torch.full((V,), float("nan"))), kinds.append("all NaN")
        z = torch.randn(V, generator=g)
        z[torch.randint(0, V, (1 + rep % 3,), generator=g)] = float("inf")
        rows.append(z), kinds.append("+inf")
        z = torch.full((V,), float("-inf"))
        z[:3] = torch.randn(min(V, 3), generator=g)
        rows.append(z), kinds.append("allowed -inf")
        z = -10 + torch.randn(V, generator=g)
        z[:3] = 100.0
        rows.append(z), kinds.append("underflow")
    return torch.stack(rows), kinds


@pytest.mark.parametrize("V", [1, 3, 4, 44, 63, 64, 65, 100, 129, 512])
def test_nonfinite_rows_standalone_kernel(V):
    from probnmn.modules.seq2seq_base import choose_tokens

    logits, kinds = _nonfinite_rows(V, V)
    B = logits.size(0)
    z64 = logits.double().numpy()
    want_lp_all = torch.log_softmax(logits.double(), 1).numpy()
    for seed, offset, step in ((1, 0, 0), (2 ** 62 - 1, 2 ** 32 - 5, 39)):
        tok, lp = choose_tokens(logits.to(DEV), False, seed, offset, step, PAD, UNK, START)
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        assert tok.min() >= 0 and tok.max() < V, tok
        u = kernel_uniform(seed, offset + np.arange(B, dtype=np.uint64), step)
        _check_sampled(tok, z64, u, 1e-5, "V=%d nonfinite rows (%s)" % (V, ", ".join(sorted(set(kinds)))))
        np.testing.assert_allclose(lp, want_lp_all[np.arange(B), tok], rtol=1e-5, atol=1e-5)  # (NaN where the row has one)
        under = np.array([k == "underflow" for k in kinds])
        if V > 3:  # the underflow rows were drawn, not arg-maxed: more than one token among them
            assert len(set(tok[under].tolist())) > 1 or V == 4
        gt, glp = choose_tokens(logits.to(DEV), True, seed, offset, step, PAD, UNK, START)
        assert torch.equal(gt.cpu(), torch.argmax(logits, 1))
        np.testing.assert_allclose(glp.cpu().numpy(), want_lp_all[np.arange(B), gt.cpu().numpy()], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("cluster", ["0", "1"])
@pytest.mark.parametrize("B,T,S,V", [(64, 12, 20, 100), (530, 9, 27, 44)])
def test_nonfinite_decoder_rows_stay_in_range_and_to_themselves(B, T, S, V, cluster, monkeypatch):
    """h0 = NaN in rows {0, 15, 16, B - 1} (across a 16-row tile): every token in range, those rows follow the rule
    (sampling: the first allowed index; greedy: index 0 -- every logit is NaN), and every other row's hidden states and
    tokens are bit for bit those of a run with those rows finite."""
    monkeypatch.setenv("PNMN_DECODER_CLUSTER", cluster)
    d = _decoder_inputs(B, S, V, 31 + B)
    bad = torch.tensor([0, 15, 16, B - 1], device=DEV)
    h0 = d["h0"].clone()
    h0[bad] = float("nan")
    good = torch.ones(B, dtype=torch.bool, device=DEV)
    good[bad] = False
    for mode, first in ((1, 3), (2, 0)):
        hs_ref, tok_ref = _decode(d, mode, T, 99, 16)
        hs, tok = _decode(d, mode, T, 99, 16, h0=h0)
        assert int(tok.min()) >= 0 and int(tok.max()) < V
        assert bool(torch.isnan(hs[bad]).all())
        assert bool((tok[bad] == first).all()), tok[bad]
        assert torch.equal(hs[good], hs_ref[good]) and torch.equal(tok[good], tok_ref[good])


# ---- f. the draws of finite rows do not change ------------------------------------------------------------------------
def _recorded_draws():
    """Tokens the sampling paths draw from fixed inputs: the decoder kernels (both families, modes 1 and 2, shapes of the
    training batches), the paired launch and the standalone kernel.  tests/golden/token_choice_draws.npz holds them as
    drawn by the library before non-finite rows had a rule of their own; ``python tests/test_token_choice_gpu.py record``
    rewrites it, for a change that is meant to change the draws."""
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoderGroup, choose_tokens

    out = {}
    saved = os.environ.get("PNMN_DECODER_CLUSTER")
    try:
        for cluster in ("0", "1"):
            os.environ["PNMN_DECODER_CLUSTER"] = cluster
            for B, T, S, V in ((64, 12, 20, 128), (530, 9, 27, 100), (1024, 26, 46, 44)):
                d = _decoder_inputs(B, S, V, 7 * B + T)
                for mode in (1, 2):
                    _, tok = _decode(d, mode, T, 2 ** 40 + B, 16)
                    out["decoder_c%s_%d_%d_%d_%d_m%d" % (cluster, B, T, S, V, mode)] = tok.cpu().numpy().astype(np.uint8)
    finally:
        if saved is None:
            os.environ.pop("PNMN_DECODER_CLUSTER", None)
        else:
            os.environ["PNMN_DECODER_CLUSTER"] = saved
    a, b = _decoder_inputs(300, 30, 44, 1), _decoder_inputs(200, 30, 44, 2)
    tf = torch.randint(3, 44, (200, 26), generator=torch.Generator().manual_seed(0)).to(DEV)
    meta_a = dict(packs=None, mode=1, T=26, start=START, pad=PAD, unk=UNK, seed=99, row_offset=5, w_p=a["w_p"], b_p=a["b_p"])
    meta_b = dict(packs=None, mode=0, T=26, start=START, in_tokens=tf)
    with torch.no_grad():
        _, tok_a, _, _ = _AttnLSTMDecoderGroup.apply(a["etable"], a["enc"], a["mask"], a["h0"], a["w_c"], a["w_hh"],
                                                     b["etable"], b["enc"], b["mask"], b["h0"], b["w_c"], b["w_hh"], (meta_a, meta_b), None)
    out["pair"] = tok_a.cpu().numpy().astype(np.uint8)
    for V in (44, 100, 512):
        logits = _standalone_logits(8192, V, 5 + V)
        for greedy in (False, True):
            tok, _ = choose_tokens(logits.to(DEV), greedy, 2 ** 62 - 1, 2 ** 32 - 5, 7, PAD, UNK, START)
            out["standalone_%d_%s" % (V, "greedy" if greedy else "sample")] = tok.cpu().numpy().astype(np.uint16)
    torch.cuda.synchronize()
    return out


def test_draws_of_finite_rows_match_the_recorded_tokens():
    """The rule for rows that are not all finite sits behind a branch finite rows never take: their draws are bit for bit
    those recorded from the library before that rule existed."""
    want = np.load(RECORDED)
    got = _recorded_draws()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        n = int((got[k] != want[k]).sum())
        assert got[k].shape == want[k].shape and n == 0, (k, n, want[k].size)


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "probnmn-clevr_amd"))
    draws = _recorded_draws()
    np.savez_compressed(sys.argv[2] if len(sys.argv) > 2 else RECORDED, **draws)
    print("recorded %d arrays, %d tokens" % (len(draws), sum(v.size for v in draws.values())))
