"""Rows grouped by length in the multi-CU attention decoders (pnmn_decoder_last, pnmn_attn_lstm_fwd_group_ordered /
_bwd_group_ordered): the ordered calls against the calls without an order of the same kernel variant -- bit for bit at every
step a row has, zeros from its tile's last step on in every buffer a later call reads over all T, every output pre-filled with
NaN so that an element that must be defined and is not shows -- the identity order, a pass cut into two row ranges, the
argument checks, and one 260-question seq2seq plan with the switch on against off.

Shapes: hidden 256 (fixed by the kernels), V = 20, S = 5, T = 9; B = 40 is two full tiles and one of 8 rows."""
import functools

import numpy as np
import pytest
import torch

from probnmn import _hip
from probnmn.modules.seq2seq_base import pack_fragments
from test_gemm_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, V, S, T = 256, 20, 5, 9
FWD_OUT = ("hs", "cs", "act", "ctx", "probs")
FWD_ZERO = ("hs", "ctx")                           # what later calls read over all T: zero filled by the forward ...
BWD_OUT = ("dgates", "dctx", "dscore", "weights", "dh0")
BWD_ZERO = ("dgates", "dctx", "dscore", "weights")  # ... and by the backward


def _stream():
    return _hip.stream_ptr(torch.device(DEV))


def _ragged_steps():
    """40 rows: lengths 1 and T, runs of equal lengths, and ten rows of length 1 -- longest first, the last tile (8 rows) then
    holds rows of one step only."""
    rng = np.random.Generator(np.random.Philox(5))
    steps = rng.integers(2, T + 1, 40)
    steps[[1, 4, 7, 12, 18, 22, 23, 30, 33, 39]] = 1
    steps[[0, 21, 38]] = T
    steps[8:12] = 4
    steps[24:28] = 6
    return steps


def _problem(B, Tn, steps, seed):
    """Inputs of one teacher-forced pass and of its backward (dhs zero from every row's own steps on: the contract)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *shape, scale=1.0: torch.randn(*shape, device=DEV, generator=g) * scale  # noqa: E731
    w_c, w_hh = r(4 * H, H, scale=0.05), r(4 * H, H, scale=0.05)
    mask = torch.ones(B, S, device=DEV)
    mask[torch.arange(B, device=DEV) % 3 == 0, S - 2:] = 0.0
    in_tokens = torch.randint(0, V, (B, Tn), device=DEV, generator=g)
    etable = r(V, 4 * H, scale=0.5)
    steps_d = torch.as_tensor(np.asarray(steps), device=DEV)
    valid = torch.arange(Tn, device=DEV)[None, :] < steps_d[:, None]
    return dict(B=B, T=Tn, steps=steps_d, valid=valid, enc=r(B, S, H, scale=0.5), mask=mask, h0=r(B, H, scale=0.5), etable=etable,
                in_tokens=in_tokens, xe=etable[in_tokens].contiguous(), w_c=pack_fragments(w_c), w_hh=pack_fragments(w_hh),
                w_c_t=pack_fragments(w_c.t()), w_hh_t=pack_fragments(w_hh.t()), dhs=r(B, Tn, H) * valid[:, :, None])


def _order_of(steps_d, Tn):
    """pnmn_length_order's lists for rows of ``steps_d`` steps."""
    B = steps_d.numel()
    last = (steps_d - 1).to(torch.int32)
    order = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tile_steps = torch.full(((B + 15) // 16,), -1, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pnmn_length_order(last.data_ptr(), B, Tn, order.data_ptr(), tile_steps.data_ptr(), _stream()), "length_order")
    return order, tile_steps


def _lists(order, tile_steps):
    arr = np.array([[order.data_ptr()], [tile_steps.data_ptr()]], np.uint64)
    return arr, (arr[0].ctypes.data, arr[1].ctypes.data)


def _workspace(B, backward):
    n = _hip.decoder_workspace_bytes([B], backward)
    assert n > 0  # (the multi-CU kernels do take this pass)
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _forward(p, form, lists=None, entry="plain"):
    """One pass forward; ``form``: the step inputs as token-table rows ("tokens") or projected ("xe").  Outputs NaN pre-filled."""
    B, Tn = p["B"], p["T"]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out = dict(hs=nan(B, Tn, H), cs=nan(B, Tn, H), act=nan(B, Tn, 4 * H), ctx=nan(B, Tn, H), probs=nan(B, Tn, S))
    job = np.zeros(1, _hip.DECODER_FWD_JOB)
    j = job[0]
    for k in ("enc", "mask", "h0", "w_c", "w_hh"):
        j[k] = p[k].data_ptr()
    for k in FWD_OUT:
        j[k] = out[k].data_ptr()
    if form == "xe":
        j["xe"] = p["xe"].data_ptr()
    else:
        j["etable"], j["in_tokens"], j["in_token_stride"] = p["etable"].data_ptr(), p["in_tokens"].data_ptr(), p["in_tokens"].stride(0)
    j["B"], j["T"], j["S"] = B, Tn, S
    ws, lib = _workspace(B, False), _hip.lib()
    if entry == "plain":
        rc = lib.pnmn_attn_lstm_fwd_group(job.ctypes.data, None, 0, None, None, None, 0, 0, 1, H, ws.data_ptr(), _stream())
    else:
        keep, ptrs = _lists(*lists) if lists is not None else (None, (None, None))
        rc = lib.pnmn_attn_lstm_fwd_group_ordered(job.ctypes.data, None, 0, None, None, None, 0, 0, 1, H, *ptrs, ws.data_ptr(), _stream())
    _hip.check(rc, "attn_lstm_fwd_group")
    torch.cuda.synchronize()
    return out


def _backward(p, fwd, lists=None, entry="plain"):
    B, Tn = p["B"], p["T"]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out = dict(dgates=nan(B, Tn, 4 * H), dctx=nan(B, Tn, H), dscore=nan(B, Tn, S), weights=nan(B, Tn, S), dh0=nan(B, H))
    job = np.zeros(1, _hip.DECODER_BWD_JOB)
    j = job[0]
    for k in ("dhs", "enc", "mask", "h0", "w_c_t", "w_hh_t"):
        j[k] = p[k].data_ptr()
    for k in ("act", "cs", "hs", "probs"):
        j[k] = fwd[k].data_ptr()
    for k in BWD_OUT:
        j[k] = out[k].data_ptr()
    j["B"], j["T"], j["S"] = B, Tn, S
    ws, lib = _workspace(B, True), _hip.lib()
    if entry == "plain":
        rc = lib.pnmn_attn_lstm_bwd_group(job.ctypes.data, 1, H, ws.data_ptr(), _stream())
    else:
        keep, ptrs = _lists(*lists) if lists is not None else (None, (None, None))
        rc = lib.pnmn_attn_lstm_bwd_group_ordered(job.ctypes.data, 1, H, *ptrs, ws.data_ptr(), _stream())
    _hip.check(rc, "attn_lstm_bwd_group")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _ragged(form):
    """The ragged batch through both calls, forward and backward: computed once per input form, shared by the tests."""
    p = _problem(40, T, _ragged_steps(), seed=3)
    order, tile_steps = _order_of(p["steps"], T)
    plain_f = _forward(p, form)
    plain_b = _backward(p, plain_f)
    ord_f = _forward(p, form, (order, tile_steps), "ordered")
    ord_b = _backward(p, ord_f, (order, tile_steps), "ordered")  # (reads the ordered forward's cs / act / probs: NaN where unwritten)
    slot = torch.empty(40, dtype=torch.long, device=DEV)
    slot[order.long()] = torch.arange(40, device=DEV)
    row_tile_steps = tile_steps.long()[slot // 16]  # steps of the tile every row sits in
    return p, order, tile_steps, row_tile_steps, plain_f, plain_b, ord_f, ord_b


def test_order_is_the_stable_sort_and_the_last_tile_has_one_step():
    p, order, tile_steps, row_tile_steps, *_ = _ragged("tokens")
    steps = p["steps"].cpu().numpy()
    assert np.array_equal(order.cpu().numpy(), np.argsort(-steps, kind="stable"))
    assert tile_steps.tolist() == [T, int(np.sort(steps)[::-1][16]), 1]
    assert bool((row_tile_steps >= p["steps"]).all())


@pytest.mark.parametrize("form", ["tokens", "xe"])
def test_forward_ragged(form):
    p, _, _, row_ts, plain, _, got, _ = _ragged(form)
    t = torch.arange(T, device=DEV)[None, :]
    ran, valid = t < row_ts[:, None], p["valid"]
    assert bool((~ran).any()) and bool((ran & ~valid).any())
    for k in FWD_OUT:
        assert not bool(torch.isnan(plain[k]).any()), k
        assert torch.equal(got[k][valid], plain[k][valid]), k   # bit for bit at every step a row has
        assert torch.equal(got[k][ran], plain[k][ran]), k       # (and at every step its tile ran)
    for k in FWD_ZERO:
        assert not bool(torch.isnan(got[k]).any()), k
        assert float(got[k][~ran].abs().max()) == 0.0, k


@pytest.mark.parametrize("form", ["tokens", "xe"])
def test_backward_ragged(form):
    p, _, _, row_ts, _, plain, _, got = _ragged(form)
    t = torch.arange(T, device=DEV)[None, :]
    ran, valid = t < row_ts[:, None], p["valid"]
    for k in BWD_OUT:
        assert not bool(torch.isnan(plain[k]).any()), k
        assert not bool(torch.isnan(got[k]).any()), k
    assert torch.equal(got["dh0"], plain["dh0"])
    for k in BWD_ZERO:
        assert torch.equal(got[k][valid], plain[k][valid]), k
        assert float(got[k][~ran].abs().max()) == 0.0, k
    for k in ("dgates", "dctx", "dscore"):  # (zero from the row's own steps on in either call: dhs is zero there)
        assert float(got[k][~valid].abs().max()) == 0.0 and float(plain[k][~valid].abs().max()) == 0.0, k


@pytest.mark.parametrize("form", ["tokens", "xe"])
def test_identity_order_gives_the_bits_of_the_call_without_one(form):
    p = _ragged(form)[0]
    plain_f, plain_b = _ragged(form)[4], _ragged(form)[5]
    ident = (torch.arange(40, dtype=torch.int32, device=DEV), torch.full((3,), T, dtype=torch.int32, device=DEV))
    got_f = _forward(p, form, ident, "ordered")
    got_b = _backward(p, got_f, ident, "ordered")
    null_f = _forward(p, form, None, "ordered")  # (null lists through the new entry points: the call as it was)
    for k in FWD_OUT:
        assert torch.equal(got_f[k], plain_f[k]) and torch.equal(null_f[k], plain_f[k]), k
    for k in BWD_OUT:
        assert torch.equal(got_b[k], plain_b[k]), k


def test_row_ranges_take_their_part_of_the_lists():
    """B = 520 runs as two launches (512 rows + 8).  By hand: each range as an ordered call of its own over the range's rows
    gathered into a pass of their own (identity order there, the range's part of tile_steps) -- a row's bits depend neither on
    its slot nor on its neighbours, so the results are equal wherever the range's hand-over (order + r0, tile_steps + r0 / 16,
    the pass's own base pointers) is right."""
    B, Tn = 520, 4
    rng = np.random.Generator(np.random.Philox(8))
    p = _problem(B, Tn, rng.integers(1, Tn + 1, B), seed=6)
    order, tile_steps = _order_of(p["steps"], Tn)
    got_f = _forward(p, "tokens", (order, tile_steps), "ordered")
    got_b = _backward(p, got_f, (order, tile_steps), "ordered")
    for r0, r1 in ((0, 512), (512, 520)):
        rows = order[r0:r1].long()
        q = dict(p, B=r1 - r0)
        for k in ("enc", "mask", "h0", "in_tokens", "xe", "dhs", "steps", "valid"):
            q[k] = p[k][rows].contiguous()
        part = (torch.arange(r1 - r0, dtype=torch.int32, device=DEV), tile_steps[r0 // 16:(r1 + 15) // 16].contiguous())
        want_f = _forward(q, "tokens", part, "ordered")
        want_b = _backward(q, want_f, part, "ordered")
        ran = torch.arange(Tn, device=DEV)[None, :] < part[1].long().repeat_interleave(16)[:r1 - r0, None]
        for k in FWD_OUT:
            assert torch.equal(got_f[k][rows][ran], want_f[k][ran]), (k, r0)
        for k in FWD_ZERO:
            assert torch.equal(got_f[k][rows], want_f[k]), (k, r0)
        for k in BWD_OUT:
            assert torch.equal(got_b[k][rows], want_b[k]), (k, r0)
    for k in FWD_ZERO:
        assert not bool(torch.isnan(got_f[k]).any()), k


def test_rejected_jobs():
    lib, einval = _hip.lib(), _hip.CONSTANTS["PNMN_EINVAL"]
    p = _ragged("tokens")[0]
    order, tile_steps = _ragged("tokens")[1:3]
    keep, ptrs = _lists(order, tile_steps)
    ws = _workspace(40, True)
    job = np.zeros(1, _hip.DECODER_FWD_JOB)
    job[0]["B"], job[0]["T"], job[0]["S"], job[0]["V"] = 40, T, S, V

    def fwd(order_p, steps_p, hidden=H):
        return lib.pnmn_attn_lstm_fwd_group_ordered(job.ctypes.data, None, 0, None, None, None, 0, 0, 1, hidden, order_p, steps_p,
                                                    ws.data_ptr(), _stream())
    for sample in (1, 2):  # a sampling and a greedy job with an order
        job[0]["sample"] = sample
        assert fwd(*ptrs) == einval
    job[0]["sample"] = 0
    assert fwd(ptrs[0], None) == einval and fwd(None, ptrs[1]) == einval  # one list without the other
    half = np.array([[order.data_ptr()], [0]], np.uint64)
    assert fwd(half[0].ctypes.data, half[1].ctypes.data) == einval
    assert fwd(*ptrs, hidden=128) == einval
    job[0]["S"] = 65
    assert fwd(*ptrs) == einval
    bjob = np.zeros(1, _hip.DECODER_BWD_JOB)
    bjob[0]["B"], bjob[0]["T"], bjob[0]["S"] = 40, T, 65
    assert lib.pnmn_attn_lstm_bwd_group_ordered(bjob.ctypes.data, 1, H, *ptrs, ws.data_ptr(), _stream()) == einval
    bjob[0]["S"] = S
    assert lib.pnmn_attn_lstm_bwd_group_ordered(bjob.ctypes.data, 1, H, ptrs[0], None, ws.data_ptr(), _stream()) == einval
    assert p["B"] == 40


def test_decoder_last_counts_the_steps_the_loss_weights():
    pad = 0
    tokens = torch.randint(1, V, (70, T + 2), device=DEV)
    tokens[0, :] = pad                   # no weighted step: one step all the same
    tokens[1, 4:] = pad
    tokens[2, 3] = pad                   # a pad inside drops no later step
    tokens[3, T:] = pad
    last = torch.full((70,), -7, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pnmn_decoder_last(tokens.data_ptr() + 8, tokens.stride(0), pad, 70, T, last.data_ptr(), _stream()), "decoder_last")
    w = tokens[:, 1:T + 1] != pad
    steps = (w * torch.arange(1, T + 1, device=DEV)[None, :]).amax(1)
    assert torch.equal(last.long(), steps.clamp(min=1) - 1)


N_NOSUP, N_SUP, TQ, TP = 130, 130, 20, 12  # 260 questions: the reconstructor's pass is above the 256-row threshold


def _plan(monkeypatch, switch):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.runtime.seq_plan import Seq2SeqPlan
    from probnmn.vocabulary import Vocabulary

    dev = torch.device(DEV)
    vocab = Vocabulary.clevr()
    torch.manual_seed(1)
    models = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256)]
    for m in models:
        m.to(dev)
    models[2].eval()
    B = N_NOSUP + N_SUP
    batch = synthetic_batch(vocab, B, seed=4, with_image=False)
    question, program = batch["question"][:, :TQ].contiguous().to(dev), batch["program"][:, :TP].contiguous().to(dev)
    monkeypatch.setenv("PNMN_DECODER_LENGTH_ORDER", switch)
    plan = Seq2SeqPlan(*models, dev, N_NOSUP, N_SUP, TQ, TP)
    names = [name for calls in (plan.fwd_pg, plan.fwd_qr, plan.bwd_a) for _, _, name in calls]
    ordered = [n for n in names if n.endswith("_group_ordered")]
    assert (sorted(ordered) == ["pnmn_attn_lstm_bwd_group_ordered", "pnmn_attn_lstm_fwd_group_ordered"]) if switch == "1" else not ordered
    assert ("pnmn_decoder_last" in names) == (switch == "1")
    # (a fresh plan's buffers are whatever the allocator held: make an element of the reconstructor's decoder that a later
    # call reads and nobody wrote show)
    for name in ["qr.d." + k for k in ("hs", "cs", "cx", "act", "dg", "dctx")] + ["qr.q." + k for k in ("probs", "dscore", "weights")]:
        plan[name].fill_(float("nan"))
    torch.manual_seed(9)
    plan.run_encoder(question, program, torch.arange(N_NOSUP, device=dev), torch.arange(N_NOSUP, B, device=dev))
    plan.run_decoders()
    plan.run_generator_finish()
    plan.run_reconstructor()
    plan.run_prior()
    g = torch.Generator(device=dev).manual_seed(2)
    plan.backward(*(torch.randn(r, device=dev, generator=g) for r in (N_NOSUP, N_SUP, B)))
    torch.cuda.synchronize()
    return plan


def test_plan_with_the_switch_on_against_off(monkeypatch):
    on, off = _plan(monkeypatch, "1"), _plan(monkeypatch, "0")
    assert torch.equal(on.out["z"], off.out["z"])
    for key in ("loss_s", "loss_t", "loss_q", "loss_p"):
        assert bool(torch.isfinite(on.out[key]).all()) and torch.equal(on.out[key], off.out[key]), key  # per-row losses: bit-equal
    K = (N_NOSUP + N_SUP) * max(on.e_pg["T"], on.e_qr["T"], on.D)  # (the bar of tests/test_seq_plan_pairs_gpu.py)
    for mm, ref in ((on.pg, off.pg), (on.qr, off.qr)):
        for got, want in zip(mm.grads, ref.grads):
            assert bool(torch.isfinite(got).all())
            if float(want.abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0
            else:
                _close(got, want.double(), K)
