"""pnmn_lstm_stack_fwd / _bwd (csrc/lstm_stack.hip): the two layers of an encoder as a wavefront in one launch, several
encoders per launch -- against the per-layer entry points with the input projection / its data gradient as torch products.
A FIRST / TOP job must be bit-identical to pnmn_lstm_seq_fwd / _bwd; a SECOND / BELOW job agrees to fp32 round-off (2e-5 of
the largest entry; the products are associated differently)."""
import numpy as np
import pytest
import torch

from probnmn import _hip
from probnmn.modules.seq2seq_base import pack_fragments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: (torch.rand(*s, device=DEV, generator=g) - 0.5) * 0.125  # noqa: E731
    return dict(w_ih=r(1024, 256), w_hh=r(1024, 256), b=r(1024))


def _seq_fwd(xp, tokens, w_hh, B, T):
    hs, cs, act = torch.empty(B, T, 256, device=DEV), torch.empty(B, T, 256, device=DEV), torch.empty(B, T, 1024, device=DEV)
    ws = torch.empty(int(_hip.lib().pnmn_lstm_seq_workspace_bytes(B, 0)), dtype=torch.uint8, device=DEV)
    wp = pack_fragments(w_hh)
    _hip.check(_hip.lib().pnmn_lstm_seq_fwd(xp.data_ptr(), tokens.data_ptr() if tokens is not None else None,
                                            tokens.stride(0) if tokens is not None else 0, wp.data_ptr(), hs.data_ptr(), cs.data_ptr(),
                                            act.data_ptr(), B, T, 256, ws.data_ptr(), _hip.stream_ptr(torch.device(DEV))), "lstm_seq_fwd")
    return hs, cs, act


def _seq_bwd(dhs, act, cs, w_hh, B, T):
    dg = torch.empty(B, T, 1024, device=DEV)
    ws = torch.empty(int(_hip.lib().pnmn_lstm_seq_workspace_bytes(B, 1)), dtype=torch.uint8, device=DEV)
    wt = pack_fragments(w_hh.t())
    _hip.check(_hip.lib().pnmn_lstm_seq_bwd(dhs.data_ptr(), act.data_ptr(), cs.data_ptr(), wt.data_ptr(), dg.data_ptr(), B, T, 256,
                                            ws.data_ptr(), _hip.stream_ptr(torch.device(DEV))), "lstm_seq_bwd")
    return dg


def _reference(enc, B, T, seed):
    """Separate launches: layer 1 from a token table, projection, layer 2; backward from a random output gradient."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    V = 40
    table = (torch.rand(V, 1024, device=DEV, generator=g) - 0.5)
    tokens = torch.randint(0, V, (B, T), device=DEV, generator=g)
    l1, l2 = enc
    hs1, cs1, act1 = _seq_fwd(table, tokens, l1["w_hh"], B, T)
    xp2 = (hs1.double() @ l2["w_ih"].double().t() + l2["b"].double()).float().contiguous()
    hs2, cs2, act2 = _seq_fwd(xp2, None, l2["w_hh"], B, T)
    dhs2 = torch.randn(B, T, 256, device=DEV, generator=g)
    dg2 = _seq_bwd(dhs2, act2, cs2, l2["w_hh"], B, T)
    dhs1 = (dg2.double() @ l2["w_ih"].double()).float().contiguous()
    dg1 = _seq_bwd(dhs1, act1, cs1, l1["w_hh"], B, T)
    return dict(table=table, tokens=tokens, hs1=hs1, cs1=cs1, act1=act1, hs2=hs2, cs2=cs2, act2=act2, dhs2=dhs2, dg2=dg2, dg1=dg1)


def _stack(encs, refs, shapes):
    """All encoders' layers in one forward and one backward launch; returns per encoder the stack's tensors."""
    lib, st = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    n = 2 * len(encs)
    fj, bj = np.zeros(n, _hip.LSTM_STACK_JOB), np.zeros(n, _hip.LSTM_STACK_JOB)
    outs, keep = [], []
    for k, ((l1, l2), ref, (B, T)) in enumerate(zip(encs, refs, shapes)):
        o = {name: torch.full((B, T, w), float("nan"), device=DEV) for name, w in (("hs1", 256), ("cs1", 256), ("act1", 1024), ("hs2", 256),
                                                                                  ("cs2", 256), ("act2", 1024), ("dg1", 1024), ("dg2", 1024))}
        packs = [pack_fragments(l1["w_hh"]), pack_fragments(l2["w_hh"]), pack_fragments(l2["w_ih"]), pack_fragments(l1["w_hh"].t()),
                 pack_fragments(l2["w_hh"].t()), pack_fragments(l2["w_ih"].t())]
        keep.append(packs)
        a, b = fj[2 * k], fj[2 * k + 1]
        a["xp"], a["tokens"], a["token_stride"], a["w_hh"] = ref["table"].data_ptr(), ref["tokens"].data_ptr(), T, packs[0].data_ptr()
        a["hs"], a["cs"], a["act"], a["B"], a["T"], a["dep"] = o["hs1"].data_ptr(), o["cs1"].data_ptr(), o["act1"].data_ptr(), B, T, -1
        b["w_hh"], b["w_ih"], b["bias"] = packs[1].data_ptr(), packs[2].data_ptr(), l2["b"].data_ptr()
        b["hs"], b["cs"], b["act"], b["B"], b["T"], b["dep"] = o["hs2"].data_ptr(), o["cs2"].data_ptr(), o["act2"].data_ptr(), B, T, 2 * k
        # backward: job 2k = layer 2 (top), job 2k + 1 = layer 1 (below it)
        a, b = bj[2 * k], bj[2 * k + 1]
        a["dhs"], a["act"], a["cs"], a["w_hh"], a["dgates"] = ref["dhs2"].data_ptr(), ref["act2"].data_ptr(), ref["cs2"].data_ptr(), packs[4].data_ptr(), o["dg2"].data_ptr()
        a["B"], a["T"], a["dep"] = B, T, -1
        b["act"], b["cs"], b["w_hh"], b["w_ih"], b["dgates"] = ref["act1"].data_ptr(), ref["cs1"].data_ptr(), packs[3].data_ptr(), packs[5].data_ptr(), o["dg1"].data_ptr()
        b["B"], b["T"], b["dep"] = B, T, 2 * k
        outs.append(o)
    for jobs, fn, backward in ((fj, lib.pnmn_lstm_stack_fwd, 0), (bj, lib.pnmn_lstm_stack_bwd, 1)):
        nbytes = int(lib.pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, n, backward))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        for _ in range(2):  # (twice: the counters must come back to zero)
            _hip.check(fn(jobs.ctypes.data, n, ws.data_ptr(), st), "lstm_stack")
        torch.cuda.synchronize()
    return outs


def _close(got, want, tol=2e-5):
    assert torch.isfinite(got).all()
    return float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30) < tol


@pytest.mark.parametrize("shapes", [[(128, 46)], [(20, 5)], [(128, 27), (64, 28)], [(256, 12)], [(33, 1), (50, 9)]])
def test_stack_equals_separate_layers(shapes):
    encs = [(_layer(10 * k + 1), _layer(10 * k + 2)) for k in range(len(shapes))]
    refs = [_reference(enc, B, T, 100 + k) for k, (enc, (B, T)) in enumerate(zip(encs, shapes))]
    outs = _stack(encs, refs, shapes)
    for o, ref in zip(outs, refs):
        for name in ("hs1", "cs1", "act1", "dg2"):  # FIRST / TOP jobs: the per-layer kernels' arithmetic
            assert torch.equal(o[name], ref[name]), name
        for name in ("hs2", "cs2", "act2", "dg1"):
            assert _close(o[name], ref[name]), name


def test_stack_layer_and_decoder_launches_share_one_zeroed_counter_block():
    """Every multi-CU launch leaves the stream's hand-off counter block zeroed for the next one, whichever kernel that is
    (csrc/cluster.h: a stack launch uses five words of a tile's line, the layer and decoder kernels three).  On ONE stream:
    a stack forward (a linked FIRST + SECOND pair of 40 rows x 4 steps -- three tiles, the last of 8 rows -- and an
    independent job of 20 rows x 3 steps), a multi-CU layer forward, a multi-CU teacher-forced decoder forward, the stack
    backward of the same jobs, a multi-CU layer backward; three rounds, every tensor equal to its call's run alone."""
    from probnmn.modules.seq2seq_base import _AttnLSTMDecoder

    lib, st = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    B, T, B3, T3, S, V = 40, 4, 20, 3, 5, 40
    g = torch.Generator(device=DEV).manual_seed(11)
    r = lambda *s, scale=1.0: (torch.rand(*s, device=DEV, generator=g) - 0.5) * scale  # noqa: E731
    l1, l2, l3 = _layer(1), _layer(2), _layer(3)
    table, tokens = r(V, 1024), torch.randint(0, V, (B, T), device=DEV, generator=g)
    xp3, xp = r(B3, T3, 1024), r(B, T, 1024)
    dhs2, dhs3, dhs = r(B, T, 256, scale=2.0), r(B3, T3, 256, scale=2.0), r(B, T, 256, scale=2.0)
    xe, enc, h0 = r(B, T, 1024), r(B, S, 256, scale=2.0), r(B, 256, scale=2.0)
    mask = (torch.arange(S, device=DEV)[None, :] < torch.randint(1, S + 1, (B,), device=DEV, generator=g)[:, None]).float()
    w_c, w_p, b_p = r(1024, 256, scale=0.1), r(V, 256, scale=0.6), r(V)
    packs = dict(hh1=pack_fragments(l1["w_hh"]), hh2=pack_fragments(l2["w_hh"]), ih2=pack_fragments(l2["w_ih"]), hh3=pack_fragments(l3["w_hh"]),
                 hh1t=pack_fragments(l1["w_hh"].t()), hh2t=pack_fragments(l2["w_hh"].t()), ih2t=pack_fragments(l2["w_ih"].t()),
                 hh3t=pack_fragments(l3["w_hh"].t()))
    assert int(lib.pnmn_lstm_seq_workspace_bytes(B, 0)) > 0  # (the layer calls below take the multi-CU kernels)
    fresh = lambda rows, steps, w: torch.full((rows, steps, w), float("nan"), device=DEV)  # noqa: E731

    def launch(fn, jobs, backward):
        nbytes = int(lib.pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, len(jobs), backward))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _hip.check(fn(jobs.ctypes.data, len(jobs), ws.data_ptr(), st), "lstm_stack")

    def stack_fwd():
        o = dict(hs1=fresh(B, T, 256), cs1=fresh(B, T, 256), act1=fresh(B, T, 1024), hs2=fresh(B, T, 256), cs2=fresh(B, T, 256),
                 act2=fresh(B, T, 1024), hs3=fresh(B3, T3, 256), cs3=fresh(B3, T3, 256), act3=fresh(B3, T3, 1024))
        j = np.zeros(3, _hip.LSTM_STACK_JOB)
        a, b, c = j[0], j[1], j[2]
        a["xp"], a["tokens"], a["token_stride"], a["w_hh"] = table.data_ptr(), tokens.data_ptr(), T, packs["hh1"].data_ptr()
        a["hs"], a["cs"], a["act"], a["B"], a["T"], a["dep"] = o["hs1"].data_ptr(), o["cs1"].data_ptr(), o["act1"].data_ptr(), B, T, -1
        b["w_hh"], b["w_ih"], b["bias"] = packs["hh2"].data_ptr(), packs["ih2"].data_ptr(), l2["b"].data_ptr()
        b["hs"], b["cs"], b["act"], b["B"], b["T"], b["dep"] = o["hs2"].data_ptr(), o["cs2"].data_ptr(), o["act2"].data_ptr(), B, T, 0
        c["xp"], c["w_hh"] = xp3.data_ptr(), packs["hh3"].data_ptr()
        c["hs"], c["cs"], c["act"], c["B"], c["T"], c["dep"] = o["hs3"].data_ptr(), o["cs3"].data_ptr(), o["act3"].data_ptr(), B3, T3, -1
        launch(lib.pnmn_lstm_stack_fwd, j, 0)
        return o

    def stack_bwd(f):
        o = dict(dg2=fresh(B, T, 1024), dg1=fresh(B, T, 1024), dg3=fresh(B3, T3, 1024))
        j = np.zeros(3, _hip.LSTM_STACK_JOB)
        a, b, c = j[0], j[1], j[2]
        a["dhs"], a["act"], a["cs"], a["w_hh"], a["dgates"] = dhs2.data_ptr(), f["act2"].data_ptr(), f["cs2"].data_ptr(), packs["hh2t"].data_ptr(), o["dg2"].data_ptr()
        a["B"], a["T"], a["dep"] = B, T, -1
        b["act"], b["cs"], b["w_hh"], b["w_ih"], b["dgates"] = f["act1"].data_ptr(), f["cs1"].data_ptr(), packs["hh1t"].data_ptr(), packs["ih2t"].data_ptr(), o["dg1"].data_ptr()
        b["B"], b["T"], b["dep"] = B, T, 0
        c["dhs"], c["act"], c["cs"], c["w_hh"], c["dgates"] = dhs3.data_ptr(), f["act3"].data_ptr(), f["cs3"].data_ptr(), packs["hh3t"].data_ptr(), o["dg3"].data_ptr()
        c["B"], c["T"], c["dep"] = B3, T3, -1
        launch(lib.pnmn_lstm_stack_bwd, j, 1)
        return o

    def layer_fwd():
        return dict(zip(("hs", "cs", "act"), _seq_fwd(xp, None, l3["w_hh"], B, T)))

    def decoder_fwd():
        with torch.no_grad():
            hs, _ = _AttnLSTMDecoder.apply(xe, None, enc, mask, h0, w_c, l1["w_hh"], w_p, b_p, 0, T, 5, 3, 0, 1, 2)
        return dict(dec_hs=hs)

    def alone(fn, *args):
        out = fn(*args)
        torch.cuda.synchronize()
        return out

    assert _hip.decoder_workspace_bytes([B], False) > 0  # (the decoder call takes the multi-CU kernel)
    want_f = alone(stack_fwd)
    want_l = alone(layer_fwd)
    layer_bwd = lambda: dict(dg=_seq_bwd(dhs, want_l["act"], want_l["cs"], l3["w_hh"], B, T))  # noqa: E731
    calls = [(stack_fwd, (), want_f), (layer_fwd, (), want_l), (decoder_fwd, (), alone(decoder_fwd)),
             (stack_bwd, (want_f,), alone(stack_bwd, want_f)), (layer_bwd, (), alone(layer_bwd))]
    for want in (c[2] for c in calls):
        assert all(torch.isfinite(v).all() for v in want.values())
    for rnd in range(3):
        got = [fn(*args) for fn, args, _ in calls]  # back to back, nothing but the stream orders them
        torch.cuda.synchronize()
        for (_, _, want), out in zip(calls, got):
            for name in want:
                assert torch.equal(out[name], want[name]), (rnd, name)


def test_does_not_fit_reports_zero_workspace():
    jobs = np.zeros(2, _hip.LSTM_STACK_JOB)
    jobs["B"], jobs["T"], jobs["dep"] = 1024, 10, -1
    assert int(_hip.lib().pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, 2, 0)) == 0


def test_rate_report(capsys):
    B, T = 128, 46
    enc = [(_layer(1), _layer(2))]
    ref = [_reference(enc[0], B, T, 5)]
    import time
    lib, st = _hip.lib(), _hip.stream_ptr(torch.device(DEV))

    def clock(fn, reps=10):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    t_sep = clock(lambda: _reference(enc[0], B, T, 5))
    t_stack = clock(lambda: _stack(enc, ref, [(B, T)]))
    with capsys.disabled():
        print("encoder forward + backward, %d rows x %d steps: separate launches (+ torch fp64 projections) %.0f us, stack (x2 runs) %.0f us"
              % (B, T, t_sep, t_stack))
