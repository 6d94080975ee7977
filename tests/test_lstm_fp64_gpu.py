"""The recurrent layer kernels against the fp64 host reference (tests/helpers/lstm_reference.py), forward and backward, every
tensor they save or emit:

  one_workgroup          pnmn_lstm_seq_fwd / _bwd with workspace = NULL: one workgroup per 16-row tile
  cluster                the same with a workspace of pnmn_lstm_seq_workspace_bytes: 8 or 4 workgroups per tile
  ordered_one_workgroup  pnmn_lstm_seq_fwd_ordered / _bwd_ordered with the lists of pnmn_length_order_steps (held to
  ordered_cluster        row_tile_steps first), against the reference with zeros from the tile's steps on
  stack                  pnmn_lstm_stack_fwd_dropout / _bwd_dropout (pnmn_lstm_stack_fwd / _bwd too where p = 0): a linked pair
                         of layers and an independent rider job in one launch, each launch made twice
  cell                   pnmn_lstm_cell_fwd / _bwd at hidden 1, 3, 256, 300

Every output is NaN before each call and the backward takes the cs / act its own entry point's forward just wrote.  Which
kernel ran is asserted from the workspace size (the members per tile), on the full chip and with all but 64 CUs reserved,
where 144 rows take the 4-member kernels and 260 rows run as two launches over row ranges.  The cases, their three input
regimes and the error bar -- derived from the reference's own float32 round-off, bar = min(1e-4, max(16 e32, 2e-6)) of the
tensor's largest entry -- are stated in the helper; tests/test_lstm_reference.py shows on the CPU that every case can tell a
wrong recurrence from the right one.  Each test prints error / bar of every tensor before it asserts.

Worst error / bar over all cases and tensors, measured on an MI355X (256 CUs) with the kernels of commit 6ca4aa8 (the parent of
the commit that added this file, which changes no kernel), and the tensor and case that gave it:

  one_workgroup          0.33   cs of b520_t2 (bar 2e-6); then act of b520_t2 0.33, dgates of b144_t3_tok 0.29
  cluster                0.33   the same three, the reserved runs (4 members, row ranges) included
  ordered_one_workgroup  0.33   the same: the figures of the plain calls wherever a tile runs
  ordered_cluster        0.33   the same
  stack                  0.42   act of the rider beside s_b40_t3_tok_p05 (bar 2e-6); of a pair: below 0.3
  cell                   0.088  dgates of hidden 1, B = 17 (bar 2.3e-6)

All 71 tests together take 3.3 s.  No kernel defect was found.  A build in which the forget-gate gradient of every backward
cell uses c_t where c_{t-1} belongs (df = dc c_t f (1 - f); the cell kernel, both layer kernels, the stack kernel; no
addressing, hand-off or launch code touched) fails 69 of them: every layer, ordered, reserved, stack and cell test, T = 1
included (c_0 is not the zero that c_{-1} is); the two forward-only act == NULL tests pass it.  All 57 of the
kernel-against-kernel tests pass that build: the 8 of test_lstm_stack_gpu.py, the 42 of test_lstm_length_order_gpu.py and the 7
cases of test_multi_cu_lstm_layer_matches_one_workgroup_per_tile in test_seq2seq_gpu.py.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_reference as lr  # noqa: E402

from probnmn import _hip  # noqa: E402
from probnmn.modules.seq2seq_base import pack_fragments  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = lr.H
NAMES = [c["name"] for c in lr.CASES]
ENTRIES = dict(one_workgroup=(False, False), cluster=(False, True), ordered_one_workgroup=(True, False), ordered_cluster=(True, True))
LEFT = 64  # CUs the reserved tests leave to the multi-CU kernels


def _stream():
    return _hip.stream_ptr(torch.device(DEV))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.fixture
def reserve():
    lib = _hip.lib()
    full = lib.pnmn_cluster_reserve_cus(0)
    yield lambda n: lib.pnmn_cluster_reserve_cus(n)
    lib.pnmn_cluster_reserve_cus(0)
    assert lib.pnmn_cluster_reserve_cus(-1) == full


# ---- which kernel runs: the rule of include/probnmn_hip.h and csrc/cluster.h, restated -------------------------------------
def _split(tiles, cus):
    """Members per tile of one launch over ``tiles`` tiles: 8 when 8 workgroups for every tile of every group of eight tiles
    are resident at once on ``cus`` CUs, else 4 when those are, else 0 (no single launch)."""
    groups = (tiles + 7) // 8
    return 8 if 64 * groups <= cus else 4 if 32 * groups <= cus else 0


def _ranges(B, cus):
    """[(tiles, members)] of the launches that cover B rows: one when the tiles fit, else ranges of 8 * (cus // 32) tiles."""
    tiles = (B + 15) // 16
    if _split(tiles, cus):
        return [(tiles, _split(tiles, cus))]
    most = 8 * (cus // 32)
    return [(min(most, tiles - t0), _split(min(most, tiles - t0), cus)) for t0 in range(0, tiles, most)] if most else []


def _members(B, cus):
    """The launches of a multi-CU pass over B rows, the library's exchange buffer held to them: it is sized for the first
    range's tiles x members (2 x 16 x 256 floats each), the backward workspace being the forward's plus that buffer."""
    lib = _hip.lib()
    assert lib.pnmn_cluster_reserve_cus(-1) == cus
    ranges = _ranges(B, cus)
    fwd, bwd = int(lib.pnmn_lstm_seq_workspace_bytes(B, 0)), int(lib.pnmn_lstm_seq_workspace_bytes(B, 1))
    if not ranges:
        assert fwd == 0 and bwd == 0
        return ranges
    assert fwd > 0 and (bwd - fwd) % (2 * 16 * 256 * 4) == 0
    assert (bwd - fwd) // (2 * 16 * 256 * 4) == ranges[0][0] * ranges[0][1], (B, cus, ranges)
    return ranges


def _token_view(tokens):
    """The case's token rows on the device as they are on the host: a [B,T] view into a [B,T+3] tensor."""
    B, T = tokens.shape
    view = tokens._base.to(DEV)[:, :T]
    assert view.stride() == (T + 3, 1) and torch.equal(view.cpu(), tokens)
    return view


# ---- the layer ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(name):
    """A layer case's inputs on the device, W_hh and its transpose in fragment order."""
    i = lr.case_inputs(name)
    B, T = i["dhs"].shape[:2]
    p = dict(B=B, T=T, steps=i["steps"], dhs=i["dhs"].to(DEV).contiguous(), w_hh=pack_fragments(i["w_hh"].to(DEV)),
             w_hh_t=pack_fragments(i["w_hh"].t().to(DEV)), tokens=None)
    if isinstance(i["x"], tuple):
        p["xp"], p["tokens"] = i["x"][0].to(DEV).contiguous(), _token_view(i["x"][1])
    else:
        p["xp"] = i["x"].to(DEV).contiguous()
    return p


def _lists(p):
    """The device lists of pnmn_length_order_steps for the case's steps, held to the reference's statement of them."""
    B, T = p["B"], p["T"]
    steps = torch.as_tensor(p["steps"], dtype=torch.int32, device=DEV)
    order = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tile_steps = torch.full(((B + 15) // 16,), -1, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pnmn_length_order_steps(steps.data_ptr(), B, T, order.data_ptr(), tile_steps.data_ptr(), _stream()),
               "length_order_steps")
    want_order, want_tile_steps, of_row = lr.row_tile_steps(p["steps"], T)
    assert np.array_equal(order.cpu().numpy(), want_order) and np.array_equal(tile_steps.cpu().numpy(), want_tile_steps)
    return (order, tile_steps), of_row


def _workspace(B, backward):
    n = int(_hip.lib().pnmn_lstm_seq_workspace_bytes(B, backward))
    assert n > 0  # (the multi-CU kernels do take this pass)
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _layer_forward(p, cluster, lists=None, with_act=True):
    B, T = p["B"], p["T"]
    out = dict(hs=_nan(B, T, H), cs=_nan(B, T, H))
    if with_act:
        out["act"] = _nan(B, T, 4 * H)
    ws = _workspace(B, 0) if cluster else None
    args = (p["xp"].data_ptr(), p["tokens"].data_ptr() if p["tokens"] is not None else None,
            p["tokens"].stride(0) if p["tokens"] is not None else 0, p["w_hh"].data_ptr(), out["hs"].data_ptr(), out["cs"].data_ptr(),
            out["act"].data_ptr() if with_act else None, B, T, H)
    tail = (ws.data_ptr() if cluster else None, _stream())
    lib = _hip.lib()
    if lists is None:
        rc = lib.pnmn_lstm_seq_fwd(*args, *tail)
    else:
        rc = lib.pnmn_lstm_seq_fwd_ordered(*args, lists[0].data_ptr(), lists[1].data_ptr(), *tail)
    _hip.check(rc, "lstm_seq_fwd")
    torch.cuda.synchronize()
    return out


def _layer_backward(p, fwd, cluster, lists=None, dhs=None):
    B, T = p["B"], p["T"]
    dgates = _nan(B, T, 4 * H)
    ws = _workspace(B, 1) if cluster else None
    args = ((p["dhs"] if dhs is None else dhs).data_ptr(), fwd["act"].data_ptr(), fwd["cs"].data_ptr(), p["w_hh_t"].data_ptr(),
            dgates.data_ptr(), B, T, H)
    tail = (ws.data_ptr() if cluster else None, _stream())
    lib = _hip.lib()
    if lists is None:
        rc = lib.pnmn_lstm_seq_bwd(*args, *tail)
    else:
        rc = lib.pnmn_lstm_seq_bwd_ordered(*args, lists[0].data_ptr(), lists[1].data_ptr(), *tail)
    _hip.check(rc, "lstm_seq_bwd")
    torch.cuda.synchronize()
    return dgates


def _compare(name, entry, got, ref, bars, ran=None):
    """error / bar of every tensor in ``got``, printed, then asserted <= 1; a reference that is identically zero: exactly
    zero.  ``ran`` [B,T]: where the UNWRITTEN tensors are defined."""
    ratios = {}
    for k, tensor in got.items():
        g, want = tensor.double().cpu(), ref[k]
        assert g.shape == want.shape, k
        if ran is not None and k in lr.UNWRITTEN:
            g, want = g[ran], want[ran]
        assert bool(torch.isfinite(g).all()), (name, entry, k)
        scale, bar = bars[k]
        if scale == 0.0:
            assert float(g.abs().max()) == 0.0, (name, entry, k)
            continue
        ratios[k] = float((g - want).abs().max()) / scale / bar
        print("%s %s %s: bar %.3g, error / bar %.3g" % (name, entry, k, bar, ratios[k]))
    over = {k: round(r, 3) for k, r in ratios.items() if not r <= 1.0}
    assert not over, (name, entry, over)


def _run_layer(name, entry):
    ordered, cluster = ENTRIES[entry]
    p = _problem(name)
    if not ordered:
        fwd = _layer_forward(p, cluster)
        got = dict(fwd, dgates=_layer_backward(p, fwd, cluster))
        _compare(name, entry, got, lr.case_reference(name), lr.case_bars(name))
        return
    B, T = p["B"], p["T"]
    lists, of_row = _lists(p)
    ran = torch.arange(T)[None, :] < torch.as_tensor(of_row)[:, None]
    valid = torch.arange(T)[None, :] < torch.as_tensor(p["steps"])[:, None]
    dhs = torch.where(ran[:, :, None].to(DEV), p["dhs"], torch.full_like(p["dhs"], float("nan")))  # not read behind the tile
    fwd = _layer_forward(p, cluster, lists)
    got = dict(fwd, dgates=_layer_backward(p, fwd, cluster, lists, dhs))
    for k in lr.ZEROED:  # exactly zero from the tile's step count on; dgates from the row's own on
        cut = got[k].cpu()[~(ran if k == "hs" else valid)]
        assert cut.numel() == 0 or float(cut.abs().max()) == 0.0, (name, entry, k)
    # (cs / act where the tile ran, the steps between a row's own count and its tile's included: the plain recurrence there)
    _compare(name, entry, got, lr.zero_tails(lr.case_reference(name), p["steps"], T), lr.case_bars(name, ordered=True), ran)


def _expect_on_the_full_chip(name, cluster):
    """The launches of the case on the chip as it is; on 256 CUs: 8 members up to 512 rows, 4 for 520."""
    if not cluster:
        return
    B = _problem(name)["B"]
    full = _hip.lib().pnmn_cluster_reserve_cus(0)
    ranges = _members(B, full)
    if not ranges:
        pytest.skip("no multi-CU launch covers %d rows on %d CUs" % (B, full))
    if full == 256:
        assert ranges == [((B + 15) // 16, 4 if B == 520 else 8)]
    elif B == 520 and ranges[0][1] != 4:
        pytest.skip("%d CUs: 33 tiles do not take the 4-member kernels in one launch" % full)


@pytest.mark.parametrize("entry", ["one_workgroup", "cluster"])
@pytest.mark.parametrize("name", NAMES)
def test_layer_matches_the_fp64_reference(name, entry):
    _expect_on_the_full_chip(name, ENTRIES[entry][1])
    _run_layer(name, entry)


@pytest.mark.parametrize("entry", ["ordered_one_workgroup", "ordered_cluster"])
@pytest.mark.parametrize("name", NAMES)
def test_ordered_layer_matches_the_fp64_reference_with_its_tails_zeroed(name, entry):
    _expect_on_the_full_chip(name, ENTRIES[entry][1])
    _run_layer(name, entry)


@pytest.mark.parametrize("entry", ["cluster", "ordered_cluster"])
@pytest.mark.parametrize("name", ["b144_t3_tok", "b260_t3_tok", "b260_t3"])
def test_four_member_kernels_and_row_ranges_match_the_fp64_reference(reserve, name, entry):
    """All but 64 CUs reserved: 9 tiles take the 4-member kernels, 17 tiles run as a launch of 16 (4 members) and one of 1 (8):
    the token rows, the tensor bases and the order / tile_steps lists each advance differently with the range."""
    full = reserve(0)
    if full < LEFT + 32:
        pytest.skip("%d CUs: nothing to reserve down to %d" % (full, LEFT))
    assert reserve(full - LEFT) == LEFT
    B = _problem(name)["B"]
    assert _members(B, LEFT) == ([(9, 4)] if B == 144 else [(16, 4), (1, 8)])
    _run_layer(name, entry)


@pytest.mark.parametrize("cluster", [False, True])
def test_forward_without_act_writes_the_same_hs_and_cs(cluster):
    p = _problem("b17_t9_tok")
    with_act, without = _layer_forward(p, cluster), _layer_forward(p, cluster, with_act=False)
    for k in ("hs", "cs"):
        assert bool(torch.isfinite(without[k]).all()) and torch.equal(without[k], with_act[k]), k


# ---- the stack ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack_problem(name):
    i = lr.stack_inputs(name)
    B, T = i["dhs2"].shape[:2]
    p = dict(B=B, T=T, p=i["p"], seed=i["seed"], row_offset=i["row_offset"], tokens=None)
    if isinstance(i["x"], tuple):
        p["xp"], p["tokens"] = i["x"][0].to(DEV).contiguous(), _token_view(i["x"][1])
    else:
        p["xp"] = i["x"].to(DEV).contiguous()
    for k in ("b2", "dhs2", "x3", "dhs3"):
        p[k] = i[k].to(DEV).contiguous()
    for k in ("w_hh1", "w_ih2", "w_hh2", "w_hh3"):
        p[k], p[k + "_t"] = pack_fragments(i[k].to(DEV)), pack_fragments(i[k].t().to(DEV))
    return p


def _twice(fn, jobs, drops, backward, outs):
    """The launch made twice, the outputs NaN again in between: the second finds the hand-off counters as the first left them."""
    lib = _hip.lib()
    nbytes = int(lib.pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, len(jobs), backward))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        args = (jobs.ctypes.data,) + (() if drops is None else (drops.ctypes.data,)) + (len(jobs), ws.data_ptr(), _stream())
        _hip.check(fn(*args), "lstm_stack")
        torch.cuda.synchronize()


def _run_stack(name, plain):
    """Forward: job 0 = layer 1 (FIRST), job 1 = layer 2 (SECOND, above job 0), job 2 = the rider.  Backward: job 0 = layer 2
    (TOP), job 1 = layer 1 (BELOW job 0), job 2 = the rider.  ``plain``: the entry points without descriptors (p = 0)."""
    p, lib = _stack_problem(name), _hip.lib()
    B, T, (B3, T3) = p["B"], p["T"], lr.RIDER
    o = {k: _nan(B, T, 4 * H if k[:2] in ("ac", "dg") else H) for k in lr.STACK}
    o.update(hs3=_nan(B3, T3, H), cs3=_nan(B3, T3, H), act3=_nan(B3, T3, 4 * H), dg3=_nan(B3, T3, 4 * H))
    ptr = {k: v.data_ptr() for k, v in o.items()}
    fj, bj = np.zeros(3, _hip.LSTM_STACK_JOB), np.zeros(3, _hip.LSTM_STACK_JOB)
    fd, bd = np.zeros(3, _hip.LSTM_DROPOUT_DESC), np.zeros(3, _hip.LSTM_DROPOUT_DESC)
    a, b, c = fj[0], fj[1], fj[2]
    a["xp"], a["w_hh"] = p["xp"].data_ptr(), p["w_hh1"].data_ptr()
    if p["tokens"] is not None:
        a["tokens"], a["token_stride"] = p["tokens"].data_ptr(), p["tokens"].stride(0)
    a["hs"], a["cs"], a["act"], a["B"], a["T"], a["dep"] = ptr["hs1"], ptr["cs1"], ptr["act1"], B, T, -1
    b["w_hh"], b["w_ih"], b["bias"] = p["w_hh2"].data_ptr(), p["w_ih2"].data_ptr(), p["b2"].data_ptr()
    b["hs"], b["cs"], b["act"], b["B"], b["T"], b["dep"] = ptr["hs2"], ptr["cs2"], ptr["act2"], B, T, 0
    c["xp"], c["w_hh"] = p["x3"].data_ptr(), p["w_hh3"].data_ptr()
    c["hs"], c["cs"], c["act"], c["B"], c["T"], c["dep"] = ptr["hs3"], ptr["cs3"], ptr["act3"], B3, T3, -1
    a, b, c = bj[0], bj[1], bj[2]
    a["dhs"], a["act"], a["cs"], a["w_hh"], a["dgates"] = p["dhs2"].data_ptr(), ptr["act2"], ptr["cs2"], p["w_hh2_t"].data_ptr(), ptr["dg2"]
    a["B"], a["T"], a["dep"] = B, T, -1
    b["act"], b["cs"], b["w_hh"], b["w_ih"], b["dgates"] = ptr["act1"], ptr["cs1"], p["w_hh1_t"].data_ptr(), p["w_ih2_t"].data_ptr(), ptr["dg1"]
    b["B"], b["T"], b["dep"] = B, T, 0
    c["dhs"], c["act"], c["cs"], c["w_hh"], c["dgates"] = p["dhs3"].data_ptr(), ptr["act3"], ptr["cs3"], p["w_hh3_t"].data_ptr(), ptr["dg3"]
    c["B"], c["T"], c["dep"] = B3, T3, -1
    fd[0]["p"], fd[0]["seed"], fd[0]["row_offset"], fd[0]["hsd"] = p["p"], p["seed"], p["row_offset"], ptr["hsd"]
    bd[1]["p"], bd[1]["seed"], bd[1]["row_offset"] = p["p"], p["seed"], p["row_offset"]
    forward = [o[k] for k in ("hs1", "hsd", "cs1", "act1", "hs2", "cs2", "act2", "hs3", "cs3", "act3")]
    backward = [o[k] for k in ("dg2", "dg1", "dg3")]
    if plain:
        assert p["p"] == 0.0
        _twice(lib.pnmn_lstm_stack_fwd, fj, None, 0, forward)
        _twice(lib.pnmn_lstm_stack_bwd, bj, None, 1, backward)
    else:
        _twice(lib.pnmn_lstm_stack_fwd_dropout, fj, fd, 0, forward)
        _twice(lib.pnmn_lstm_stack_bwd_dropout, bj, bd, 1, backward)
    if p["p"] == 0.0:
        assert bool(torch.isnan(o.pop("hsd")).all())  # (p = 0: nothing written)
    entry = "stack" if plain else "stack_dropout"
    _compare(name, entry, o, lr.stack_case_reference(name), lr.stack_case_bars(name))  # (p = 1: hsd and dg1 exactly zero)


@pytest.mark.parametrize("name", [c["name"] for c in lr.STACK_CASES])
def test_stack_with_dropout_descriptors_matches_the_fp64_reference(name):
    _run_stack(name, plain=False)


@pytest.mark.parametrize("name", [c["name"] for c in lr.STACK_CASES if c["p"] == 0.0])
def test_stack_matches_the_fp64_reference(name):
    _run_stack(name, plain=True)


# ---- the cell -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("hidden", [1, 3, 256, 300])
def test_cell_matches_the_fp64_reference(hidden, B):
    """Forward with and without ``act``; backward with both gradients, with dh alone and with dc_in alone.  c_prev ~ 2 N(0, 1)."""
    g = torch.Generator().manual_seed(4000 + 7 * hidden + B)
    gates, c_prev = 1.5 * torch.randn(B, 4 * hidden, generator=g), 2.0 * torch.randn(B, hidden, generator=g)
    dh, dc = torch.randn(B, hidden, generator=g), torch.randn(B, hidden, generator=g)
    dev = {k: v.to(DEV) for k, v in dict(gates=gates, c_prev=c_prev, dh=dh, dc=dc).items()}
    lib, name = _hip.lib(), "cell_h%d_b%d" % (hidden, B)

    def forward(with_act):
        out = dict(h=_nan(B, hidden), c=_nan(B, hidden))
        if with_act:
            out["act"] = _nan(B, 4 * hidden)
        _hip.check(lib.pnmn_lstm_cell_fwd(dev["gates"].data_ptr(), dev["c_prev"].data_ptr(), out["h"].data_ptr(), out["c"].data_ptr(),
                                          out["act"].data_ptr() if with_act else None, B, hidden, _stream()), "lstm_cell_fwd")
        torch.cuda.synchronize()
        return out

    fwd, bare = forward(True), forward(False)
    for k in ("h", "c"):
        assert torch.equal(bare[k], fwd[k]), k
    for which, (use_dh, use_dc) in dict(both=(True, True), dh=(True, False), dc_in=(False, True)).items():
        out = dict(dgates=_nan(B, 4 * hidden), dc_prev=_nan(B, hidden))
        _hip.check(lib.pnmn_lstm_cell_bwd(fwd["act"].data_ptr(), dev["c_prev"].data_ptr(), fwd["c"].data_ptr(),
                                          dev["dh"].data_ptr() if use_dh else None, dev["dc"].data_ptr() if use_dc else None,
                                          out["dgates"].data_ptr(), out["dc_prev"].data_ptr(), B, hidden, _stream()), "lstm_cell_bwd")
        torch.cuda.synchronize()
        args = (gates, c_prev, dh if use_dh else None, dc if use_dc else None)
        ref, f32 = lr.cell_reference(*args), lr.cell_reference(*args, dtype=torch.float32)
        _compare(name, "cell " + which, dict(fwd, **out), ref, lr.error_bars(ref, f32))
