"""The teacher-forced attention decoders against the fp64 host reference (tests/helpers/decoder_reference.py), forward and
backward, every tensor they save or emit, through three entry points:

  one_workgroup  pnmn_attn_lstm_fwd / pnmn_attn_lstm_bwd (denc zero on entry, accumulated by the kernel)
  group          pnmn_attn_lstm_fwd_group / pnmn_attn_lstm_bwd_group with n = 1, then pnmn_attn_denc: dctx, dscore and weights
                 one by one, and the denc assembled from them
  ordered        pnmn_attn_lstm_fwd_group_ordered / pnmn_attn_lstm_bwd_group_ordered with the lists of pnmn_length_order_steps,
                 against the reference with zeros from the tile's steps on (cs, act and probs, unwritten there, up to there)

Every output is NaN before each call.  The cases, their three input regimes and the error bar -- derived from the reference's
own float32 round-off, bar = min(1e-4, max(16 e32, 2e-6)) of the tensor's largest entry -- are stated in the helper;
tests/test_decoder_reference.py shows on the CPU that every case can tell a wrong attention rule from the right one.  Each
test prints error / bar of every tensor before it asserts.

Worst error / bar over all cases and tensors, measured on an MI355X with the kernels of commit 9111e35 (the parent of the
commit that added this file, which changes no kernel), and the tensor and case that gave it:

  one_workgroup  0.43   dgates of b1_t9_s64 (bar 2.3e-6); every other case stays below 0.17
  group          0.098  act of b1_t1_s1 (bar 5.9e-6); the diffuse cases stay below 0.08
  ordered        0.098  act of b1_t1_s1 (bar 5.9e-6): the bits of the group call wherever a tile runs

All 42 tests together take 3 s.  No kernel defect was found.  A build with the mask dropped from the first level of the
masked-softmax backward (dp = dq in the place of dp = dq * mask, in both kernel families) fails every case but the unmasked one,
through all three entry points, while the group-against-lone and ordered-against-plain tests (test_decoder_variants_gpu.py,
test_decoder_length_order_gpu.py) pass it.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_reference as dr  # noqa: E402

from probnmn import _hip  # noqa: E402
from probnmn.modules.seq2seq_base import pack_fragments  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = dr.H
NO_OPTIONS = (None, 0, None, None, None, 0, 0)  # (filter, end index, the automaton's three tables, n_states, n_classes)
FWD_OUT = dict(hs=H, cs=H, act=4 * H, ctx=H, probs="S")
GROUP_BWD_OUT = dict(dgates=4 * H, dctx=H, dscore="S", weights="S")


def _stream():
    return _hip.stream_ptr(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _problem(name):
    """A case's inputs on the device, W_c / W_hh and their transposes in fragment order."""
    i = dr.case_inputs(name)
    d = i["d"]
    p = {k: d[k].to(DEV).contiguous() for k in ("enc", "mask", "h0", "etable")}
    p.update(w_c=pack_fragments(d["w_c"].to(DEV)), w_hh=pack_fragments(d["w_hh"].to(DEV)),
             w_c_t=pack_fragments(d["w_c"].t().to(DEV)), w_hh_t=pack_fragments(d["w_hh"].t().to(DEV)),
             xe=None if i["xe"] is None else i["xe"].to(DEV).contiguous(),
             in_tokens=None if i["in_tokens"] is None else i["in_tokens"].to(DEV).contiguous(),
             dhs=i["dhs"].to(DEV).contiguous(), steps=i["steps"])
    p["B"], p["T"], p["S"] = i["dhs"].size(0), i["dhs"].size(1), d["enc"].size(1)
    return p


def _nan(p, widths):
    return {k: torch.full((p["B"], p["T"], p["S"] if w == "S" else w), float("nan"), device=DEV) for k, w in widths.items()}


def _workspace(B, backward):
    n = _hip.decoder_workspace_bytes([B], backward)
    assert n > 0  # (the multi-CU kernels do take this pass)
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _lists(p):
    """The device lists of pnmn_length_order_steps for the case's steps, held to the reference's statement of them."""
    B, T = p["B"], p["T"]
    steps = torch.as_tensor(p["steps"], dtype=torch.int32, device=DEV)
    order = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tile_steps = torch.full(((B + 15) // 16,), -1, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pnmn_length_order_steps(steps.data_ptr(), B, T, order.data_ptr(), tile_steps.data_ptr(), _stream()),
               "length_order_steps")
    want_order, want_tile_steps, of_row = dr.row_tile_steps(p["steps"], T)
    assert np.array_equal(order.cpu().numpy(), want_order) and np.array_equal(tile_steps.cpu().numpy(), want_tile_steps)
    arr = np.array([[order.data_ptr()], [tile_steps.data_ptr()]], np.uint64)
    return (order, tile_steps, arr), (arr[0].ctypes.data, arr[1].ctypes.data), of_row


def _forward(p, entry, ptrs=None):
    out = _nan(p, FWD_OUT)
    job = np.zeros(1, _hip.DECODER_FWD_JOB)
    j = job[0]
    for k in ("enc", "mask", "h0", "w_c", "w_hh"):
        j[k] = p[k].data_ptr()
    for k in FWD_OUT:
        j[k] = out[k].data_ptr()
    if p["xe"] is not None:
        j["xe"] = p["xe"].data_ptr()
    else:
        j["etable"], j["in_tokens"], j["in_token_stride"] = p["etable"].data_ptr(), p["in_tokens"].data_ptr(), p["in_tokens"].stride(0)
    j["B"], j["T"], j["S"] = p["B"], p["T"], p["S"]
    lib = _hip.lib()
    if entry == "one_workgroup":
        rc = lib.pnmn_attn_lstm_fwd(job.ctypes.data, H, *NO_OPTIONS, _stream())
    else:
        ws = _workspace(p["B"], False)
        if entry == "group":
            rc = lib.pnmn_attn_lstm_fwd_group(job.ctypes.data, *NO_OPTIONS, 1, H, ws.data_ptr(), _stream())
        else:
            rc = lib.pnmn_attn_lstm_fwd_group_ordered(job.ctypes.data, *NO_OPTIONS, 1, H, *ptrs, ws.data_ptr(), _stream())
    _hip.check(rc, "attn_lstm_fwd " + entry)
    torch.cuda.synchronize()
    return out


def _backward(p, fwd, entry, ptrs=None):
    B, T, S = p["B"], p["T"], p["S"]
    lib = _hip.lib()
    dh0 = torch.full((B, H), float("nan"), device=DEV)
    if entry == "one_workgroup":
        out = dict(_nan(p, dict(dgates=4 * H)), dh0=dh0, denc=torch.zeros(B, S, H, device=DEV))  # (denc: zero on entry)
        rc = lib.pnmn_attn_lstm_bwd(p["dhs"].data_ptr(), fwd["act"].data_ptr(), fwd["cs"].data_ptr(), fwd["hs"].data_ptr(),
                                    fwd["ctx"].data_ptr(), fwd["probs"].data_ptr(), p["enc"].data_ptr(), p["mask"].data_ptr(),
                                    p["h0"].data_ptr(), p["w_c_t"].data_ptr(), p["w_hh_t"].data_ptr(), out["dgates"].data_ptr(),
                                    out["denc"].data_ptr(), out["dh0"].data_ptr(), B, T, S, H, _stream())
        _hip.check(rc, "attn_lstm_bwd")
        torch.cuda.synchronize()
        return out
    out = dict(_nan(p, GROUP_BWD_OUT), dh0=dh0, denc=torch.full((B, S, H), float("nan"), device=DEV))
    job = np.zeros(1, _hip.DECODER_BWD_JOB)
    j = job[0]
    for k in ("dhs", "enc", "mask", "h0", "w_c_t", "w_hh_t"):
        j[k] = p[k].data_ptr()
    for k in ("act", "cs", "hs", "probs"):
        j[k] = fwd[k].data_ptr()
    for k in tuple(GROUP_BWD_OUT) + ("dh0",):
        j[k] = out[k].data_ptr()
    j["B"], j["T"], j["S"] = B, T, S
    ws = _workspace(B, True)
    if entry == "group":
        rc = lib.pnmn_attn_lstm_bwd_group(job.ctypes.data, 1, H, ws.data_ptr(), _stream())
    else:
        rc = lib.pnmn_attn_lstm_bwd_group_ordered(job.ctypes.data, 1, H, *ptrs, ws.data_ptr(), _stream())
    _hip.check(rc, "attn_lstm_bwd " + entry)
    _hip.check(lib.pnmn_attn_denc(out["weights"].data_ptr(), out["dscore"].data_ptr(), out["dctx"].data_ptr(), fwd["hs"].data_ptr(),
                                  p["h0"].data_ptr(), out["denc"].data_ptr(), B, T, S, H, _stream()), "attn_denc")
    torch.cuda.synchronize()
    return out


def _compare(name, entry, got, ref, bars, ran=None):
    """error / bar of every tensor in ``got``, printed, then asserted <= 1; a reference that is identically zero: exactly
    zero.  ``ran`` [B,T]: where the UNWRITTEN tensors are defined."""
    ratios = {}
    for k, tensor in got.items():
        g, want = tensor.double().cpu(), ref[k]
        assert g.shape == want.shape, k
        if ran is not None and k in dr.UNWRITTEN:
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


@pytest.mark.parametrize("entry", ["one_workgroup", "group"])
@pytest.mark.parametrize("name", [c["name"] for c in dr.CASES])
def test_decoder_matches_the_fp64_reference(name, entry):
    p, ref, bars = _problem(name), dr.case_reference(name), dr.case_bars(name)
    fwd = _forward(p, entry)
    _compare(name, entry, dict(fwd, **_backward(p, fwd, entry)), ref, bars)


@pytest.mark.parametrize("name", [c["name"] for c in dr.CASES])
def test_ordered_decoder_matches_the_fp64_reference_with_its_tails_zeroed(name):
    p = _problem(name)
    keep, ptrs, of_row = _lists(p)
    ref, bars = dr.zero_tails(dr.case_reference(name), p["steps"], p["T"]), dr.case_bars(name, ordered=True)
    ran = torch.arange(p["T"])[None, :] < torch.as_tensor(of_row)[:, None]
    fwd = _forward(p, "ordered", ptrs)
    _compare(name, "ordered", dict(fwd, **_backward(p, fwd, "ordered", ptrs)), ref, bars, ran)
