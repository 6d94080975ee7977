"""Launching a group of attention-decoder passes is launching its members (pnmn_attn_lstm_fwd_group / _fwd_group_ordered,
pnmn_attn_lstm_bwd_group / _bwd_group_ordered): every kernel variant the launcher can pick -- one or more passes per launch,
OVERLAP on and off, every mode of a pass, with and without the token automaton, with and without an order -- against the lone
calls of the same passes, bit for bit on every output of every job.  Every output is pre-filled with a marker before each
call, so a pass that was not launched cannot pass.

Shapes: hidden 256 (fixed by the kernels), V = 20, T = 3.  A forward pair is 17 rows (two tiles, the second partial) beside 5;
S = 58, 59, 60 are the two LDS boundaries where OVERLAP flips (58 / 59 under the automaton, 59 / 60 otherwise).  520 rows are
two launches (512 + 8); two passes of 400 rows do not fit one launch; a pass with an order goes out alone."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from probnmn import _hip
from probnmn.modules.seq2seq_base import pack_fragments

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filtered_inputs as fi  # noqa: E402
import test_decoder_length_order_gpu as lo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, V, T = 256, 20, 3
END = 3
MARK = -7
FILTER = fi.FILTERS[0]  # (0.7, 5, 1.0)
IDENTITY = (1.0, 0, 1.0)
MODES = ("forced", "sample", "greedy", "filtered")
SAMPLE = dict(forced=0, sample=1, greedy=2, filtered=1)
FWD_OUT = ("hs", "cs", "act", "ctx", "probs", "tokens")
BWD_OUT = ("dgates", "dctx", "dscore", "weights", "dh0")
# A small automaton over the V tokens: class 0 the even tokens, class 1 the odd ones; accepted: any string that holds an even
# token and, later, an odd one.  State 0 start, 1 an even token seen, 2 accepting; min_left = fewest tokens to state 2.
TOKEN_CLASS = (np.arange(V) % 2).astype(np.uint8)
NEXT_STATE = np.array([[1, 0], [1, 2], [2, 2]], np.uint8)
MIN_LEFT = np.array([2, 1, 0], np.uint8)
TABLES = (END, TOKEN_CLASS.ctypes.data, NEXT_STATE.ctypes.data, MIN_LEFT.ctypes.data, 3, 2)


def _stream():
    return _hip.stream_ptr(torch.device(DEV))


def _workspace(rows, backward):
    n = _hip.decoder_workspace_bytes(rows, backward)
    assert n > 0  # (the multi-CU kernels do take these passes)
    return torch.empty(n, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=None)
def _pass(B, Tn, S, seed, steps_seed=None):
    """The tensors of one pass in both directions, and its outputs.  ``steps_seed``: the rows get lengths in [1, Tn] and the
    pass its length order (the backward contract: dhs zero from a row's own steps on)."""
    d = {k: v.to(DEV) for k, v in fi.decoder_inputs(B, S, V, seed).items()}
    g = torch.Generator().manual_seed(seed + 1000)
    p = dict(d, B=B, T=Tn, S=S, seed=seed, w_c=pack_fragments(d["w_c"]), w_hh=pack_fragments(d["w_hh"]),
             w_c_t=pack_fragments(d["w_c"].t()), w_hh_t=pack_fragments(d["w_hh"].t()),
             in_tokens=torch.randint(0, V, (B, Tn), generator=g).to(DEV), dhs=torch.randn(B, Tn, H, generator=g).to(DEV), lists=None)
    if steps_seed is not None:
        steps = torch.as_tensor(np.random.Generator(np.random.Philox(steps_seed)).integers(1, Tn + 1, B), device=DEV)
        p["dhs"] = p["dhs"] * (torch.arange(Tn, device=DEV)[None, :] < steps[:, None])[:, :, None]
        p["lists"] = lo._order_of(steps, Tn)
    f = lambda *shape: torch.empty(*shape, device=DEV)  # noqa: E731
    p["out"] = dict(hs=f(B, Tn, H), cs=f(B, Tn, H), act=f(B, Tn, 4 * H), ctx=f(B, Tn, H), probs=f(B, Tn, S),
                    tokens=torch.empty(B, Tn, dtype=torch.long, device=DEV),
                    dgates=f(B, Tn, 4 * H), dctx=f(B, Tn, H), dscore=f(B, Tn, S), weights=f(B, Tn, S), dh0=f(B, H))
    return p


def _fwd_record(rec, p, mode, r0=0, r1=None):
    """Rows [r0, r1) of pass ``p`` in ``mode`` as a job record: every pointer and the row offset advanced by r0."""
    r1 = p["B"] if r1 is None else r1
    for k in ("enc", "mask", "h0"):
        rec[k] = p[k][r0:].data_ptr()
    for k in ("etable", "w_c", "w_hh"):
        rec[k] = p[k].data_ptr()
    for k in FWD_OUT[:5]:
        rec[k] = p["out"][k][r0:].data_ptr()
    if mode == "forced":
        rec["in_tokens"], rec["in_token_stride"] = p["in_tokens"][r0:].data_ptr(), p["in_tokens"].stride(0)
    else:
        rec["w_p"], rec["b_p"], rec["tokens"] = p["w_p"].data_ptr(), p["b_p"].data_ptr(), p["out"]["tokens"][r0:].data_ptr()
    rec["B"], rec["T"], rec["S"], rec["V"], rec["sample"] = r1 - r0, p["T"], p["S"], V, SAMPLE[mode]
    rec["pad_index"], rec["unk_index"], rec["start_index"] = fi.PAD, fi.UNK, fi.START
    rec["seed"], rec["row_offset"] = 2 ** 32 + 7 + p["seed"], 2 ** 32 - 5 + r0


def _bwd_record(rec, p):
    for k in ("dhs", "enc", "mask", "h0", "w_c_t", "w_hh_t"):
        rec[k] = p[k].data_ptr()
    for k in ("act", "cs", "hs", "probs") + BWD_OUT:
        rec[k] = p["out"][k].data_ptr()
    rec["B"], rec["T"], rec["S"] = p["B"], p["T"], p["S"]


def _group_lists(passes, ordered):
    """The two pointer lists of an ordered group call (entry i null for a pass without an order), or nulls."""
    if not ordered:
        return None, (None, None)
    arr = np.array([[0 if p["lists"] is None else p["lists"][i].data_ptr() for p in passes] for i in (0, 1)], np.uint64)
    return arr, (arr[0].ctypes.data, arr[1].ctypes.data)


def _marked(passes, names):
    for p in passes:
        for k in names:
            p["out"][k].fill_(MARK)


def _copies(passes, names):
    torch.cuda.synchronize()
    return [{k: p["out"][k].clone() for k in names} for p in passes]


def _forward(passes, modes, tables=fi.NO_TABLES, ordered=False, ranges=None, expect=0):
    """ONE forward call on ``passes`` (``ranges[i]``: the rows of pass i the call covers).  Nothing is marked here: the caller
    marks the outputs before the calls whose results it collects together."""
    n = len(passes)
    jobs = np.zeros(n, _hip.DECODER_FWD_JOB)
    for i, (p, mode) in enumerate(zip(passes, modes)):
        _fwd_record(jobs[i], p, mode, *(ranges[i] if ranges else ()))
    filters = None
    if "filtered" in modes:
        filters = np.array([(*(FILTER if m == "filtered" else IDENTITY), 0) for m in modes], _hip.SAMPLING_FILTER)
    ws = _workspace([int(j["B"]) for j in jobs], False)
    keep, lists = _group_lists(passes, ordered)
    head = (jobs.ctypes.data, None if filters is None else filters.ctypes.data, *tables, n, H)
    if ordered:
        rc = _hip.lib().pnmn_attn_lstm_fwd_group_ordered(*head, *lists, ws.data_ptr(), _stream())
    else:
        rc = _hip.lib().pnmn_attn_lstm_fwd_group(*head, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, modes)


def _backward(passes, ordered=False):
    n = len(passes)
    jobs = np.zeros(n, _hip.DECODER_BWD_JOB)
    for i, p in enumerate(passes):
        _bwd_record(jobs[i], p)
    ws = _workspace([p["B"] for p in passes], True)
    keep, lists = _group_lists(passes, ordered)
    if ordered:
        rc = _hip.lib().pnmn_attn_lstm_bwd_group_ordered(jobs.ctypes.data, n, H, *lists, ws.data_ptr(), _stream())
    else:
        rc = _hip.lib().pnmn_attn_lstm_bwd_group(jobs.ctypes.data, n, H, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc


def _assert_same(got, want, names, what):
    for i, (g, w) in enumerate(zip(got, want)):
        for k in names:
            assert torch.equal(g[k], w[k]), (what, "job %d" % i, k)


def _assert_written(copies, modes, what):
    """(the marker must not survive where a pass ran: hs of every job, the tokens of a free-running one)"""
    for c, mode in zip(copies, modes):
        assert not bool((c["hs"] == MARK).any()), (what, mode)
        assert (mode == "forced") == bool((c["tokens"] == MARK).all()) and (mode == "forced" or bool((c["tokens"] >= 0).all())), (what, mode)


def _group_against_members(passes, modes, tables=fi.NO_TABLES, ordered=False, what=None):
    """The group call against the lone calls of its members, the outputs marked before either."""
    _marked(passes, FWD_OUT)
    for p, mode in zip(passes, modes):
        _forward([p], [mode], tables, ordered=ordered and p["lists"] is not None)
    want = _copies(passes, FWD_OUT)
    _marked(passes, FWD_OUT)
    _forward(passes, modes, tables, ordered=ordered)
    got = _copies(passes, FWD_OUT)
    _assert_written(want, modes, what)
    _assert_same(got, want, FWD_OUT, what)


# ---- forward pairs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", MODES)
@pytest.mark.parametrize("m0", MODES)
@pytest.mark.parametrize("S", [58, 59, 60])
def test_forward_pair_is_its_two_passes(S, m0, m1):
    _group_against_members([_pass(17, T, S, seed=10 + S), _pass(5, T, S, seed=20 + S)], (m0, m1), what=(S, m0, m1))


CONSTRAINED_PAIRS = [(m0, m1) for m0 in MODES for m1 in MODES if (m0, m1) != ("forced", "forced")]
assert len(CONSTRAINED_PAIRS) == 15


@pytest.mark.parametrize("m0,m1", CONSTRAINED_PAIRS)
@pytest.mark.parametrize("S", [58, 59, 60])
def test_constrained_forward_pair_is_its_two_passes(S, m0, m1):
    """Under the automaton: every pair with a free-running pass, in both orders (the launcher puts the pair's passes in the
    order the kernels are compiled for).

    The six cases at S = 59 that hold a teacher-forced pass are where a launcher can get this wrong.  The pair counts the
    automaton's tables into its LDS and runs without OVERLAP (S <= 58); a lone teacher-forced pass stages no tables, and a
    launcher that let it take OVERLAP up to S = 59 ran the other compilation of the forward body, which agrees to round-off
    only, from the attention of step 0 on (measured on an MI355X on the 17-row pass of (forced, sample), T = 3: hs 6737 of
    13056 elements differ, max |d| 8.8e-7; ctx 6761, 3.5e-6; probs 1473 of 3009, 8.9e-7).  So every launch of a call with an
    automaton takes OVERLAP by the constrained rule."""
    _group_against_members([_pass(17, T, S, seed=10 + S), _pass(5, T, S, seed=20 + S)], (m0, m1), TABLES,
                           what=(S, m0, m1, "constrained"))


def test_the_automaton_constrains():
    """(so that the constrained cases above do run under it: it accepts every constrained row, cut at its first end token, and
    not every row of the unconstrained draw)"""
    def accepted(row):
        state = 0
        for v in row:
            if v == END:
                break
            state = int(NEXT_STATE[state][TOKEN_CLASS[v]])
        return state == 2

    p = _pass(17, T, 58, seed=68)
    _marked([p], FWD_OUT)
    _forward([p], ["sample"], TABLES)
    constrained = _copies([p], FWD_OUT)[0]["tokens"].tolist()
    _forward([p], ["sample"])
    free = _copies([p], FWD_OUT)[0]["tokens"].tolist()
    assert all(accepted(row) for row in constrained) and not all(accepted(row) for row in free)


# ---- a lone pass in row ranges ----------------------------------------------------------------------------------------
def _rows_per_launch():
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (cus // 64) * 128 if cus >= 64 else 0  # (all tiles x 8 members resident, one workgroup per CU)


@pytest.mark.parametrize("mode,tables", [(m, fi.NO_TABLES) for m in MODES] + [("sample", TABLES)])
def test_lone_forward_pass_runs_in_row_ranges(mode, tables):
    if _rows_per_launch() != 512:
        pytest.skip("a launch of this device takes %d rows, not 512: the ranges by hand would not be the launcher's" % _rows_per_launch())
    p = _pass(520, 2, 4, seed=7)
    _marked([p], FWD_OUT)
    _forward([p], [mode], tables)
    got = _copies([p], FWD_OUT)
    _marked([p], FWD_OUT)
    for r in ((0, 512), (512, 520)):
        _forward([p], [mode], tables, ranges=[r])
    want = _copies([p], FWD_OUT)
    _assert_written(want, [mode], mode)
    _assert_same(got, want, FWD_OUT, mode)


# ---- groups that fall back --------------------------------------------------------------------------------------------
def test_forward_group_that_does_not_fit_is_its_passes():
    assert 2 * 32 * 16 > _rows_per_launch()  # (two passes of 25 tiles, padded to 32 each)
    _group_against_members([_pass(400, 2, 4, seed=31), _pass(400, 2, 4, seed=32)], ("forced", "forced"), what="400 + 400")


@pytest.mark.parametrize("position", [0, 1])
def test_forward_group_with_an_ordered_pass_is_its_passes(position):
    passes = [_pass(40, T, 4, seed=41, steps_seed=5), _pass(17, T, 4, seed=42)]
    passes = passes[::-1] if position else passes
    _group_against_members(passes, ("forced", "forced"), ordered=True, what="ordered pass at %d" % position)


# ---- backward ---------------------------------------------------------------------------------------------------------
def _backward_group_against_members(passes, ordered=False):
    """(the forward passes first: the backward reads their cs, act, hs and probs -- the same tensors in both calls)"""
    _marked(passes, FWD_OUT)
    for p in passes:
        _forward([p], ["forced"], ordered=ordered and p["lists"] is not None)
    _marked(passes, BWD_OUT)
    for p in passes:
        _backward([p], ordered=ordered and p["lists"] is not None)
    want = _copies(passes, BWD_OUT)
    _marked(passes, BWD_OUT)
    _backward(passes, ordered=ordered)
    got = _copies(passes, BWD_OUT)
    for w in want:
        assert not bool((w["dh0"] == MARK).any()) and not bool((w["dgates"][:, 0] == MARK).any())
    _assert_same(got, want, BWD_OUT, [p["B"] for p in passes])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_backward_group_is_its_passes(n):
    _backward_group_against_members([_pass(B, T, 4, seed=50 + B) for B in (17, 5, 16)][:n])


def test_backward_group_that_does_not_fit_is_its_passes():
    _backward_group_against_members([_pass(400, 2, 4, seed=31), _pass(400, 2, 4, seed=32)])


@pytest.mark.parametrize("position", [0, 1])
def test_backward_group_with_an_ordered_pass_is_its_passes(position):
    passes = [_pass(40, T, 4, seed=41, steps_seed=5), _pass(17, T, 4, seed=42)]
    _backward_group_against_members(passes[::-1] if position else passes, ordered=True)


# ---- return codes -----------------------------------------------------------------------------------------------------
def test_return_codes():
    lib, einval = _hip.lib(), _hip.CONSTANTS["PNMN_EINVAL"]
    lo.test_rejected_jobs()  # (the rejected inputs of the ordered entry points)
    passes = [_pass(B, T, 4, seed=50 + B) for B in (17, 5, 16)]
    every = FWD_OUT + BWD_OUT
    ws = _workspace([17, 5, 16], True)
    jobs, bjobs = np.zeros(4, _hip.DECODER_FWD_JOB), np.zeros(4, _hip.DECODER_BWD_JOB)
    for i, p in enumerate(passes):
        _fwd_record(jobs[i], p, "sample")
        _bwd_record(bjobs[i], p)
    bjobs[3] = bjobs[2]
    _marked(passes, every)
    assert lib.pnmn_attn_lstm_fwd_group(jobs.ctypes.data, None, *fi.NO_TABLES, 3, H, ws.data_ptr(), _stream()) == einval
    assert lib.pnmn_attn_lstm_fwd_group(jobs.ctypes.data, None, *fi.NO_TABLES, 0, H, ws.data_ptr(), _stream()) == einval
    assert lib.pnmn_attn_lstm_bwd_group(bjobs.ctypes.data, 4, H, ws.data_ptr(), _stream()) == einval
    assert lib.pnmn_attn_lstm_bwd_group(bjobs.ctypes.data, 0, H, ws.data_ptr(), _stream()) == einval
    # a lone pass without rows: nothing to do, and nothing done (in either direction, under the automaton or not)
    jobs[0]["B"], bjobs[0]["B"] = 0, 0
    for tables in (fi.NO_TABLES, TABLES):
        assert lib.pnmn_attn_lstm_fwd_group(jobs.ctypes.data, None, *tables, 1, H, ws.data_ptr(), _stream()) == 0
    assert lib.pnmn_attn_lstm_bwd_group(bjobs.ctypes.data, 1, H, ws.data_ptr(), _stream()) == 0
    for c in _copies(passes, every):
        assert all(bool((t == MARK).all()) for t in c.values())
    # (the three-job helper of the filtered-sampling tests agrees: the entries with n <= 2 run, n = 3 is refused)
    sides = [((p["out"]["hs"], p["out"]["tokens"]), (None, p["out"]["cs"])) for p in passes]
    jobs[0]["B"] = 17
    for entry, rc, outputs in fi.decoder_entry_calls(jobs[:3], sides, ws, None):
        assert rc == (einval if entry == "group n=3" else 0), entry
        ran = {"fwd": 1, "group n=1": 1, "group n=2": 2, "group n=3": 0}[entry]
        for i in range(3):
            assert all(bool((t == MARK).all()) == (i >= ran) for t in outputs[3 * i:3 * i + 3]), (entry, i)
