"""pnmn_gemm_rows / pnmn_valid_rows (csrc/gemm.hip, csrc/seqglue.hip) through the C ABI: a weight gradient dy^T x of a padded
[rows][T][.] pass summed over the listed (row, step) pairs only, against the fp64 product over the listed rows.  In every
case the rows of BOTH operands that the list leaves out are NaN and the output must be finite: they are not read.  Bar:
test_gemm_gpu's ``_close`` at K = the number of listed rows."""
import numpy as np
import pytest
import torch

from probnmn import _hip
from test_gemm_gpu import _close, _desc, _ws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _pointers(values):
    return np.array(values, np.uint64)


def _valid_rows(segments):
    """One list of pnmn_valid_rows over `segments` = (last [rows] int32 or None, mask tokens [rows][>= T] int64 or None, pad, T),
    passes stored one behind the other; returns (list [capacity][2] int32, count [1] int32), both on the device."""
    n, rows = len(segments), [len(last if last is not None else mask) for last, mask, _, _ in segments]
    lst = torch.full((sum(r * T for r, (_, _, _, T) in zip(rows, segments)) + 1, 2), -77, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    last = _pointers([0 if s[0] is None else s[0].data_ptr() for s in segments])
    mask = _pointers([0 if s[1] is None else s[1].data_ptr() for s in segments])
    stride = np.array([0 if s[1] is None else s[1].stride(0) for s in segments], np.int64)
    pad, T, nrows = (np.array(x, np.int32) for x in ([s[2] for s in segments], [s[3] for s in segments], rows))
    lists, counts = _pointers([lst.data_ptr()] * n), _pointers([count.data_ptr()] * n)
    _hip.check(_hip.lib().pnmn_valid_rows(last.ctypes.data, mask.ctypes.data, stride.ctypes.data, pad.ctypes.data, nrows.ctypes.data,
                                          T.ctypes.data, lists.ctypes.data, counts.ctypes.data, n, _hip.stream_ptr(torch.device(DEV))),
               "valid_rows")
    torch.cuda.synchronize()
    return lst, count


def _list_of_steps(steps, T):
    """The list for sequences of `steps` [rows] (>= 1 each) of T steps, built by the kernel under test from last = steps - 1."""
    return _valid_rows([(torch.as_tensor(steps, dtype=torch.int32, device=DEV) - 1, None, 0, T)])


def _empty_list(rows, T):
    """count == 0: a decoder pass whose mask tokens are all padding."""
    return _valid_rows([(None, torch.zeros(rows, T, dtype=torch.long, device=DEV), 0, T)])


def _run_rows(descs, lists, max_workgroups=0):
    rec = np.concatenate(descs)
    rows = _pointers([0 if l is None else l[0].data_ptr() for l in lists])
    count = _pointers([0 if l is None else l[1].data_ptr() for l in lists])
    rc = _hip.lib().pnmn_gemm_rows(rec.ctypes.data, len(rec), rows.ctypes.data, count.ctypes.data, max_workgroups,
                                   _hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc


class _Case:
    """dy [rows T][M], x [rows T][N] with NaN wherever the list (and the shift) leaves a row unread, and the fp64 product."""

    def __init__(self, rows, T, M, N, steps, seed, shift=False, h0=False):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.rows, self.T, self.M, self.N, self.K = rows, T, M, N, rows * T
        steps = torch.as_tensor(steps, device=DEV)
        t = torch.arange(T, device=DEV)
        self.valid = (t[None, :] < steps[:, None])                                   # [rows][T]
        self.dy = torch.randn(rows, T, M, device=DEV, generator=g)
        self.x = torch.randn(rows, T, N, device=DEV, generator=g)
        self.h0 = torch.randn(rows, N, device=DEV, generator=g) if h0 else None
        self.dy[~self.valid] = NAN
        # the shifted operand of a listed (b, t) is x[b][t - 1]: x is read at t <= steps - 2 only
        self.x[~(t[None, :] < steps[:, None] - 1) if shift else ~self.valid] = NAN
        xs = self.x.double()
        if shift:
            first = self.h0.double() if h0 else torch.zeros(rows, N, dtype=torch.float64, device=DEV)
            xs = torch.cat((first[:, None], xs[:, :-1]), 1)
        keep = self.valid.reshape(-1)
        self.listed = int(keep.sum())
        self.dy_kept = self.dy.double().reshape(self.K, M)[keep]
        self.want = self.dy_kept.t() @ xs.reshape(self.K, N)[keep]
        self.shift = shift

    def desc(self, C, split=1, ws=None, flags=0, colsum=None, colsum2=None):
        d = _desc(self.dy.view(self.K, self.M), self.x.view(self.K, self.N), C, self.M, self.N, self.K, flags=_hip.GEMM_A_T | flags,
                  split=split, ws=ws, shift_t=self.T if self.shift else 0, h0=self.h0)
        if colsum is not None:
            d["colsum"], d["colsum2"] = colsum.data_ptr(), colsum2.data_ptr()
        return d

    def check(self, C):
        assert bool(torch.isfinite(C).all())
        _close(C, self.want, max(self.listed, 1))


def _mixed(rows, T, seed):
    return torch.randint(1, T + 1, (rows,), generator=torch.Generator().manual_seed(seed)).tolist()


def test_single_ragged_k_tile():
    steps = [3, 7, 1, 5, 2]
    case = _Case(5, 7, 44, 256, steps, 1)
    C = torch.full((44, 256), NAN, device=DEV)
    assert _run_rows([case.desc(C)], [_list_of_steps(steps, 7)]) == 0
    case.check(C)


@pytest.mark.parametrize("steps,split", [("1..13", 1), ("1..13", 3), ("ones", 3)])
def test_ragged_shapes_and_empty_last_chunk(steps, split):
    rows, T, M, N = 40, 13, 160, 200
    steps = [1] * rows if steps == "ones" else [1 + b % 13 for b in range(rows)]  # ("ones": 40 rows = 2 k tiles for 3 chunks)
    case = _Case(rows, T, M, N, steps, 2 + split)
    C = torch.full((M, N), NAN, device=DEV)
    ws = _ws(M, N, split)
    ws.view(torch.float32)[: ws.numel() // 4].fill_(NAN)  # (nothing may depend on what the workspace held)
    assert _run_rows([case.desc(C, split=split, ws=ws if split > 1 else None)], [_list_of_steps(steps, T)]) == 0
    case.check(C)


@pytest.mark.parametrize("what", ["shift_h0", "shift_zero", "colsum", "accumulate"])
def test_interior_tiles(what):
    rows, T, M, N, split = 64, 46, 1024, 256, 4
    steps = _mixed(rows, T, 7)
    shift = what.startswith("shift")
    case = _Case(rows, T, M, N, steps, 11, shift=shift, h0=what == "shift_h0")
    C = torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    before = C.double().clone()
    cs, cs2 = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
    ws = _ws(M, N, split)
    d = case.desc(C, split=split, ws=ws, flags=_hip.GEMM_ACC if what == "accumulate" else 0,
                  colsum=cs if what == "colsum" else None, colsum2=cs2)
    assert _run_rows([d], [_list_of_steps(steps, T)]) == 0
    if what == "accumulate":
        case.want = case.want + before
    case.check(C)
    if what == "colsum":
        _close(cs, case.dy_kept.sum(0), case.listed)
        assert torch.equal(cs, cs2)


@pytest.mark.parametrize("split", [1, 4])
def test_identity_list_equals_pnmn_gemm(split):
    rows, T, M, N = 24, 11, 300, 256
    case = _Case(rows, T, M, N, [T] * rows, 5, shift=True, h0=True)
    outs = []
    for listed in (True, False):
        C = torch.full((M, N), NAN, device=DEV)
        ws = _ws(M, N, split)
        d = case.desc(C, split=split, ws=ws if split > 1 else None)
        if listed:
            assert _run_rows([d], [_list_of_steps([T] * rows, T)]) == 0
        else:
            _hip.check(_hip.lib().pnmn_gemm(d.ctypes.data, 1, _hip.stream_ptr(torch.device(DEV))), "gemm")
            torch.cuda.synchronize()
        outs.append(C)
    assert torch.equal(outs[0], outs[1])
    case.check(outs[0])


@pytest.mark.parametrize("accumulate", [False, True])
def test_count_zero(accumulate):
    rows, T, M, N, split = 9, 5, 130, 140, 2
    lst = _empty_list(rows, T)
    assert int(lst[1]) == 0
    dy, x = torch.full((rows * T, M), NAN, device=DEV), torch.full((rows * T, N), NAN, device=DEV)
    for sp in (1, split):
        C = torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(sp))
        before = C.clone()
        ws = _ws(M, N, sp)
        ws.view(torch.float32)[: ws.numel() // 4].fill_(NAN)
        d = _desc(dy, x, C, M, N, rows * T, flags=_hip.GEMM_A_T | (_hip.GEMM_ACC if accumulate else 0), split=sp, ws=ws if sp > 1 else None)
        assert _run_rows([d], [lst]) == 0
        assert torch.equal(C, before if accumulate else torch.zeros_like(C))


def test_three_problems_three_counts_one_without_a_list():
    cases = [(_Case(30, 9, 200, 256, _mixed(30, 9, 1), 21), True, 2), (_Case(12, 20, 128, 130, [20] * 12, 22), False, 1),
             (_Case(50, 6, 384, 128, _mixed(50, 6, 3), 23, shift=True), True, 3)]
    descs, lists, outs, keep = [], [], [], []
    for case, listed, split in cases:
        C = torch.full((case.M, case.N), NAN, device=DEV)
        ws = _ws(case.M, case.N, split)
        keep.append(ws)
        descs.append(case.desc(C, split=split, ws=ws if split > 1 else None))
        steps = case.valid.sum(1).tolist()
        lists.append(_list_of_steps(steps, case.T) if listed else None)
        outs.append(C)
    assert len({int(l[1]) for l in lists if l is not None}) == 2
    assert _run_rows(descs, lists) == 0
    for (case, _, _), C in zip(cases, outs):
        case.check(C)


@pytest.mark.parametrize("flags", [0, "b_t", "a_t_b_t"])
def test_a_list_needs_both_operands_k_major(flags):
    flags = {0: 0, "b_t": _hip.GEMM_B_T, "a_t_b_t": _hip.GEMM_A_T | _hip.GEMM_B_T}[flags]
    M = N = K = 64
    A, B, C = (torch.zeros(64, 64, device=DEV) for _ in range(3))
    assert _run_rows([_desc(A, B, C, M, N, K, flags=flags)], [_list_of_steps([8] * 8, 8)]) == _hip.ESHAPE
    assert _run_rows([_desc(A, B, C, M, N, K, flags=flags)], [None]) == 0  # (without a list: pnmn_gemm_cus)


def _numpy_list(segments):
    """The specification of pnmn_valid_rows' list."""
    out, row0, seq0 = [], 0, 0
    for steps, T in segments:
        for b, s in enumerate(steps):
            out += [(row0 + b * T + t, row0 + b * T + t - 1 if t else ~(seq0 + b)) for t in range(s)]
        row0, seq0 = row0 + len(steps) * T, seq0 + len(steps)
    return np.array(out, np.int32).reshape(-1, 2)


def test_valid_rows_from_last_clamps_as_length_order_does():
    T = 9
    last = torch.tensor([-1, 0, 3, 8, 9, 40, -5, 7] * 150 + [2, 2, 8], dtype=torch.int32)  # (1203 rows: two rounds of the scan)
    lst, count = _valid_rows([(last.to(DEV), None, 0, T)])
    want = _numpy_list([(np.clip(last.numpy() + 1, 1, T).tolist(), T)])
    assert int(count) == len(want)
    got = lst.cpu().numpy()
    assert np.array_equal(got[: len(want)], want) and (np.diff(got[: len(want), 0]) > 0).all()
    assert (got[len(want):] == -77).all()  # (nothing behind the count is written)


def test_valid_rows_of_two_decoder_passes_in_one_list():
    g = torch.Generator().manual_seed(9)
    pad, segs, spec = 0, [], []
    for rows, T, width in ((70, 26, 26), (33, 13, 14)):
        tokens = torch.randint(1, 40, (rows, width), generator=g)
        steps = torch.randint(0, T + 1, (rows,), generator=g)
        tokens[torch.arange(width)[None, :] >= steps[:, None]] = pad
        inner = steps >= 3
        tokens[inner, 1] = pad  # (a pad inside the weighted steps drops nothing behind it)
        if width > T:
            tokens[:, T:] = 5   # (beyond the pass's T steps: another view's tokens, not read)
        segs.append((None, tokens.to(DEV), pad, T))
        spec.append((steps.tolist(), T))
    lst, count = _valid_rows(segs)
    want = _numpy_list(spec)
    assert int(count) == len(want)
    assert np.array_equal(lst.cpu().numpy()[: len(want)], want)
