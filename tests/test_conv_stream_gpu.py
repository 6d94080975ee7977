"""The streamed convolution, forward and data-gradient (csrc/conv_stream.h, launched from csrc/conv_nhwc.hip), across its
splits, bodies, geometries, prologues, epilogues and launch plans -- through the C ABI (pnmn_conv_nhwc_cus, and
pnmn_conv_nhwc once per group) against the float64 reference of tests/helpers/conv_reference.py computed on the device
with torch (independent of the library; tests/test_conv_reference.py holds it against F.conv2d and float64 autograd,
and holds the restated planner against the compiled csrc/conv_plan.h).

EXACT cases.  Small integers stored as float32 (x, w, mb_feats in [-2, 2]; masks and mb_attn in {0, 1, 2}; gates in
{-1, -0.0, 0, 1}; bias and prefills in [-3, 3]): every product, every partial sum in any order and every atomic add is
exact in float32 as long as the largest reachable magnitude stays below 2^24, which conv_reference.exact_ok asserts per
launch (the 128-channel mb_dattn sum and all items adding into one map included).  The comparison is torch.equal, so a
tap shifted by the wrong dilation, a band's halo row dropped, a stage contracted twice, a mask taken from the neighbouring
piece, an m-tile skipped that a tap does reach, or a missed `+=` shows as a whole number; the failure message names the
items, bands, pixels and channels that differ.  Every written map sits between sentinel guards; where out_stride is wider
than the output channels the columns beside them must keep their sentinels; input columns the shape does not read
(in_stride wider than the channels) hold NaN, and `out` is NaN before a plain store.

  (a) a dozen items mixing dilations 1, 2, 4, 8, masks, bias / no bias and three weights, under every forced split, as
      forward (relu off, and on with wide strides), data gradient (gate on every item), ACCUMULATE onto a prefill and
      ACCUMULATE | ATOMIC with two items per map; the 1x1 under 1, 2, 4, 8 and under 6, 14, 26 (which fall back);
  (b) the MASKBWD (sole / three items per map / no attention) and DATTN epilogues under every forced split, dilation 8
      in each, so that KIND 1 meets them at split 1 and 2;
  (c) the stem (8 chunks, in_stride 1024), two sources, the classifier (8 and 4 output blocks) and a 3x3 with two output
      blocks, under the planner and under forced splits 1 and 26 (8 for the 1x1 shapes);
  (d) the planner's own 1-, 2- and 3-segment plans at cus in {8, 16, 24, 40} and 0, items sorted by weight or not:
      segments with holes, and at a grid of 8 workgroups walks of seven and more units whose band, dilation and slot
      count change -- the LDS ring, the row-table refill and the end-of-unit hand-over;
  (e) gated and ungated items taking turns (test_mixed_slots, below).

Reached, per map size (asserted from the restated planner in tests/test_conv_reference.py::test_coverage; every test
prints its plan and (split, KIND) set):
  14x14: (split, KIND 0) for split 1, 2, 4, 6, 8, 14, 26; (1, KIND 1), (2, KIND 1); (1 | 2 | 4 | 8, KIND 2)
  28x28: (split, KIND 0) for split 1, 2, 4, 6, 8, 14, 26; (1 | 2 | 4 | 8, KIND 2).  KIND 1 does not exist at 28x28
         (conv_stream takes it for whole 14x14 maps only), so "splits 1 and 2 with KIND 1" holds for 14x14 alone.
Segment plans of group (d), as splits over units: 14x14: (1,2,6)/(8,4,1), (1,2,4)/(8,4,2), (2,4,14)/(8,4,1),
(1,4,26)/(40,10,3), (1,2,14)/(16,8,1), (1,2,8)/(48,4,1), (2,4,14)/(12,6,1), (26)/3, (14)/12, (8)/22, (6)/40, (4)/50;
28x28: (1,2)/(8,4), (1,2)/(48,4), (1,2,4)/(16,8,4), (1,2,6)/(24,12,4), (1,4,14)/(40,10,2), (1,2,8)/(80,20,4), (26)/4,
(14)/12, (8)/20, (6)/40, (4)/44, (2)/88, (2,4,26)/(128,64,4), (1)/212; and the 1x1 plans (1,8), (1,4), (1,2), (4), (2), (1).

ROUND-OFF cases.  The data of tests/test_hip_kernels.py, one launch per path.  Per tensor err = max|got - ref64| /
max|ref64|; the bar is 4 * err32 + 2 * 2^-24 with err32 the same figure of the reference run in float32 on the CPU (both
are float32 sums of the same products in another order).  For the non-atomic tensors every forced split must be
torch.equal to split 1; the atomic ones (mb_dattn: 8 partial sums per pixel in free order; mb_dfeats with several
writers) are held to their bar under every split.

The 3x3 launches exceed the factor 4 on `out` / mb_dfeats without a defect (4.1 to 6.5 err32 at K = 1152, 12.6 and 15.7 at
the stem's K = 9216; their exact twins pass, and every split gives the same bits): an output is ONE float32 accumulator
over K / 4 MFMA steps, each rounding a partial sum that has grown to the size of the result, where the CPU sums in
blocks.  So ALL launches with ntaps = 9 -- the rule is the length of the chain, not the measurement: 3x3 one chunk, stem,
dgrad with gate, MASKBWD sole / shared, DATTN -- and no 1x1 launch (K = 128 or 256: 0.97 to 1.74 err32) carry one more
term on `out` and mb_dfeats (never on mb_dattn): six standard deviations of the round-off of that chain, computed from
the inputs and the float64 reference's partial sums in the kernel's order of additions (conv_reference.chain_sigma: one
rounding of variance ulp(S)^2 / 12 per non-zero product, an upper count).  Six because a tensor has up to 1.2e6 entries.
tests/test_conv_reference.py runs such a chain in float32 with numpy and finds it at one sigma of this model.

Measured err / err32 under the planner (MI355X, the kernels of commit cd8ddd0; `out` or mb_dfeats, then mb_dattn), and in
brackets the bar of the first tensor in units of err32 where the chain term is in it:

    launch                                   14x14                  28x28
    3x3 one chunk, 12 items                   4.10       (19.1)      4.36       (20.8)
    stem, K = 9216, 3 items                  15.65       (45.6)     12.64       (42.2)
    two-source 1x1, 5 items                   1.16                   1.74
    classifier (cout 1024), 3 items           1.15                   0.97
    dgrad with gate, 12 items                 5.80       (20.9)      4.56       (19.4)
    MASKBWD sole, 6 items                     4.65, 2.13 (17.2)      6.49, 2.42 (20.2)
    MASKBWD, 3 items per map                  3.96, 3.69 (17.0)      2.74, 2.30 (15.2)
    DATTN, 6 items                            4.82, 2.14 (17.6)      5.07, 2.76 (19.1)

(mb_dattn moves from run to run in its last bits: 2.14 and 2.24 on two runs of the same launch.)

A bad pnmn_conv_force_split value returns PNMN_EINVAL; that the previous split is kept cannot be observed through the ABI
(the results do not depend on the split, and there is no getter), so it is read off csrc/conv_nhwc.hip: the check
returns before the assignment.

SEEDED DEFECTS.  Three builds of the library, each with one change of which in-bounds value is used (no address, barrier,
wait count or loop bound touched), each run once against this file, the convolution tests of tests/test_hip_kernels.py
and tests/test_nmn_gpu.py::test_conv_splits_give_bit_identical_activations:
  1. KIND 1 contracts the FIRST half's m-tiles for the taps of row -8 instead of the second's (I1 for I2 on taps 0..2, both
     weight-set variants).  tests/test_hip_kernels.py PASSES it (its dilation-8 launches go out at split 26 / 14: KIND 0).
     The network test fails (4 of its cases).  Here 34 cases fail, all at 14x14 and only where a (1 | 2, KIND 1) unit
     is reached: every group (a) and (b) launch under forced split 1 and 2, stem and cout2 under split 1, the seven
     planner launches whose plan has a split-1 or -2 segment, test_mixed_slots at cus = 8, and the six 14x14 3x3
     round-off launches.
  2. The ACCUMULATE epilogue drops `old[j]`.  The network test PASSES it; tests/test_hip_kernels.py fails (the dgrad test's
     second, accumulating call, 8 cases).  Here the 14 "3x3 acc" cases of group (a) fail, every split at both sizes.
  3. fixup() multiplies by the mask values of the loader wave's NEXT piece.  The network test PASSES it (a defect common to
     every split); tests/test_hip_kernels.py fails (30 cases).  Here 181 cases fail: every masked launch of groups (a),
     (c), (d) and (e) and the masked round-off launches; group (b), whose items carry no mask, passes.

Time: the 269 tests of this file take 5.9 s on an MI355X (references, uploads and the CPU float32 yardsticks included).
"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64          # floats in front of and behind every written map
SENTINEL = 4242.0
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    from probnmn import _hip

    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a MI355X"
    return _hip


def dev():
    return torch.device("cuda:0")


class Uploaded:
    """The pools of a launch in device memory (inputs padded to in_stride with NaN) and its item records without outputs."""

    def __init__(self, L):
        nan = float("nan")
        d = dev()
        self.L = L
        cx = L.x_pool.shape[2]
        assert cx <= L.in_stride and L.cin <= L.in_stride or L.two_sources
        self.x = torch.full((L.x_pool.shape[0], L.HW, L.in_stride), nan, device=d)
        self.x[:, :, :cx] = L.x_pool.to(d)
        self.x2 = None
        if L.two_sources:
            assert not any(it.gate >= 0 for it in L.items), "a gate map has in_stride columns for every chunk: not with a second source"
            self.x2 = torch.full((L.x2_pool.shape[0], L.HW, L.in_stride), nan, device=d)
            self.x2[:, :, :R.CB] = L.x2_pool.to(d)
        self.g = None
        if any(it.gate >= 0 for it in L.items):
            self.g = torch.full((L.g_pool.shape[0], L.HW, L.in_stride), nan, device=d)
            self.g[:, :, :L.cin] = L.g_pool.to(d)
        self.m, self.w, self.b, self.f = (t.to(d).contiguous() for t in (L.m_pool, L.w_pool, L.b_pool, L.f_pool))


def guarded(pre, row, width):
    """[n][GUARD + HW * row + GUARD] of sentinels with `pre` [n][HW][width] in the first `width` columns of every row."""
    n, HW = pre.shape[0], pre.shape[1]
    big = torch.full((max(n, 1), 2 * GUARD + HW * row), SENTINEL, device=dev())
    if n:
        body = torch.full((n, HW, row), SENTINEL, device=dev())
        body[:, :, :width] = pre.to(dev()).reshape(n, HW, width)
        big[:, GUARD:GUARD + HW * row] = body.reshape(n, HW * row)
    return big


def launch(hip, up, *, cus=0, forced=0, entry="cus"):
    """One call.  Returns {"out", "dfeats", "dattn"} as the call left them (guards and side columns checked)."""
    L, HW = up.L, up.L.HW
    out = guarded(L.out_pre, L.out_stride, L.cout)
    df = guarded(L.df_pre, R.CB, R.CB)
    da = guarded(L.da_pre.unsqueeze(2), 1, 1)
    p = lambda t, i: t[i].data_ptr()  # noqa: E731
    recs = np.zeros(len(L.items), hip.CONV_ITEM)
    for i, it in enumerate(L.items):
        r = recs[i]
        r["in"] = p(up.x, it.x)
        r["in2"] = p(up.x2, it.x2) if it.x2 >= 0 else 0
        r["mask"] = p(up.m, it.mask) if it.mask >= 0 else 0
        r["gate"] = p(up.g, it.gate) if it.gate >= 0 else 0
        r["weight"] = p(up.w, it.w)
        r["bias"] = p(up.b, it.w) if it.bias else 0
        r["out"] = p(out, it.out) + 4 * GUARD if it.out >= 0 else 0
        r["dilation"], r["flags"] = it.dil, it.flags
        if it.flags & (R.MASKBWD | R.DATTN):
            r["mb_feats"] = p(up.f, it.feats)
            r["mb_attn"] = p(up.m, it.attn) if it.attn >= 0 else 0
            r["mb_dfeats"] = p(df, it.dfeats) + 4 * GUARD if it.dfeats >= 0 else 0
            r["mb_dattn"] = p(da, it.dattn) + 4 * GUARD if it.dattn >= 0 else 0
    ibuf = hip.to_device(recs, dev())
    args = (ibuf.data_ptr(), len(recs), L.H, L.W, L.cin_chunks, L.ntaps, L.in_stride, L.out_stride, L.cout_blocks, L.relu)
    lib = hip.lib()
    try:
        assert lib.pnmn_conv_force_split(forced) == 0
        if entry == "cus":
            hip.check(lib.pnmn_conv_nhwc_cus(*args, cus, hip.stream_ptr(dev())), "conv (cus = %d, split %d)" % (cus, forced))
        else:
            assert cus == 0
            hip.check(lib.pnmn_conv_nhwc(*args, hip.stream_ptr(dev())), "conv")
        torch.cuda.synchronize()
    except RuntimeError as e:  # (a HIP error is sticky: nothing after it on this device means anything)
        pytest.exit("the device reported an error in %s: %s" % (L.note, e), returncode=3)
    finally:
        lib.pnmn_conv_force_split(0)
    got = {}
    for what, big, n, row, width in (("out", out, L.count("out"), L.out_stride, L.cout), ("dfeats", df, L.count("dfeats"), R.CB, R.CB),
                                     ("dattn", da, L.count("dattn"), 1, 1)):
        assert bool((big[:, :GUARD] == SENTINEL).all()) and bool((big[:, GUARD + HW * row:] == SENTINEL).all()), \
            "floats in front of or behind a map of %s were written" % what
        body = big[:n, GUARD:GUARD + HW * row].reshape(n, HW, row)
        assert bool((body[:, :, width:] == SENTINEL).all()), "columns beside the output channels of %s were written" % what
        got[what] = body[:, :, :width].reshape(L.da_pre.shape if what == "dattn" else (n, HW, width)).clone()
    return got


_LAUNCH, _REF = {}, {}


def launch_of(case, kind="int"):
    """The launch of a case with its data, uploaded once per (name, map size, data kind); its float64 reference, on the device."""
    key = (case.name, case.H, kind)
    if key not in _LAUNCH:
        L = case.make()
        R.fill(L, kind, seed=zlib.crc32(repr(key).encode()) % 10007, dgrad=any(it.gate >= 0 for it in L.items))
        if kind == "int":
            R.exact_ok(L)
        _LAUNCH[key] = Uploaded(L)
        _REF[key] = R.reference(L, device=dev())
    return _LAUNCH[key], _REF[key]


def describe(case):
    f = R.facts_of(case)
    p = f["plan"]
    return "%s: plan %s over %s units, grid %d, (split, KIND) %s, longest walk %d" % (
        case.id, p.splits, p.counts, f["grid"], sorted(f["kinds"]), f["longest_walk"])


def assert_exact(L, what, got, ref, where):
    if torch.equal(got.double(), ref):
        return
    wrong = torch.nan_to_num(got.double() - ref, nan=1e30) != 0          # [maps][HW][channels]
    maps = torch.nonzero(wrong.reshape(wrong.shape[0], -1).any(1)).flatten().tolist()
    m0 = maps[0]
    w0 = wrong[m0].reshape(L.HW, -1)
    px = torch.nonzero(w0.any(1)).flatten().tolist()
    ch = torch.nonzero(w0.any(0)).flatten().tolist()
    d0 = (got[m0].double() - ref[m0]).reshape(L.HW, -1)[w0]
    vals = torch.unique(d0[:4096]).tolist()[:12]
    writers = [(i, it.dil, it.flags) for i, it in enumerate(L.items) if getattr(it, what) == m0]
    raise AssertionError(
        "%s differs (%s): %d entries in maps %s; map %d (items (index, dilation, flags) %s): %d pixels, image rows %s, first pixels %s, "
        "%d channels, first %s; differences %s (reference magnitude %g)"
        % (what, where, int(wrong.sum()), maps[:12], m0, writers, len(px), sorted({q // L.W for q in px}), px[:12], len(ch), ch[:16], vals,
           float(ref.abs().max())))


def run_exact(hip, case):
    up, ref = launch_of(case)
    print("\n[plan] " + describe(case))
    got = launch(hip, up, cus=case.cus, forced=case.forced, entry=case.entry)
    for what in ("out", "dfeats", "dattn"):
        assert_exact(up.L, what, got[what], ref[what], case.id)


def group(g):
    cs = [c for c in R.cases() if c.group == g]
    return pytest.mark.parametrize("case", cs, ids=[c.id for c in cs])


@group("a")
def test_exact_mixed_dozen_under_every_split(hip, case):
    run_exact(hip, case)


@group("b")
def test_exact_epilogues_under_every_split(hip, case):
    """MASKBWD with MB_SOLE, with three items adding into one mb_dfeats map, with mb_attn == NULL; DATTN with and without
    mb_attn (mb_dattn stays exactly zero where there is no attention -- its prefill is zero and the comparison is exact --
    and dx is fully written: `out` is NaN before the call)."""
    run_exact(hip, case)


@group("c")
def test_exact_shapes(hip, case):
    run_exact(hip, case)


@group("d")
def test_exact_planner_and_walker(hip, case):
    run_exact(hip, case)


@group("e")
def test_mixed_slots(hip, case):
    """Gated items (two ring slots per stage: the stage and, behind it, its gate map) and ungated ones (one slot) take turns
    in one launch.  Why loader()'s accounting holds across the change, read from csrc/conv_stream.h:
      * `issued`, `freed` and `cstart` count SLOTS, not stages, and the producer, the consumer cursor and the contraction
        waves (run_unit's own cstart += slots) advance by the same Walker::slots of the same unit sequence, so all three
        name slot (count % RING) for a stage whatever mix came before;
      * top_up issues a stage only while issued - freed + P.slots <= RING, and `freed` is the start of the stage handed over
        LAST (freed = cstart before cstart += C.slots): the slots of the stage being contracted stay counted as in use, so
        a two-slot stage never lands on a slot still being read, with RING = 4 (28x28) as with 6;
      * prepare() waits until at most `younger` slots' worth of this wave's loads are outstanding, younger = issued -
        (cstart + C.slots) counting slots, each of which is exactly NP2 loads of this wave whether it holds a stage or a
        gate map (issue_rows issues the same pieces for both); loads complete in order, so everything up to the end of the
        consumer's stage -- its gate map included -- has landed.  younger can reach RING - 1 = 5 at 14x14, where the
        wait is capped at 3 * NP2: a stricter wait than needed, never a weaker one;
      * fixup reads the gate from slot (cstart + 1) % RING, the slot top_up issued it to ((issued + 1) % RING at a time
        when issued == that stage's cstart).
    At cus = 8 a workgroup walks gated and ungated items back to back (asserted from the restated walk)."""
    run_exact(hip, case)


# ---------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------
def small(hip, H=14, ntaps=9):
    c = R.Case("args", "args %d" % ntaps, H, lambda: R.shape_launch(H, "cout2") if ntaps == 9 else R.shape_launch(H, "classifier4"))
    return launch_of(c)[0]


def raw_call(hip, up, *, n=None, H=None, W=None, ntaps=None, in_stride=None, out_stride=None):
    """The entry point with one argument replaced; outputs are sentinel-filled and returned with the code."""
    L = up.L
    out = torch.full((L.count("out"), L.HW * L.out_stride + 2 * GUARD), SENTINEL, device=dev())
    recs = np.zeros(len(L.items), hip.CONV_ITEM)
    for i, it in enumerate(L.items):
        recs[i]["in"], recs[i]["weight"], recs[i]["out"], recs[i]["dilation"] = up.x[it.x].data_ptr(), up.w[it.w].data_ptr(), out[i].data_ptr() + 4 * GUARD, 1
    ibuf = hip.to_device(recs, dev())
    pick = lambda v, d: d if v is None else v  # noqa: E731
    code = hip.lib().pnmn_conv_nhwc_cus(ibuf.data_ptr(), pick(n, len(recs)), pick(H, L.H), pick(W, L.W), L.cin_chunks, pick(ntaps, L.ntaps),
                                        pick(in_stride, L.in_stride), pick(out_stride, L.out_stride), L.cout_blocks, 0, 0, hip.stream_ptr(dev()))
    torch.cuda.synchronize()
    return code, out


def test_arguments(hip):
    up = small(hip)
    for bad in (dict(ntaps=3), dict(ntaps=0), dict(ntaps=8), dict(in_stride=130), dict(out_stride=258), dict(in_stride=129)):
        code, out = raw_call(hip, up, **bad)
        assert code == hip.EINVAL, bad
        assert bool((out == SENTINEL).all()), bad
    for bad in (dict(H=7, W=7), dict(H=14, W=28), dict(H=28, W=14)):
        code, out = raw_call(hip, up, **bad)
        assert code == hip.ESHAPE, bad
        assert bool((out == SENTINEL).all()), bad
    code, out = raw_call(hip, up, n=0)
    assert code == 0 and bool((out == SENTINEL).all())


def test_force_split_values(hip):
    lib = hip.lib()
    try:
        for s in (0, 1, 2, 4, 6, 8, 14, 26):
            assert lib.pnmn_conv_force_split(s) == 0
        assert lib.pnmn_conv_force_split(4) == 0
        for bad in (3, 5, 7, 16, 13, 27, -1, 128):
            assert lib.pnmn_conv_force_split(bad) == hip.EINVAL
    finally:
        assert lib.pnmn_conv_force_split(0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# round-off
# ---------------------------------------------------------------------------------------------------------------------
ROUNDOFF = {
    "3x3 one chunk": lambda H: R.mix_launch(H, 9, "fwd_relu"),
    "stem K=9216": lambda H: R.shape_launch(H, "stem"),
    "two-source 1x1": lambda H: R.shape_launch(H, "two_sources_mask"),
    "classifier": lambda H: R.shape_launch(H, "classifier8"),
    "dgrad with gate": lambda H: R.mix_launch(H, 9, "dgrad"),
    "MASKBWD sole": lambda H: R.epilogue_launch(H, "sole"),
    "MASKBWD shared": lambda H: R.epilogue_launch(H, "shared3"),
    "DATTN": lambda H: R.epilogue_launch(H, "dattn"),
}
ATOMIC_TENSORS = {"MASKBWD sole": {"dattn"}, "MASKBWD shared": {"dfeats", "dattn"}, "DATTN": {"dattn"}}
_ERR32 = {}


def rel_err(got, ref):
    return float((got.double().cpu() - ref.double().cpu()).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("H", [14, 28], ids=["14x14", "28x28"])
@pytest.mark.parametrize("name", sorted(ROUNDOFF))
def test_roundoff_and_bit_equality_across_splits(hip, H, name):
    """err <= 4 err32 + 2 * 2^-24 per tensor under the planner; then every forced split: the non-atomic tensors torch.equal to
    split 1 (a wave contracts all input channels of its outputs in one order, whatever the split), the atomic ones (mb_dattn:
    8 partial sums per pixel; mb_dfeats with several writers) under the same bar."""
    case = R.Case("r", "roundoff " + name, H, lambda: ROUNDOFF[name](H))
    up, ref = launch_of(case, "normal")
    L = up.L
    r32 = R.reference(L, device="cpu", dtype=torch.float32)
    tensors = [k for k in ("out", "dfeats", "dattn") if ref[k].numel()]
    tensors = [k for k in tensors if k != "dattn" or any(it.attn >= 0 for it in L.items)]
    err32 = {k: rel_err(r32[k], ref[k]) for k in tensors}
    bar = {k: 4 * err32[k] + 2 * U32 for k in tensors}
    if L.ntaps == 9:  # (the chained launches: see the module's docstring)
        sigma = R.chain_sigma(L, device=dev())
        for k in ("out", "dfeats"):
            if k in bar:
                bar[k] += 6 * sigma[k] / float(ref[k].abs().max())
    atomic = ATOMIC_TENSORS.get(name, set())
    splits = (0,) + (R.SPLITS_3X3 if L.ntaps == 9 else R.SPLITS_1X1)
    first, fails = None, []
    for s in splits:
        if s in (0, 1):
            print("\n[plan] " + describe(R.Case("r", case.name, H, case.make, forced=s)))
        got = launch(hip, up, forced=s)
        line = "[roundoff] %s %dx%d split %d:" % (name, H, H, s)
        for k in tensors:
            err = rel_err(got[k], ref[k])
            line += " %s err %.2e err32 %.2e ratio %.2f bar %.2e;" % (k, err, err32[k], err / err32[k], bar[k])
            if not err <= bar[k]:
                fails.append(line)
        if s in (0, 1):
            print("\n" + line)
        if s == 1:
            first = got
        elif s > 1:
            for k in tensors:
                if k not in atomic and not torch.equal(got[k], first[k]):
                    fails.append("%s %dx%d: %s under split %d differs from split 1 in %d entries (largest %.3e)"
                                 % (name, H, H, k, s, int((got[k] != first[k]).sum()), float((got[k] - first[k]).abs().max())))
    assert not fails, "\n".join(fails)
