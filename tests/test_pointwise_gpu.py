"""The point-wise NMN kernels (csrc/pointwise.hip, csrc/pointwise_body.h) through the C ABI against the float64 references
of tests/helpers/pointwise_reference.py (independent of the library; tests/test_pointwise_reference.py holds them against
torch in float64, holds the restated launch rules against the compiled csrc/pointwise_plan.h, and asserts from those rules
which branches the case lists below reach).

EXACT cases.  Small integers stored as float32 with pointwise_reference.exact_ok asserted per case: every product, every
partial sum in any order and every atomic add is exact, so the comparison is torch.equal and the failure message names the
item, pixel and channel of the first difference.  This is the form for everything without an expf: And / Or and their
gradients (one launch of 8 items mixing the four channel shapes with min and max; ties at broadcast and other positions;
da or db NULL; NaN in a, in b and in both), pnmn_mask_bwd (five items adding into one dfeats map, two into one dattn map,
items without attention), pnmn_feat_grad_gather (examples owning 0, 1, 3, 4, 5, 8 and 9 items, empty first and last
examples, 1 to 512 examples and five map sizes: 8, 4, 2 and 1 pixel ranges), pnmn_accumulate and pnmn_set_rows (vector
bodies and scalar tails, src == NULL), pnmn_transpose_weights (square, oblong, partial tiles, more tiles than the grid,
one item per launch and all in one), the layout changes in both directions and through `rows` (both load widths, vector
and scalar channel stores, one to three chunks), and both max-pool directions (even and odd maps, the generic backward,
short last bands, the even kernel with fewer than 7 pooled rows, ties, all-zero and all-negative windows).

Every written buffer sits between guard rows of sentinels, which must come back untouched.  Buffers that are stored to
start as NaN (an element the kernel skips stays NaN and fails the comparison); buffers that are added into start from a
non-zero prefill (so `=` and `+=` differ).

ROUND-OFF cases: the one-channel head, SameModule, the answer loss and Adam.  Per tensor err = max|got - ref64| /
max|ref64| (max|got - ref64| where the reference is all zero); the bar is 4 * err32 + 2 * 2^-24 with err32 the same figure
of the reference evaluated in float32 on the CPU, never taken from the kernel.  Adam runs three steps under 1, 3 and 2048
workgroups per item, which must give identical bits.

The head's and SameModule's dout has mean 2 and their dw / db prefills are positive, so that dw and db -- sums over every
pixel of every item -- do not cancel: err is relative to max|ref| of a tensor, db is a tensor of ONE element, and with dout
of mean 0 it came out as -0.056 from item sums of magnitude 2 (HW = 209); two float32 roundings at that magnitude, no
defect, were 32 err32 on that scale.  The factor 4 stands; the data keep the scale of a sum at the size of its partial sums.

Measured err / err32 (MI355X), per tensor the largest over the cases of its family with the case it occurs in, and the bar
there in units of err32 (`pytest -s` prints the line of every tensor of every case):

    family  tensor          err / err32   case                    bar / err32
    dot1    out                 1.07      HW 105                      5.3
    dot1    din                 1.47      HW 196                      4.6
    dot1    dw                  1.11      HW 784                      4.8
    dot1    db                  2.01      HW 784                      8.6
    same    out                 1.16      HW 784                      5.3
    same    dfeats              1.26      HW 784                      5.1
    same    dfeats, row j       1.26      HW 784                      5.1
    same    dattn               1.00      HW 1                       11.3
    same    dw                  2.64      HW 196                      6.8
    same    db                  1.00      HW 1                        9.0
    loss    loss                1.00      n 1, A 2                   37.8
    loss    dlogits             1.13      n 64, A 28                  4.4
    adam    param               1.00      n 1, clamp 0, wd 0          5.1
    adam    exp_avg             1.60      n 5, clamp 0, wd 0          9.2
    adam    exp_avg_sq          1.03      n 5, clamp 5, wd 0.01       7.1

No tensor exceeds the factor 4.  Where the float64 reference is all zero (A = 1: loss and dlogits; answers == NULL: dlogits)
the kernel gives exact zeros.  Adam: up to n = 5 most tensors have the CPU's float32 bits (ratio 1.00).

Adam's reference is evaluated AT THE HYPERPARAMETERS THE KERNEL HOLDS: pnmn_clamp_adam rounds lr, the betas, eps, weight_decay
and clamp to float32 on entry (now stated in include/probnmn_hip.h) and weighs g^2 by 1 - (float)beta2.  For 0.999 that weight
is 1.3e-5 of itself away from torch's, which rounds 1 - beta2: against a reference at the unrounded betas exp_avg_sq would miss
its bar of about 5e-7 by that much (by the arithmetic; held on the CPU in test_adam_equals_torch_optim_adam).  The kernel was
built once with the weight formed in double: exp_avg_sq then met the bar at the unrounded betas too, but the changed last bits
move every training trajectory, and tests/test_parity_hygiene_gpu.py::test_joint_baseline_objective_matches_oracle -- which
fits a generator with this optimizer for 50 iterations, samples programs from it and allows three tensors beyond 5e-3 -- then
found six (gates flipped on other sampled programs; it passes with the rounded weight, run side by side).  The update is the
exact Adam update for a beta2 that differs by 1.3e-8, so the arithmetic stays as it was and the header says what it is.

SEEDED DEFECTS.  Three scratch builds of the library, each with one change of which in-bounds value is used (no address,
bound, barrier or wait touched), each run once against this file and against tests/test_hip_kernels.py (whose last dozen
functions are the earlier point-wise tests):
  1. `>=` for `>` in the arg-max of the generic max-pool backward (maxpool_kernel<true>: the last of equal maxima takes the
     gradient).  tests/test_hip_kernels.py PASSES it (87 passed: its maps are even and take the even kernel).  Here 14 cases
     fail: test_maxpool_flatten at 3x3, 2x5, 5x2, 15x15, 29x29, 29x15 and 14x74, both channel counts -- every map that
     takes the generic backward.
  2. `m[0]` for `m[k]` at k = 1 in the four-maps-in-flight loop of feat_grad_gather_kernel (the second map of a group is
     weighted by the first one's attention).  tests/test_hip_kernels.py PASSES it (no example of its gather test owns four
     items).  Here all 10 cases of test_feat_grad_gather fail.
  3. `>=` for `>` in a thread's own scan of first_argmax (a thread that meets equal maxima 256 pixels apart keeps the later
     one).  tests/test_hip_kernels.py PASSES it (its tie sits in two different threads).  Here test_same_module[784] fails:
     the all-equal attention picks a pixel other than 0.  (HW = 196 cannot see it: no thread scans two pixels.)

Time: the 146 tests of this file take 3.5 s on an MI355X (references and the CPU float32 yardsticks included).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pointwise_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

C = R.C
GUARD = 64          # elements in front of and behind every written buffer
SENTINEL = 4242.0
U32 = 2.0 ** -24
NAN = float("nan")
F32 = torch.float32


@pytest.fixture(scope="module")
def hip():
    from probnmn import _hip

    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a MI355X"
    return _hip


def dev():
    return torch.device("cuda:0")


def up(t):
    return t.to(dev()).contiguous()


class Guarded:
    """`pre` [n][...] in device memory, every row of it between GUARD sentinels (rows start 16-byte aligned)."""

    def __init__(self, pre):
        self.shape = tuple(pre.shape)
        self.n, self.sz = pre.shape[0], int(pre[0].numel())
        self.buf = torch.full((self.n, 2 * GUARD + (self.sz + 3) // 4 * 4), SENTINEL, dtype=pre.dtype, device=dev())
        self.buf[:, GUARD:GUARD + self.sz] = pre.reshape(self.n, self.sz).to(dev())

    def ptr(self, i=0):
        return self.buf[i].data_ptr() + GUARD * self.buf.element_size()

    def get(self, what):
        assert bool((self.buf[:, :GUARD] == SENTINEL).all()) and bool((self.buf[:, GUARD + self.sz:] == SENTINEL).all()), \
            "elements in front of or behind %s were written" % what
        return self.buf[:, GUARD:GUARD + self.sz].reshape(self.shape).cpu()


def nans(*shape):
    return torch.full(shape, NAN)


def run(hip, name, recs, *args):
    buf = hip.to_device(recs, dev())
    call(hip, name, buf.data_ptr(), len(recs), *args)
    return buf


def call(hip, name, *args):
    try:
        hip.check(getattr(hip.lib(), name)(*args, hip.stream_ptr(dev())), name)
        torch.cuda.synchronize()
    except RuntimeError as e:  # (a HIP error is sticky: nothing after it on this device means anything)
        pytest.exit("the device reported an error in %s: %s" % (name, e), returncode=3)


def assert_exact(got, ref, what, names):
    """torch.equal, NaN equal to NaN; the message names the first difference by `names` (one per dimension)."""
    ref = ref.to(torch.float64).cpu()
    got = got.to(torch.float64).cpu().reshape(ref.shape)
    wrong = (torch.nan_to_num(got, nan=1e30) != torch.nan_to_num(ref, nan=1e30)) | (torch.isnan(got) != torch.isnan(ref))
    if not bool(wrong.any()):
        return
    at = torch.nonzero(wrong)
    first = tuple(at[0].tolist())
    raise AssertionError("%s differs in %d of %d entries; first at %s: got %r, want %r; %s" % (
        what, at.shape[0], ref.numel(), ", ".join("%s %d" % (nm, i) for nm, i in zip(names, first)), float(got[first]), float(ref[first]),
        "; ".join("%s in %s" % (nm, sorted(set(at[:, k].tolist()))[:12]) for k, nm in enumerate(names))))


def rel_err(got, ref):
    ref = ref.to(torch.float64).cpu()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return float((got.to(torch.float64).cpu().reshape(ref.shape) - ref).abs().max()) / (scale if scale > 0 else 1.0)


def check_roundoff(family, where, got, ref, r32, names):
    """Every tensor of `got` under 4 * err32 + 2 * 2^-24; prints one line per tensor."""
    fails = []
    for k in got:
        err, err32 = rel_err(got[k], ref[k]), rel_err(r32[k], ref[k])
        bar = 4 * err32 + 2 * U32
        line = "[roundoff] %s %s %s: err %.3e err32 %.3e ratio %s bar %.3e" % (family, where, k, err, err32,
                                                                                 "%.2f" % (err / err32) if err32 > 0 else "-", bar)
        print("\n" + line, end="")
        if not err <= bar:
            d = (got[k].to(torch.float64).cpu().reshape(ref[k].shape) - ref[k].cpu()).abs()
            first = tuple(torch.nonzero(d == d.max())[0].tolist())
            fails.append(line + "; worst at " + ", ".join("%s %d" % (nm, i) for nm, i in zip(names.get(k, ()), first)))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# conv1x1 (128 -> 1) + sigmoid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", R.DOT1_HW)
def test_dot1_head(hip, HW):
    """Three items sharing dw / db (prefilled); out and din start as NaN and must be fully written."""
    d = R.dot1_data(HW)
    ref, r32 = R.dot1_reference(d), R.dot1_reference(d, F32)
    n = R.DOT1_ITEMS
    x, w, b, dout = up(d["x"]), up(d["w"]), up(d["b"]), up(d["dout"])
    out, din = Guarded(nans(n, HW)), Guarded(nans(n, HW, C))
    dw, db = Guarded(d["dw_pre"].unsqueeze(0)), Guarded(d["db_pre"].unsqueeze(0))
    recs = np.zeros(n, hip.DOT1_ITEM)
    for i in range(n):
        r = recs[i]
        r["in"], r["w"], r["b"], r["out"] = x[i].data_ptr(), w.data_ptr(), b.data_ptr(), out.ptr(i)
        r["dout"], r["din"], r["dw"], r["db"] = dout[i].data_ptr(), din.ptr(i), dw.ptr(), db.ptr()
    run(hip, "pnmn_dot1_sigmoid_fwd", recs, HW)
    got = {"out": out.get("out")}
    run(hip, "pnmn_dot1_sigmoid_bwd", recs, HW)
    got.update(din=din.get("din"), dw=dw.get("dw")[0], db=db.get("db")[0])
    assert torch.equal(out.get("out"), got["out"]), "the backward wrote `out`"
    check_roundoff("dot1", "HW %d" % HW, got, ref, r32, dict(out=("item", "pixel"), din=("item", "pixel", "channel"), dw=("channel",)))


# ---------------------------------------------------------------------------------------------------------------------
# SameModule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", R.SAME_HW)
def test_same_module(hip, HW):
    """One item per attention kind (pointwise_reference.same_kinds): random, the maximum at the last pixel, all equal, equal
    maxima at pixels (255, 256) and (0, 783) at HW = 784, and one with dattn == NULL.  dfeats and dattn are prefilled: both are
    `+=`.  The arg-max row of dfeats, which receives both gradient paths, is also compared on its own."""
    d = R.same_data(HW)
    ref, r32 = R.same_reference(d), R.same_reference(d, F32)
    js = ref.pop("j")
    assert r32.pop("j") == js
    n = len(d["kinds"])
    feats, attn, w, b, dout = (up(d[k]) for k in ("feats", "attn", "w", "b", "dout"))
    out, dfeats, dattn = Guarded(nans(n, HW)), Guarded(d["dfeats_pre"]), Guarded(d["dattn_pre"])
    dw, db = Guarded(d["dw_pre"].unsqueeze(0)), Guarded(d["db_pre"].unsqueeze(0))
    recs = np.zeros(n, hip.SAME_ITEM)
    for i in range(n):
        r = recs[i]
        r["feats"], r["attn"], r["w"], r["b"], r["out"] = feats[i].data_ptr(), attn[i].data_ptr(), w.data_ptr(), b.data_ptr(), out.ptr(i)
        r["dout"], r["dfeats"], r["dw"], r["db"] = dout[i].data_ptr(), dfeats.ptr(i), dw.ptr(), db.ptr()
        r["dattn"] = 0 if d["kinds"][i] == "nodattn" else dattn.ptr(i)
    run(hip, "pnmn_same_fwd", recs, HW)
    got = {"out": out.get("out")}
    run(hip, "pnmn_same_bwd", recs, HW)
    got.update(dfeats=dfeats.get("dfeats"), dattn=dattn.get("dattn"), dw=dw.get("dw")[0], db=db.get("db")[0])
    got["dfeats_row_j"] = torch.stack([got["dfeats"][i, j] for i, j in enumerate(js)])
    i0 = d["kinds"].index("nodattn")
    assert torch.equal(got["dattn"][i0], d["dattn_pre"][i0]), "dattn of the item whose dattn is NULL"
    print("\n[same] HW %d: kinds %s arg-max %s" % (HW, d["kinds"], js), end="")
    check_roundoff("same", "HW %d" % HW, got, ref, r32, dict(out=("item", "pixel"), dfeats=("item", "pixel", "channel"),
                                                             dfeats_row_j=("item", "channel"), dattn=("item", "pixel"), dw=("channel",)))


# ---------------------------------------------------------------------------------------------------------------------
# And / Or
# ---------------------------------------------------------------------------------------------------------------------
def minmax_launch(hip, items, HW, variant, backward):
    n = len(items)
    a, b, dout = [up(it["a"]) for it in items], [up(it["b"]) for it in items], [up(it["dout"]) for it in items]
    out = [Guarded(nans(1, HW, max(it["ac"], it["bc"]))) for it in items]
    da, db = [Guarded(it["da_pre"].unsqueeze(0)) for it in items], [Guarded(it["db_pre"].unsqueeze(0)) for it in items]
    recs = np.zeros(n, hip.MINMAX_ITEM)
    for i, it in enumerate(items):
        r = recs[i]
        na, nb = R.minmax_nulls(variant, i)
        r["a"], r["b"], r["out"], r["dout"] = a[i].data_ptr(), b[i].data_ptr(), out[i].ptr(), dout[i].data_ptr()
        r["da"], r["db"] = 0 if na else da[i].ptr(), 0 if nb else db[i].ptr()
        r["a_channels"], r["b_channels"], r["is_max"] = it["ac"], it["bc"], it["is_max"]
    run(hip, "pnmn_minmax_fwd", recs, HW, C)
    if backward:
        run(hip, "pnmn_minmax_bwd", recs, HW, C)
    return out, da, db


@pytest.mark.parametrize("variant", R.MINMAX_NULLS)
@pytest.mark.parametrize("HW", R.MINMAX_HW)
def test_minmax_exact(hip, HW, variant):
    """One launch of 8 items: (1,1), (1,C), (C,1), (C,C) x min / max; da and db prefilled; in "alternate" one of them is NULL."""
    items = R.minmax_data(HW)
    out, da, db = minmax_launch(hip, items, HW, variant, True)
    for i, it in enumerate(items):
        where = "item %d (%d, %d, %s) HW %d" % (i, it["ac"], it["bc"], "max" if it["is_max"] else "min", HW)
        assert_exact(out[i].get("out")[0], R.minmax_fwd_reference(it), "out of " + where, ("pixel", "channel"))
        ra, rb = R.minmax_bwd_reference(it, R.minmax_nulls(variant, i))
        assert_exact(da[i].get("da")[0], ra, "da of " + where, ("pixel", "channel"))
        assert_exact(db[i].get("db")[0], rb, "db of " + where, ("pixel", "channel"))


@pytest.mark.parametrize("HW", R.MINMAX_HW)
def test_minmax_forward_propagates_nan(hip, HW):
    """NaN in a, in b and in both give NaN, as torch.min / torch.max; every other element as without them."""
    items = R.minmax_data(HW, nan=True)
    out, _, _ = minmax_launch(hip, items, HW, "none", False)
    for i, it in enumerate(items):
        ref = R.minmax_fwd_reference(it)
        assert bool(torch.isnan(ref).any())
        assert_exact(out[i].get("out")[0], ref, "out of item %d (%d, %d, is_max %d) HW %d" % (i, it["ac"], it["bc"], it["is_max"], HW), ("pixel", "channel"))


# ---------------------------------------------------------------------------------------------------------------------
# backward of feats * attn
# ---------------------------------------------------------------------------------------------------------------------
def maskbwd_records(hip, items_of, dx, attn, feats, dfeats_ptr, dattn_ptr):
    recs = np.zeros(len(items_of), hip.MASKBWD_ITEM)
    for i, (x, a, f, t, da) in enumerate(items_of):
        r = recs[i]
        r["dx"], r["dfeats"] = dx[x].data_ptr(), dfeats_ptr(t)
        if a >= 0:
            r["attn"] = attn[a].data_ptr()
            r["feats"] = feats[f].data_ptr() if feats is not None else 0
            r["dattn"] = dattn_ptr(da) if dattn_ptr is not None else 0
    return recs


@pytest.mark.parametrize("HW", R.MASKBWD_HW)
def test_mask_bwd_adds_into_shared_maps(hip, HW):
    """Seven items: five add into dfeats map 0 and two into dattn map 0 (atomics from several workgroups), three have
    attn == NULL; both outputs are prefilled: `+=`, as the header now says."""
    d = R.maskbwd_data(HW)
    rf, ra = R.maskbwd_reference(d)
    dx, feats, attn = up(d["dx"]), up(d["feats"]), up(d["attn"])
    dfeats, dattn = Guarded(d["dfeats_pre"]), Guarded(d["dattn_pre"])
    items = [(i, i if a >= 0 else -1, i, f, a) for i, (f, a) in enumerate(R.MASKBWD_ITEMS)]
    run(hip, "pnmn_mask_bwd", maskbwd_records(hip, items, dx, attn, feats, dfeats.ptr, dattn.ptr), HW)
    assert_exact(dfeats.get("dfeats"), rf, "dfeats (HW %d)" % HW, ("map", "pixel", "channel"))
    assert_exact(dattn.get("dattn"), ra, "dattn (HW %d)" % HW, ("map", "pixel"))


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=[c[0] for c in R.GATHER_CASES])
def test_feat_grad_gather(hip, case):
    """gfeat is prefilled; the ranges of examples without items must keep it bit for bit (the whole buffer is compared)."""
    name, n_ex, HW, counts = case
    d = R.gather_data(n_ex, HW)
    ref = R.gather_reference(d, counts, device=dev())
    dx, attn = up(d["dx"]), up(d["attn"])
    gfeat = Guarded(d["pre"].reshape(1, -1))
    base, stride = gfeat.ptr(), 4 * HW * C
    items = [(x, a, 0, e, 0) for (e, x, a) in R.gather_items(counts)]
    recs = maskbwd_records(hip, items, dx, attn, None, lambda e: base + e * stride, None)
    print("\n[gather] %s: %d examples, HW %d, %d items, %s" % (name, n_ex, HW, len(items), sorted(R.gather_facts(n_ex, HW, counts))), end="")
    buf = hip.to_device(recs, dev())
    call(hip, "pnmn_feat_grad_gather", buf.data_ptr(), gfeat.ptr(), len(recs), n_ex, HW)
    assert_exact(gfeat.get("gfeat").reshape(n_ex, HW, C), ref, "gfeat (%s)" % name, ("example", "pixel", "channel"))


# ---------------------------------------------------------------------------------------------------------------------
# accumulate / set_rows
# ---------------------------------------------------------------------------------------------------------------------
def axpy_launch(hip, name, data, null_src):
    src = [up(it["src"]) for it in data]
    dst = [Guarded(it["dst"].unsqueeze(0)) for it in data]
    recs = np.zeros(len(data), hip.AXPY_ITEM)
    for i, it in enumerate(data):
        recs[i]["src"], recs[i]["dst"], recs[i]["n"] = 0 if null_src(i) else src[i].data_ptr(), dst[i].ptr(), it["n"]
    run(hip, name, recs)
    return dst


def test_accumulate_bodies_and_tails(hip):
    data = R.axpy_data()
    dst = axpy_launch(hip, "pnmn_accumulate", data, lambda i: False)
    for i, it in enumerate(data):
        assert_exact(dst[i].get("dst")[0], R.accumulate_reference(it), "dst of item %d (n = %d)" % (i, it["n"]), ("element",))


@pytest.mark.parametrize("nulls", ["none", "odd items", "all"])
def test_set_rows_bodies_tails_and_zeros(hip, nulls):
    data = R.axpy_data(1)
    null = {"none": lambda i: False, "odd items": lambda i: i % 2 == 1, "all": lambda i: True}[nulls]
    dst = axpy_launch(hip, "pnmn_set_rows", data, null)
    for i, it in enumerate(data):
        assert_exact(dst[i].get("dst")[0], R.set_rows_reference(it, null(i)), "dst of item %d (n = %d, src %s)" % (i, it["n"], "NULL" if null(i) else "given"),
                     ("element",))


# ---------------------------------------------------------------------------------------------------------------------
# weight transposition
# ---------------------------------------------------------------------------------------------------------------------
WT_LAUNCHES = [[s] for s in R.WTRANS_SHAPES] + [list(R.WTRANS_SHAPES)]


@pytest.mark.parametrize("shapes", WT_LAUNCHES, ids=["x".join(map(str, s[0])) if len(s) == 1 else "all in one launch" for s in WT_LAUNCHES])
def test_transpose_weights(hip, shapes):
    """[cout][t][cin] -> [cin][taps - 1 - t][cout], every element (dst starts as NaN).  [256][9][128] has 288 tiles, more than
    the grid's 256: the workgroups walk them."""
    src = [R.wtrans_data(s) for s in shapes]
    srcd = [up(s) for s in src]
    dst = [Guarded(nans(1, s.numel())) for s in src]
    recs = np.zeros(len(shapes), hip.WTRANS_ITEM)
    for i, (cout, taps, cin) in enumerate(shapes):
        r = recs[i]
        r["src"], r["dst"], r["cout"], r["cin"], r["ntaps"] = srcd[i].data_ptr(), dst[i].ptr(), cout, cin, taps
    run(hip, "pnmn_transpose_weights", recs)
    for i, s in enumerate(shapes):
        assert_exact(dst[i].get("dst")[0], R.wtrans_reference(src[i]), "dst of item %d %s (%d tiles)" % (i, s, R.wtrans_tiles(s[0], s[2], s[1])),
                     ("cin", "tap", "cout"))


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", R.LAYOUT_HW)
def test_layout_both_directions(hip, HW):
    """NCHW -> NHWC equals permute; back again gives the input bit for bit; every C of the list at this map size."""
    n = R.LAYOUT_N
    for Cn in R.LAYOUT_C:
        x = R.layout_data(n, Cn, HW)
        xd = up(x)
        y, z = Guarded(nans(1, n * HW * Cn)), Guarded(nans(1, n * Cn * HW))
        where = "C %d HW %d (%s)" % (Cn, HW, ", ".join(sorted(R.layout_facts(Cn, HW))))
        call(hip, "pnmn_nchw_to_nhwc", xd.data_ptr(), y.ptr(), n, Cn, HW)
        assert_exact(y.get("nhwc").reshape(n, HW, Cn), R.to_nhwc_reference(x), "nhwc at " + where, ("example", "pixel", "channel"))
        call(hip, "pnmn_nhwc_to_nchw", y.ptr(), z.ptr(), n, Cn, HW)
        assert_exact(z.get("nchw").reshape(n, Cn, HW), x, "nchw (round trip) at " + where, ("example", "channel", "pixel"))


@pytest.mark.parametrize("rows", sorted(R.LAYOUT_ROWS))
def test_layout_rows(hip, rows):
    """Example i of the output is example rows[i] of a source batch of five: a repeated row, descending rows, two of five."""
    pick = R.LAYOUT_ROWS[rows]
    for (Cn, HW) in R.LAYOUT_ROWS_SHAPES:
        x = R.layout_data(5, Cn, HW, seed=1)
        xd, rd = up(x), torch.tensor(pick, dtype=torch.int64, device=dev())
        y = Guarded(nans(1, len(pick) * HW * Cn))
        call(hip, "pnmn_nchw_to_nhwc_rows", xd.data_ptr(), y.ptr(), rd.data_ptr(), len(pick), Cn, HW)
        assert_exact(y.get("nhwc").reshape(len(pick), HW, Cn), R.to_nhwc_reference(x, pick), "nhwc of rows %s at C %d HW %d" % (pick, Cn, HW),
                     ("example", "pixel", "channel"))


# ---------------------------------------------------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", R.POOL_C)
@pytest.mark.parametrize("H,W", R.POOL_MAPS, ids=["%dx%d" % m for m in R.POOL_MAPS])
def test_maxpool_flatten(hip, H, W, Cn):
    """Forward and backward on the same map list.  din starts as NaN: the row and column an odd map leaves uncovered must
    come back as written zeros.  4x74 and 14x74 are the shapes whose backward asked for 67 340 bytes of LDS."""
    d = R.pool_data(H, W, Cn)
    n, PS = R.POOL_N, (H // 2) * (W // 2)
    x, dout = up(d["x"]), up(d["dout"])
    out, din = Guarded(nans(1, n * Cn * PS)), Guarded(nans(1, n * H * W * Cn))
    print("\n[pool] %dx%d C %d: forward %s; backward %s" % (H, W, Cn, sorted(R.pool_facts(H, W, False)), sorted(R.pool_facts(H, W, True))), end="")
    call(hip, "pnmn_maxpool2_flatten_fwd", x.data_ptr(), out.ptr(), n, H, W, Cn)
    assert_exact(out.get("out").reshape(n, Cn, H // 2, W // 2), R.pool_fwd_reference(d["x"]).reshape(n, Cn, H // 2, W // 2), "out %dx%d" % (H, W),
                 ("example", "channel", "pooled row", "pooled column"))
    call(hip, "pnmn_maxpool2_flatten_bwd", x.data_ptr(), dout.data_ptr(), din.ptr(), n, H, W, Cn)
    assert_exact(din.get("din").reshape(n, H, W, Cn), R.pool_bwd_reference(d["x"], d["dout"]), "din %dx%d" % (H, W), ("example", "row", "column", "channel"))


# ---------------------------------------------------------------------------------------------------------------------
# answer loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", R.LOSS_NULLS)
@pytest.mark.parametrize("A", R.LOSS_A)
@pytest.mark.parametrize("n", R.LOSS_N)
def test_answer_loss(hip, n, A, nulls):
    """Tied maxima (the first is predicted), logits of +-80, invalid rows, and each optional pointer NULL in turn."""
    d = R.loss_data(n, A)
    ref, r32 = R.loss_reference(d, nulls), R.loss_reference(d, nulls, F32)
    z, ans, valid = up(d["logits"]), up(d["answers"]), up(d["valid"])
    pred = Guarded(torch.full((1, n), 4242, dtype=torch.int64))
    loss, dl = Guarded(nans(1, n)), Guarded(nans(1, n * A))
    call(hip, "pnmn_answer_loss", z.data_ptr(), None if nulls == "answers" else ans.data_ptr(), None if nulls == "valid" else valid.data_ptr(),
         None if nulls == "predictions" else pred.ptr(), loss.ptr(), None if nulls == "dlogits" else dl.ptr(), n, A, d["unknown"], d["scale"])
    got = {"loss": loss.get("loss")[0]}
    if nulls == "predictions":
        assert bool((pred.get("predictions") == 4242).all())
    else:
        assert_exact(pred.get("predictions")[0], ref["predictions"], "predictions (n %d, A %d)" % (n, A), ("row",))
    if nulls == "dlogits":
        assert bool(torch.isnan(dl.get("dlogits")).all())
    else:
        got["dlogits"] = dl.get("dlogits").reshape(n, A)
    check_roundoff("loss", "n %d A %d NULL %s" % (n, A, nulls), got, ref, r32, dict(loss=("row",), dlogits=("row", "answer")))


# ---------------------------------------------------------------------------------------------------------------------
# clamp + Adam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", R.ADAM_WD)
@pytest.mark.parametrize("clamp", R.ADAM_CLAMP)
def test_clamp_adam(hip, clamp, wd):
    """One launch of six items (n = 1, 3, 4, 5, 1031, 100003) whose Adam step counts differ, three steps, under 1, 3 and 2048
    workgroups per item: identical bits (an element's update does not depend on the grid), and each under its round-off bar."""
    data = R.adam_data()
    grads = [[up(g) for g in it["grads"]] for it in data]
    results = {}
    for blocks in R.ADAM_BLOCKS:
        state = {k: [Guarded(it[k].unsqueeze(0)) for it in data] for k in ("param", "exp_avg", "exp_avg_sq")}
        for step in range(R.ADAM_STEPS):
            recs = np.zeros(len(data), hip.ADAM_ITEM)
            for i, it in enumerate(data):
                r = recs[i]
                r["param"], r["exp_avg"], r["exp_avg_sq"], r["grad"], r["n"] = state["param"][i].ptr(), state["exp_avg"][i].ptr(), state["exp_avg_sq"][i].ptr(), grads[i][step].data_ptr(), it["n"]
                r["bc1"], r["bc2_sqrt"] = R.adam_bias_corrections(it["first"] + step)
            h = R.ADAM_HYPER
            if blocks == 2048:  # (what pnmn_clamp_adam launches)
                run(hip, "pnmn_clamp_adam", recs, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, clamp)
            else:
                run(hip, "pnmn_clamp_adam_blocks", recs, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, clamp, blocks)
        results[blocks] = [{k: state[k][i].get(k)[0] for k in state} for i in range(len(data))]
    for i, it in enumerate(data):
        for blocks in R.ADAM_BLOCKS[1:]:
            for k in results[blocks][i]:
                assert torch.equal(results[blocks][i][k], results[R.ADAM_BLOCKS[0]][i][k]), \
                    "%s of item %d (n = %d) under %d workgroups differs from %d" % (k, i, it["n"], blocks, R.ADAM_BLOCKS[0])
        check_roundoff("adam", "n %d clamp %g wd %g" % (it["n"], clamp, wd), results[R.ADAM_BLOCKS[0]][i], R.adam_reference(it, clamp, wd),
                       R.adam_reference(it, clamp, wd, F32), dict(param=("element",), exp_avg=("element",), exp_avg_sq=("element",)))


# ---------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(hip):
    """Every argument error returns its code and launches nothing: the output buffers keep their sentinels."""
    lib, st = hip.lib(), hip.stream_ptr(dev())
    E, S = hip.EINVAL, hip.ESHAPE
    buf = Guarded(torch.full((1, 2 * 8 * 8 * 64), SENTINEL))
    src = torch.zeros(2 * 8 * 8 * 64, device=dev())
    rows = torch.zeros(2, dtype=torch.int64, device=dev())
    items = torch.zeros(1024, dtype=torch.uint8, device=dev())
    p, o, it_, r = src.data_ptr(), buf.ptr(), items.data_ptr(), rows.data_ptr()
    for name in ("pnmn_dot1_sigmoid_fwd", "pnmn_dot1_sigmoid_bwd", "pnmn_same_fwd", "pnmn_same_bwd", "pnmn_mask_bwd"):
        f = getattr(lib, name)
        assert (f(None, 1, 196, st), f(it_, 1, 0, st), f(it_, 1, -3, st), f(None, 0, 196, st), f(it_, -1, 196, st)) == (E, E, E, 0, 0), name
    for name in ("pnmn_minmax_fwd", "pnmn_minmax_bwd"):
        f = getattr(lib, name)
        assert (f(None, 1, 196, C, st), f(it_, 1, 0, C, st), f(it_, 1, 196, 64, st), f(it_, 1, 196, 1, st), f(None, 0, 196, C, st)) == (E, E, E, E, 0), name
    f = lib.pnmn_feat_grad_gather
    assert (f(None, o, 1, 1, 4, st), f(it_, None, 1, 1, 4, st), f(it_, o, 1, 1, 0, st), f(None, None, 0, 1, 4, st), f(None, None, 1, 0, 4, st)) == (E, E, E, 0, 0)
    for name in ("pnmn_accumulate", "pnmn_set_rows", "pnmn_transpose_weights"):
        f = getattr(lib, name)
        assert (f(None, 1, st), f(None, 0, st), f(it_, -2, st)) == (E, 0, 0), name
    for name in ("pnmn_nchw_to_nhwc", "pnmn_nhwc_to_nchw"):
        f = getattr(lib, name)
        assert (f(None, o, 2, 64, 64, st), f(p, None, 2, 64, 64, st), f(p, o, 2, 0, 64, st), f(p, o, 2, 64, 0, st), f(p, o, 0, 64, 64, st)) == (E, E, E, E, 0), name
    f = lib.pnmn_nchw_to_nhwc_rows
    assert (f(p, o, None, 2, 64, 64, st), f(None, o, r, 2, 64, 64, st), f(p, None, r, 2, 64, 64, st), f(p, o, r, 2, 0, 64, st), f(p, o, r, 2, 64, 0, st)) == (E, E, E, E, E)
    f = lib.pnmn_maxpool2_flatten_fwd
    assert (f(None, o, 2, 8, 8, 64, st), f(p, None, 2, 8, 8, 64, st), f(p, o, 2, 8, 8, 96, st), f(p, o, 2, 1, 8, 64, st), f(p, o, 2, 8, 1, 64, st),
            f(p, o, 0, 8, 8, 64, st), f(p, o, 2, 2, 316, 64, st)) == (E, E, E, E, E, 0, S)
    f = lib.pnmn_maxpool2_flatten_bwd
    assert (f(None, p, o, 2, 8, 8, 64, st), f(p, None, o, 2, 8, 8, 64, st), f(p, p, None, 2, 8, 8, 64, st), f(p, p, o, 2, 8, 8, 32, st),
            f(p, p, o, 2, 1, 8, 64, st), f(p, p, o, 2, 8, 1, 64, st), f(p, p, o, 0, 8, 8, 64, st), f(p, p, o, 2, 3, 317, 64, st)) == (E, E, E, E, E, E, 0, S)
    f = lib.pnmn_answer_loss
    assert (f(None, None, None, None, o, None, 4, 4, 4, 1.0, st), f(p, None, None, None, None, None, 4, 4, 4, 1.0, st),
            f(p, None, None, None, o, None, 4, 0, 4, 1.0, st), f(p, None, None, None, o, None, 0, 4, 4, 1.0, st)) == (E, E, E, 0)
    f = lib.pnmn_clamp_adam
    assert (f(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, st), f(None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, st)) == (E, 0)
    f = lib.pnmn_clamp_adam_blocks
    assert (f(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, 8, st), f(it_, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, 0, st),
            f(it_, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, -1, st), f(it_, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5.0, 0, st)) == (E, E, E, 0)
    torch.cuda.synchronize()
    assert bool((buf.get("the output of a refused call") == SENTINEL).all())
    assert bool((src == 0).all()) and bool((items == 0).all())
