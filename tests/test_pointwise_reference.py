"""The float64 references of the point-wise NMN kernels (tests/helpers/pointwise_reference.py) and their restatement of
the launch-shape rules, held on the CPU: against the torch operations the reference project calls (float64, autograd),
against the compiled csrc/pointwise_plan.h, and for the branches the case lists of tests/test_pointwise_gpu.py reach."""
import os
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pointwise_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOL = dict(rtol=1e-11, atol=1e-12)
C = R.C


@pytest.mark.parametrize("HW", [1, 57, 196])
def test_dot1_equals_conv2d_sigmoid_autograd(HW):
    d = R.dot1_data(HW)
    x = d["x"].double().permute(0, 2, 1).reshape(-1, C, HW, 1).requires_grad_(True)
    w = d["w"].double().reshape(1, C, 1, 1).requires_grad_(True)
    b = d["b"].double().requires_grad_(True)
    y = torch.sigmoid(F.conv2d(x, w, b))
    y.backward(d["dout"].double().reshape(y.shape))
    ref = R.dot1_reference(d)
    torch.testing.assert_close(ref["out"], y.detach().reshape(-1, HW), **TOL)
    torch.testing.assert_close(ref["din"], x.grad.reshape(-1, C, HW).permute(0, 2, 1), **TOL)
    torch.testing.assert_close(ref["dw"], d["dw_pre"].double() + w.grad.reshape(C), **TOL)
    torch.testing.assert_close(ref["db"], d["db_pre"].double() + b.grad, **TOL)


@pytest.mark.parametrize("side", [1, 14, 28])
def test_same_equals_the_oracle_module(side):
    """oracle.nmn_oracle.same_module (max_pool2d(return_indices) + index_select + conv + sigmoid) under float64 autograd, every
    attention kind: ties, the maximum at the last pixel, all equal."""
    from oracle import nmn_oracle

    HW = side * side
    d = R.same_data(HW)
    ref = R.same_reference(d)
    n = len(d["kinds"])
    feats = d["feats"].double().permute(0, 2, 1).reshape(n, C, side, side).requires_grad_(True)
    attn = d["attn"].double().reshape(n, 1, side, side).requires_grad_(True)
    sd = {"s.conv.weight": d["w"].double().reshape(1, C + 1, 1, 1).requires_grad_(True), "s.conv.bias": d["b"].double().requires_grad_(True)}
    y = torch.cat([nmn_oracle.same_module(sd, "s", feats[i:i + 1], attn[i:i + 1]) for i in range(n)])
    y.backward(d["dout"].double().reshape(y.shape))
    torch.testing.assert_close(ref["out"], y.detach().reshape(n, HW), **TOL)
    torch.testing.assert_close(ref["dfeats"], d["dfeats_pre"].double() + feats.grad.reshape(n, C, HW).permute(0, 2, 1), **TOL)
    for i, k in enumerate(d["kinds"]):
        want = d["dattn_pre"][i].double() + (0 if k == "nodattn" else attn.grad[i].reshape(HW))
        torch.testing.assert_close(ref["dattn"][i], want, **TOL)
        if R.same_expected_argmax(k, HW) is not None:
            assert ref["j"][i] == R.same_expected_argmax(k, HW), k
    torch.testing.assert_close(ref["dw"], d["dw_pre"].double() + sd["s.conv.weight"].grad.reshape(C + 1), **TOL)
    torch.testing.assert_close(ref["db"], d["db_pre"].double() + sd["s.conv.bias"].grad, **TOL)
    if HW == 784:
        assert {"tie255_256", "tie0_783"} <= set(d["kinds"])


@pytest.mark.parametrize("HW", [1, 99])
def test_minmax_equals_torch_min_max(HW):
    for it in R.minmax_data(HW):
        a, b = it["a"].double().requires_grad_(True), it["b"].double().requires_grad_(True)
        y = torch.max(a, b) if it["is_max"] else torch.min(a, b)
        y.backward(it["dout"].double())
        assert torch.equal(R.minmax_fwd_reference(it), y.detach())
        da, db = R.minmax_bwd_reference(it)
        assert torch.equal(da, it["da_pre"].double() + a.grad) and torch.equal(db, it["db_pre"].double() + b.grad)
        ties = it["a"] == it["b"]
        assert bool(ties.any()) or HW == 1
        da0, db0 = R.minmax_bwd_reference(it, nulls=(True, False))
        assert torch.equal(da0, it["da_pre"].double()) and torch.equal(db0, db)
    for it in R.minmax_data(HW, nan=True):
        y = torch.max(it["a"].double(), it["b"].double()) if it["is_max"] else torch.min(it["a"].double(), it["b"].double())
        ref = R.minmax_fwd_reference(it)
        assert bool(torch.isnan(y).any()) and torch.equal(torch.isnan(ref), torch.isnan(y))
        assert torch.equal(torch.nan_to_num(ref, nan=7.0), torch.nan_to_num(y, nan=7.0))
        if HW > 1 and it["ac"] == it["bc"] == C:   # NaN in a alone, in b alone and in both at one output element
            na, nb = torch.isnan(it["a"]), torch.isnan(it["b"])
            assert bool((na & ~nb).any()) and bool((nb & ~na).any()) and bool((na & nb).any())


@pytest.mark.parametrize("HW", [1, 9, 196])
def test_mask_bwd_equals_autograd(HW):
    d = R.maskbwd_data(HW)
    feats, attn = d["feats"].double().requires_grad_(True), d["attn"].double().requires_grad_(True)
    total = 0
    for i, (f, a) in enumerate(R.MASKBWD_ITEMS):
        x = feats[i] * (attn[i].unsqueeze(-1) if a >= 0 else 1.0)
        total = total + (x * d["dx"][i].double()).sum()
    total.backward()
    dfeats, dattn = R.maskbwd_reference(d)
    want_f, want_a = d["dfeats_pre"].double().clone(), d["dattn_pre"].double().clone()
    for i, (f, a) in enumerate(R.MASKBWD_ITEMS):
        want_f[f] += feats.grad[i]      # (d/dfeats of item i's product lands in the map the item names)
        if a >= 0:
            want_a[a] += attn.grad[i]
    assert torch.equal(dfeats, want_f) and torch.equal(dattn, want_a)
    assert sum(1 for f, _ in R.MASKBWD_ITEMS if f == 0) == 5 and sum(1 for _, a in R.MASKBWD_ITEMS if a == 0) == 2
    assert any(a < 0 for _, a in R.MASKBWD_ITEMS)


def test_gather_equals_the_sum_of_mask_bwd_contributions():
    name, n_ex, HW, counts = R.GATHER_CASES[1]
    d = R.gather_data(n_ex, HW)
    ref = R.gather_reference(d, counts)
    feats = torch.zeros(n_ex, HW, C, dtype=torch.float64, requires_grad=True)
    total = 0
    for (e, x, a) in R.gather_items(counts):
        total = total + (feats[e] * (d["attn"][a].double().unsqueeze(-1) if a >= 0 else 1.0) * d["dx"][x].double()).sum()
    total.backward()
    assert torch.equal(ref, d["pre"].double() + feats.grad)
    assert torch.equal(ref[0], d["pre"][0].double())      # the example without items


@pytest.mark.parametrize("H,W", R.POOL_MAPS)
def test_pool_equals_max_pool2d_with_ties(H, W):
    d = R.pool_data(H, W, 64)
    x = d["x"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)   # the pre-activation: ReLU is part of what is differentiated
    y = F.max_pool2d(F.relu(x), 2, 2).reshape(R.POOL_N, -1)
    y.backward(d["dout"].double())
    # the kernel's input is the ReLU'd map; the reference is also defined on maps with negative entries (the gate is `> 0`)
    xr = torch.relu(d["x"])
    assert torch.equal(R.pool_fwd_reference(xr), y.detach())
    assert torch.equal(R.pool_bwd_reference(xr, d["dout"]), x.grad.permute(0, 2, 3, 1))
    # on the raw integers: forward is a plain maximum, backward gates on a positive maximum and picks the first one
    raw = d["x"].double().permute(0, 3, 1, 2)
    val, idx = F.max_pool2d(raw, 2, 2, return_indices=True)
    assert torch.equal(R.pool_fwd_reference(d["x"]), val.reshape(R.POOL_N, -1))
    g = torch.where(val > 0, d["dout"].double().reshape(val.shape), torch.zeros_like(val))
    want = torch.zeros(R.POOL_N, 64, H * W, dtype=torch.float64).scatter_(2, idx.reshape(R.POOL_N, 64, -1), g.reshape(R.POOL_N, 64, -1))
    assert torch.equal(R.pool_bwd_reference(d["x"], d["dout"]), want.reshape(R.POOL_N, 64, H, W).permute(0, 2, 3, 1))
    best, bi = R.pool_scan(d["x"])
    assert float(best[0, 0, 0, 0]) == 0 and float(best[0, 0, 0, 1]) == -1 and float(best[0, 0, 0, 2]) == 3 and int(bi[0, 0, 0, 2]) == 0


@pytest.mark.parametrize("n", R.LOSS_N)
@pytest.mark.parametrize("A", R.LOSS_A)
def test_loss_equals_cross_entropy(n, A):
    d = R.loss_data(n, A)
    z = d["logits"].double().requires_grad_(True)
    ce = F.cross_entropy(z, d["answers"], reduction="none")
    ok = d["valid"] != 0
    (torch.where(ok, ce, torch.zeros_like(ce)).sum() * d["scale"]).backward()
    ref = R.loss_reference(d)
    torch.testing.assert_close(ref["loss"], torch.where(ok, ce.detach(), torch.full_like(ce, 3.33).detach()), rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref["dlogits"], z.grad, rtol=1e-11, atol=1e-15)
    first = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in d["logits"]])
    assert torch.equal(ref["predictions"], torch.where(ok, first, torch.full_like(first, d["unknown"])))
    if A >= 2 and n > 2:
        assert int((d["logits"] == d["logits"].max(1, keepdim=True).values).sum(1).max()) >= 2      # tied maxima exist
        assert float(d["logits"].abs().max()) == 80.0
    nov = R.loss_reference(d, "valid")
    torch.testing.assert_close(nov["loss"], ce.detach(), rtol=1e-11, atol=1e-13)
    noa = R.loss_reference(d, "answers")
    torch.testing.assert_close(noa["loss"], torch.where(ok, -F.log_softmax(z.detach(), 1).max(1).values, torch.full_like(ce, 3.33).detach()),
                               rtol=1e-11, atol=1e-13)
    assert float(noa["dlogits"].abs().max()) == 0.0


@pytest.mark.parametrize("clamp", R.ADAM_CLAMP)
@pytest.mark.parametrize("wd", R.ADAM_WD)
def test_adam_equals_torch_optim_adam(clamp, wd):
    """torch.optim.Adam in float64 from the same state and step count, three steps, at the hyperparameters the kernel holds
    (rounded to float32: include/probnmn_hip.h); and the float32 run of the reference is the yardstick of the GPU test: its
    err32 is printed.  The rounding matters for one number: 1 - f32(0.999) is 1.3e-5 of itself away from 1 - 0.999."""
    h = {k: R.f32(v) for k, v in R.ADAM_HYPER.items()}
    assert abs((1 - h["beta2"]) / (1 - R.ADAM_HYPER["beta2"]) - 1) == pytest.approx(1.287e-5, rel=1e-2)
    for it in R.adam_data():
        p = it["param"].double().clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=h["lr"], eps=h["eps"], weight_decay=R.f32(wd), betas=(h["beta1"], h["beta2"]))
        opt.state[p] = dict(step=torch.tensor(float(it["first"] - 1)), exp_avg=it["exp_avg"].double().clone(),
                            exp_avg_sq=it["exp_avg_sq"].double().clone())
        for k in range(R.ADAM_STEPS):
            g = it["grads"][k].double()
            p.grad = g.clamp(-clamp, clamp) if clamp > 0 else g.clone()
            opt.step()
        ref = R.adam_reference(it, clamp, wd, bc_betas=(h["beta1"], h["beta2"]))
        torch.testing.assert_close(ref["param"], p.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(ref["exp_avg"], opt.state[p]["exp_avg"], rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(ref["exp_avg_sq"], opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=1e-14)
        ref = R.adam_reference(it, clamp, wd)
        r32 = R.adam_reference(it, clamp, wd, dtype=torch.float32)
        print("\n[adam err32] n %d clamp %g wd %g: " % (it["n"], clamp, wd)
              + " ".join("%s %.2e" % (k, float((r32[k].double() - ref[k]).abs().max() / ref[k].abs().max())) for k in ref))


def test_transpose_and_layout_are_permutations():
    for shape in R.WTRANS_SHAPES[:5]:
        src = R.wtrans_data(shape)
        cout, taps, cin = shape
        dst = R.wtrans_reference(src)
        assert dst.shape == (cin, taps, cout)
        for (co, t, ci) in ((0, 0, 0), (cout - 1, 0, cin - 1), (cout // 2, taps - 1, cin // 3)):
            assert float(dst[ci, taps - 1 - t, co]) == float(src[co, t, ci])
    x = R.layout_data(5, 3, 49)
    assert torch.equal(R.to_nhwc_reference(x, [4, 2, 0])[1, 7], x[2, :, 7])


def test_exact_data_is_exact_in_float32():
    """What exact_ok promises: the float32 run of an exact reference has the float64 run's values."""
    d = R.maskbwd_data(196)
    for a, b in zip(R.maskbwd_reference(d), R.maskbwd_reference(d, dtype=torch.float32)):
        assert torch.equal(a, b.double())
    name, n_ex, HW, counts = R.GATHER_CASES[1]
    g = R.gather_data(n_ex, HW)
    assert torch.equal(R.gather_reference(g, counts), R.gather_reference(g, counts, dtype=torch.float32).double())
    for it in R.minmax_data(98):
        for a, b in zip(R.minmax_bwd_reference(it), R.minmax_bwd_reference(it, dtype=torch.float32)):
            assert torch.equal(a, b.double())
    with pytest.raises(AssertionError):
        R.exact_ok(2.0 ** 24, "too large")


# ---------------------------------------------------------------------------------------------------------------------
# launch shapes
# ---------------------------------------------------------------------------------------------------------------------
PLAN_MAIN = r"""
#include <stdio.h>
#include "pointwise_plan.h"
int main() {
    int a, b;
    char what;
    while (scanf(" %c %d %d", &what, &a, &b) == 3) {
        if (what == 'l') printf("%d\n", pnmn::layout_chunk(a));
        if (what == 'p') printf("%d %d %zu %d\n", pnmn::pool_band(a, b), pnmn::pool_bwd_even_rows(a, b), pnmn::pool_bwd_even_lds(a, b),
                                (int)pnmn::pool_bwd_takes_even(a, b));
        if (what == 'g') printf("%d\n", pnmn::gather_parts(a, b));
        if (what == 't') printf("%d %d\n", pnmn::wtrans_tiles(a, b, 9), pnmn::WTRANS_GRID);
    }
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_rules_restate_the_compiled_header(tmp_path):
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "probnmn-clevr_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    asks = [("l", hw, 0) for hw in list(range(1, 2000)) + [3136, 12544, 50176]]
    asks += [("p", h, w) for h in range(2, 61) for w in list(range(2, 80)) + [112, 224, 448]]
    asks += [("g", n, hw) for n in list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 511, 512, 513] for hw in list(range(1, 200)) + [784]]
    asks += [("t", a, b) for a in (1, 3, 32, 33, 128, 256, 1024) for b in (1, 5, 65, 128)]
    got = subprocess.run([str(exe)], input="".join("%s %d %d\n" % a for a in asks), capture_output=True, text=True, check=True)
    lines = got.stdout.strip().split("\n")
    assert len(lines) == len(asks)
    for (what, a, b), line in zip(asks, lines):
        v = [int(t) for t in line.split()]
        if what == "l":
            mine = [R.layout_chunk(a)]
        elif what == "p":
            mine = [R.pool_band(a, b), R.pool_bwd_even_rows(a, b), R.pool_bwd_even_lds(a, b), int(R.pool_bwd_takes_even(a, b))]
        elif what == "g":
            mine = [R.gather_parts(a, b)]
        else:
            mine = [R.wtrans_tiles(a, b, 9), R.WTRANS_GRID]
        assert mine == v, "%s(%d, %d): %s here, %s from pointwise_plan.h" % (what, a, b, mine, v)


def test_the_engine_shapes_launch_as_before():
    """14x14 and 28x28, the shapes every network launch has: one layout chunk / two of 392, one pool band / two of 14 rows, the
    even backward with 7 pooled rows, eight pixel ranges per example below 64 examples."""
    assert (R.layout_chunk(196), R.layout_chunk(784)) == (196, 392)
    assert (R.pool_band(14, 14), R.pool_band(28, 28)) == (14, 14)
    assert all(R.pool_bwd_takes_even(s, s) and R.pool_bwd_even_rows(s, s) == 7 for s in (14, 28))
    assert (R.pool_bwd_even_lds(14, 14), R.pool_bwd_even_lds(28, 28)) == (7 * 7 * 260, 7 * 14 * 260)
    assert [R.gather_parts(n, 196) for n in (1, 7, 64, 128, 256, 512)] == [8, 8, 8, 4, 2, 1]


def test_the_two_launch_defects_by_arithmetic():
    """What the parent commit's launch code asked for, and what it asks for now.
    Transposition: a fixed grid of 256 tiles and `return` past an item's tiles left [256][9][128] (288 tiles) partly unwritten.
    Even max-pool backward: 7 pooled rows whatever the map has, 7 * 37 * 65 * 4 = 67 340 bytes of LDS at 4x74 and 14x74 with
    no opt-in -- above the 64 KB a launch gets."""
    assert R.wtrans_tiles(256, 128, 9) == 288 > R.WTRANS_GRID
    assert all(R.wtrans_tiles(co, ci, t) <= R.WTRANS_GRID for (co, t, ci) in R.WTRANS_SHAPES[:5])
    for (H, W) in ((4, 74), (14, 74)):
        assert 7 * (W // 2) * 65 * 4 == 67340 > R.LDS_NO_OPT_IN
    assert R.pool_bwd_even_rows(4, 74) == 2 and R.pool_bwd_takes_even(4, 74) and R.pool_bwd_even_lds(4, 74) == 19240
    assert not R.pool_bwd_takes_even(14, 74) and R.pool_band(14, 74) * 74 * 65 * 4 <= R.LDS_BUDGET
    for H in range(2, 61):
        for W in range(2, 120):
            assert not R.pool_bwd_takes_even(H, W) or R.pool_bwd_even_lds(H, W) <= R.LDS_NO_OPT_IN


def test_coverage():
    """What the GPU case lists reach, from the restated rules alone: a later edit of a list cannot quietly drop a branch."""
    # max-pool: the generic backward, left-over row and column, a short last band (H = 29: bands of 8, the last of 5 rows),
    # the even kernel with one and two bands and with fewer than 7 pooled rows, an even map on the generic kernel
    bwd = set().union(*[R.pool_facts(H, W, True) for H, W in R.POOL_MAPS])
    fwd = set().union(*[R.pool_facts(H, W, False) for H, W in R.POOL_MAPS])
    assert {"generic kernel", "row left over", "column left over", "generic short last band", "generic bands 1", "generic bands 3", "even kernel",
            "even bands 1", "even bands 2", "even PRB below 7 at more than 64 positions", "even map on the generic kernel"} <= bwd, bwd
    assert {"generic kernel", "row left over", "column left over", "generic short last band", "generic bands 1", "generic bands 2", "generic bands 3"} <= fwd, fwd
    assert R.pool_band(29, 29) == 8 and 29 % 8 == 5
    assert "even PRB below 7 at more than 64 positions" in R.pool_facts(4, 74, True) and "even map on the generic kernel" in R.pool_facts(14, 74, True)
    assert set(R.POOL_C) == {64, 128}
    # gather: every count, the four-way loop with and without a tail, parts 8, 4, 2, 1, empty ends, mixed groups of four
    gf = set().union(*[R.gather_facts(n, hw, counts) for _, n, hw, counts in R.GATHER_CASES])
    assert {"count %d" % k for k in (0, 1, 3, 4, 5, 8, 9)} <= gf
    assert {"parts 8", "parts 4", "parts 2", "parts 1", "four in flight", "tail after four", "first and last empty",
            "NULL and non-NULL attn in one group of four"} <= gf, gf
    assert [R.gather_parts(n, 196) for n in (1, 7, 128, 256, 512)] == [8, 8, 4, 2, 1]
    assert {n for _, n, hw, _ in R.GATHER_CASES if hw == 196} >= {1, 7, 128, 256, 512}
    assert {hw for _, _, hw, _ in R.GATHER_CASES} >= {47, 48, 96, 196, 784}
    for _, n, hw, counts in R.GATHER_CASES:
        assert len(counts) == n and (n < 128 or sum(counts) <= 16)
    # layout: both load widths, vector and both scalar channel paths, one, two and three chunks, the 447 / 448 boundary
    lf = set().union(*[R.layout_facts(Cn, HW) for Cn in R.LAYOUT_C for HW in R.LAYOUT_HW])
    assert {"load16", "load4", "load4 at HW % 4 == 0", "vector channels", "scalar channels, cw < 64", "scalar channels, C % 4 != 0", "chunks 1",
            "chunks 2", "chunks 3"} <= lf, lf
    assert R.layout_chunk(447) == 447 and R.layout_chunk(448) == 224 and {447, 448} <= set(R.LAYOUT_HW)
    assert set(R.LAYOUT_C) >= {1, 3, 64, 66, 68, 128, 132} and set(R.LAYOUT_HW) >= {1, 3, 4, 49, 196, 447, 448, 785, 900}
    rf = set().union(*[R.layout_facts(Cn, HW) for Cn, HW in R.LAYOUT_ROWS_SHAPES])
    assert {"load16", "load4", "vector channels", "scalar channels, cw < 64", "chunks 2", "chunks 3"} <= rf
    # transposition: square and not, partial tiles, an item with more tiles than the grid and items with fewer in one launch
    tiles = [R.wtrans_tiles(co, ci, t) for (co, t, ci) in R.WTRANS_SHAPES]
    assert max(tiles) > R.WTRANS_GRID > min(tiles) and any(co % 32 or ci % 32 for (co, t, ci) in R.WTRANS_SHAPES)
    assert any(co != ci for (co, t, ci) in R.WTRANS_SHAPES)
    # partial rounds: 104 pixels per forward round and 56 per backward round of the head, 98 per forward round of And / Or
    assert {1, 56, 57, 104, 105, 196, 209, 784} <= set(R.DOT1_HW) and {1, 97, 98, 99, 196, 784} <= set(R.MINMAX_HW)
    assert {1, 7, 196, 784} <= set(R.SAME_HW) and {1, 9, 196, 784} <= set(R.MASKBWD_HW)
    assert set(R.same_kinds(784)) == {"random", "last", "allequal", "nodattn", "tie255_256", "tie0_783"}
    assert R.SAME_TIES["tie255_256"] == (255, 256)      # threads 255 and 0 of a 256-thread scan
    assert len(R.MINMAX_ITEMS) == 8 and {(a, b) for a, b, _ in R.MINMAX_ITEMS} == {(1, 1), (1, C), (C, 1), (C, C)}
    # tails and sizes
    assert set(R.AXPY_N) >= {1, 3, 4, 5, 1023, 25088, 25091} and set(R.ADAM_N) >= {1, 3, 4, 5, 1031, 100003}
    assert len(set(R.ADAM_FIRST_STEP)) == len(R.ADAM_N) and set(R.ADAM_BLOCKS) == {1, 3, 2048}
    assert set(R.ADAM_CLAMP) == {0.0, 5.0} and set(R.ADAM_WD) == {0.0, 0.01}
    assert set(R.LOSS_N) == {1, 64, 65} and set(R.LOSS_A) == {1, 2, 28} and set(R.LOSS_NULLS) == {"none", "valid", "predictions", "answers", "dlogits"}
