"""The float64 weight-gradient reference of tests/wgrad_reference.py against float64 CPU autograd of
F.conv2d(x * xmask, w, b, padding=d, dilation=d) + ReLU, and the property the exact GPU cases rest on: for the
integer-valued generator float32 autograd equals the float64 reference bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_reference as R


def close64(got, want):
    for g, w in zip(got, want):
        scale = max(1.0, float(w.abs().max()))
        assert float((g - w).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize("H", [14, 28])
@pytest.mark.parametrize("dilation", [1, 2, 4, 8])
def test_3x3_every_dilation(H, dilation):
    L = R.make_launch(H, 9, 1, 1, [2, 1], [0, 0], dilation, pools=R.normal_pools(dilation, H, H, 9, 128, 128))
    dw, db = R.reference(L)
    aw, ab = R.autograd_wgrad(L, torch.float64)
    close64(dw, aw)
    close64(db, ab)
    assert float(dw[0].abs().max()) > 1.0  # (not a comparison of zeros)


@pytest.mark.parametrize("H", [14, 28])
def test_through_autograds_own_relu(H):
    """Gate = the forward output, ReLU differentiated by autograd: the (gate > 0) of the formula is that backward."""
    g = torch.Generator().manual_seed(5)
    n, C = 3, 128
    pools = list(R.normal_pools(6, H, H, 9, C, C))
    w = (torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * C)) ** 0.5)
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    L = R.make_launch(H, 9, 1, 1, [n], [0], 2, pools=pools)
    x, _ = R._operands(L, np.arange(n), torch.float64, "cpu")
    y = F.relu(F.conv2d(x.reshape(n, H, H, C).permute(0, 3, 1, 2), w, b, padding=2, dilation=2))
    gate = torch.zeros_like(pools[3], dtype=torch.float64)
    gate[:n] = y.permute(0, 2, 3, 1).reshape(n, H * H, C)  # item i reads dy / gate map i (n <= PD)
    L.g_pool = gate
    dw, db = R.reference(L)
    aw, ab = R.autograd_wgrad(L, torch.float64, through_relu=[(w, b)])
    close64(dw, aw)
    close64(db, ab)
    zeros = float((gate[:n] == 0).double().mean())
    assert 0.2 < zeros < 0.8  # the gate does cut


@pytest.mark.parametrize("H", [14, 28])
def test_1x1_two_sources_and_wide_output(H):
    L = R.make_launch(H, 1, 2, 1, [2, 0, 3], [0, 1, 0], 1, two_sources=True, pools=R.normal_pools(7, H, H, 1, 256, 128))
    close64(R.reference(L)[0], R.autograd_wgrad(L, torch.float64)[0])
    L = R.make_launch(H, 1, 1, 4, [1, 2], [0, 1], 1, mask="some", gate="some", pools=R.normal_pools(8, H, H, 1, 128, 512))
    for got, want in zip(R.reference(L), R.autograd_wgrad(L, torch.float64)):
        close64(got, want)


@pytest.mark.parametrize("H", [14, 28])
def test_mixed_dilations_empty_jobs_and_missing_maps(H):
    """Dilations mixed inside jobs, empty jobs first / in the middle / last, a weight no job adds into, items without a
    mask or a gate."""
    orders = ([], [1, 2, 4, 8], [], [8, 1], [1, 1, 8, 8, 1], [])
    L = R.make_launch(H, 9, 1, 1, [len(o) for o in orders], [0, 1, 2, 0, 1, 0], lambda j, k: orders[j][k], mask="some",
                      gate="some", pools=R.normal_pools(9, H, H, 9, 128, 128))
    assert L.n_weights == 3 and len(L.items_of(2)) == 0
    dw, db = R.reference(L)
    aw, ab = R.autograd_wgrad(L, torch.float64)
    close64(dw, aw)
    close64(db, ab)
    assert float(dw[2].abs().max()) == 0.0 and float(db[2].abs().max()) == 0.0
    # per item dilation matters: the same launch at the first item's dilation is another gradient
    L1 = R.make_launch(H, 9, 1, 1, [len(o) for o in orders], [0, 1, 2, 0, 1, 0], lambda j, k: orders[j][0], mask="some",
                       gate="some", pools=R.normal_pools(9, H, H, 9, 128, 128))
    assert float((R.reference(L1)[0][0] - dw[0]).abs().max()) > 1.0


def test_shift_is_the_formulas():
    """shifted() against the definition, pixel by pixel."""
    H = W = 14
    x = torch.arange(H * W, dtype=torch.float64).reshape(1, H * W, 1) + 1
    for dil in (1, 2, 4, 8):
        for tap in range(9):
            s = R.shifted(x, H, W, tap, dil).reshape(H, W)
            for y in range(H):
                for xx in range(W):
                    yy, xs = y + (tap // 3 - 1) * dil, xx + (tap % 3 - 1) * dil
                    want = float(yy * W + xs + 1) if 0 <= yy < H and 0 <= xs < W else 0.0
                    assert float(s[y, xx]) == want


@pytest.mark.parametrize("n_items", [64, 512])
def test_integer_inputs_are_exact_in_float32(n_items):
    """The exact GPU cases compare with torch.equal: for the integer generator float32 autograd IS the float64 reference,
    and the sums stay far below 2^24."""
    counts = [n_items // 4] * 4
    L = R.make_launch(14, 9, 1, 1, counts, [0, 0, 0, 0], lambda j, k: (1, 2, 4, 8)[(j + k) % 4], mask="some", gate="some", seed=3)
    dw, db = R.reference(L, chunk=64)
    aw, ab = R.autograd_wgrad(L, torch.float32)
    assert torch.equal(aw[0].double(), dw[0]) and torch.equal(ab[0].double(), db[0])
    assert 100 < float(dw[0].abs().max()) < 2 ** 24 / 64 and float(db[0].abs().max()) < 2 ** 24 / 64
    assert 18 * 196 * n_items < 2 ** 24
    # -0.0 and 0.0 both close the gate, and both are among the gate values
    assert bool(((L.g_pool == 0) & torch.signbit(L.g_pool)).any()) and bool(((L.g_pool == 0) & ~torch.signbit(L.g_pool)).any())
