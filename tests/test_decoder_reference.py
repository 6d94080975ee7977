"""The decoder reference checked on the CPU (tests/helpers/decoder_reference.py): its backward against central differences,
and every case of the table against two deliberately wrong attention rules -- a case whose inputs cannot tell a wrong rule
from the right one by 100 times its own error bar checks little on the GPU and is not allowed in the table.

What the wrong rules show.  Apart from the 1e-13, softmax(score * mask) * mask / sum IS the softmax over the valid positions:
the exp(0) of the masked positions cancels in the second normalisation.  So rule (a) leaves weights and gradients where they
are and moves ``probs``, the softmax before masking that the forward saves and the backward starts from -- by the mass the
masked positions hold there.  Rule (b) moves the weights of a row by 1e-13 / Z, which only the faint cases can see."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_reference as dr  # noqa: E402

NAMES = [c["name"] for c in dr.CASES]


def _small():
    """Hidden 8, B = 4, S = 5, T = 3; mask lengths 5, 1, 0 (all zero) and 3."""
    g = torch.Generator().manual_seed(0)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).double()  # noqa: E731
    Hs, B, S, T = 8, 4, 5, 3
    mask = (torch.arange(S)[None, :] < torch.tensor([5, 1, 0, 3])[:, None]).double()
    d = dict(enc=r(B, S, Hs, scale=0.7), mask=mask, h0=r(B, Hs, scale=0.7), w_c=r(4 * Hs, Hs, scale=0.3), w_hh=r(4 * Hs, Hs, scale=0.3))
    return d, r(B, T, 4 * Hs), r(B, T, Hs), T


def test_reference_backward_matches_central_differences():
    """loss = sum(hs * dhs): the reference's denc, dh0 and dgates (= d xe) against (loss(x + e) - loss(x - e)) / 2e of every
    element, and dctx / dscore against the same difference with the perturbation added to that step's context / scores."""
    d, xe, dhs, T = _small()
    ref = dr.decoder_reference(d, T, xe=xe, dhs=dhs)
    for k in ("weights", "ctx", "denc", "dscore"):  # the all-zero mask row: weights 0, context 0, finite (zero) gradients
        assert float(ref[k][2].abs().max()) == 0.0, k
    assert bool(torch.isfinite(ref["dh0"]).all()) and float(ref["dh0"][2].abs().max()) > 0.0
    assert torch.allclose(ref["weights"][1, :, 0], torch.ones(T, dtype=torch.float64), atol=1e-12)  # (mask length 1)

    def loss(d2, xe2):
        return float((dr.decoder_reference(d2, T, xe=xe2)["hs"] * dhs).sum())

    eps = 1e-6
    for name, got in (("enc", ref["denc"]), ("h0", ref["dh0"]), ("xe", ref["dgates"])):
        base = xe if name == "xe" else d[name]
        num = torch.zeros_like(base)
        for idx in np.ndindex(*base.shape):
            hi, lo = base.clone(), base.clone()
            hi[idx] += eps
            lo[idx] -= eps
            args = [(d, hi), (d, lo)] if name == "xe" else [(dict(d, **{name: hi}), xe), (dict(d, **{name: lo}), xe)]
            num[idx] = (loss(*args[0]) - loss(*args[1])) / (2 * eps)
        assert float((num - got).abs().max()) <= 1e-7 * max(1.0, float(got.abs().max())), name
    # d ctx_t and d score_t are no gradients of an input.  The context enters the gates only, so dctx = dgates W_c; and the 40
    # entries of a row's denc = w^T dctx + dscore^T h_prev, checked above, pin down the 15 of its dscore
    hprev = torch.cat((d["h0"][:, None], ref["hs"][:, :-1]), 1)
    denc = torch.einsum("bts,bth->bsh", ref["weights"], ref["dctx"]) + torch.einsum("bts,bth->bsh", ref["dscore"], hprev)
    assert float((denc - ref["denc"]).abs().max()) <= 1e-12 * float(ref["denc"].abs().max())
    assert float((ref["dctx"] - ref["dgates"] @ d["w_c"]).abs().max()) <= 1e-12 * float(ref["dctx"].abs().max())


def test_steps_zero_the_gradient_behind_a_row_and_the_tails_behind_a_tile():
    d, xe, dhs, T = _small()
    steps = np.array([3, 1, 2, 1])
    ref = dr.decoder_reference(d, T, xe=xe, dhs=dhs, steps=steps)
    valid = torch.arange(T)[None, :] < torch.as_tensor(steps)[:, None]
    for k in ("dgates", "dctx", "dscore"):
        assert float(ref[k][~valid].abs().max()) == 0.0 and float(ref[k][valid].abs().max()) > 0.0, k
    order, tile_steps, of_row = dr.row_tile_steps(np.array([2, 9, 0] + [5] * 15 + [3]), 7)
    assert order[:3].tolist() == [1, 3, 4] and tile_steps.tolist() == [7, 3] and of_row[[0, 1, 2, 17, 18]].tolist() == [3, 7, 3, 7, 3]
    cut = dr.zero_tails(ref, np.array([2, 1, 2, 1]), T)  # one tile of two steps
    for k in dr.ZEROED:
        assert float(cut[k][:, 2:].abs().max()) == 0.0 and torch.equal(cut[k][:, :2], ref[k][:, :2]), k
    for k in dr.UNWRITTEN + ("dh0", "denc"):
        assert cut[k] is ref[k]


def test_the_table_covers_what_it_must():
    col = lambda k: [c[k] for c in dr.CASES]  # noqa: E731
    assert 12 <= len(dr.CASES) <= 16 and len(set(NAMES)) == len(NAMES)
    assert set(col("S")) == {1, 2, 7, 9, 33, 58, 59, 60, 63, 64} and set(col("B")) == {1, 15, 16, 17, 33}
    assert set(col("T")) == {1, 2, 9, 64}
    assert [c["B"] <= 17 for c in dr.CASES if c["T"] == 64] == [True]
    for form in ("xe", "tokens"):
        assert col("form").count(form) >= 2
    for regime in ("diffuse", "saturated", "faint"):
        assert col("regime").count(regime) >= 3
    assert col("zero_row").count(True) >= 2 and col("ragged").count(True) >= 2
    assert 4 * len(dr.EXEMPT) <= len(dr.CASES)
    for c in dr.CASES:
        mask = dr.case_inputs(c["name"])["d"]["mask"]
        lens = mask.sum(1).long()
        assert torch.equal(mask, (torch.arange(c["S"])[None, :] < lens[:, None]).float())  # prefixes
        assert (c["name"] in dr.EXEMPT) == bool((lens == c["S"]).all())
        if c["B"] > 1:
            assert lens[:3].tolist() == [c["S"], 1, max(1, c["S"] - 1)][:c["B"]]
        assert bool((lens == 0).any()) == c["zero_row"]
        steps = dr.case_inputs(c["name"])["steps"]
        assert (len(set(steps.tolist())) > 1) == c["ragged"] and steps.max() == c["T"]
        if c["ragged"]:  # some tile stops early, and some row stops before its tile does
            of_row = dr.row_tile_steps(steps, c["T"])[2]
            assert of_row.min() < c["T"] or c["B"] <= 16
            assert (steps < of_row).any()


@pytest.mark.parametrize("name", [c["name"] for c in dr.CASES if c["regime"] == "faint"])
def test_faint_cases_are_faint(name):
    """Median over the rows of Z = sum(p * mask) at step 0, rows with an all-zero mask left out."""
    i = dr.case_inputs(name)
    probs, mask = dr.case_reference(name)["probs"], i["d"]["mask"].double()
    z = (probs[:, 0] * mask).sum(1)[mask.sum(1) > 0]
    print(name, "Z at step 0: median %.3g, min %.3g, max %.3g" % (float(z.median()), float(z.min()), float(z.max())))
    assert dr.FAINT_Z[0] <= float(z.median()) <= dr.FAINT_Z[1]


def _moved(name, rule):
    """The largest move of a compared tensor under a wrong rule, in units of the case's error bar for that tensor."""
    ref, wrong, bars = dr.case_reference(name), dr.case_reference(name, rule=rule), dr.case_bars(name)
    rows = dr.case_inputs(name)["d"]["mask"].sum(1) > 0  # (a row with an all-zero mask divides by zero without the 1e-13)
    worst = (0.0, None)
    for k in dr.FWD + dr.BWD:
        scale, bar = bars[k]
        if scale > 0:
            worst = max(worst, (float((wrong[k][rows] - ref[k][rows]).abs().max()) / scale / bar, k))
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_inputs_tell_the_plain_softmax_from_the_masked_one(name):
    ratio, k = _moved(name, "plain_softmax")
    print(name, "plain softmax moves %s by %.3g bars" % (k, ratio))
    if name in dr.EXEMPT:
        assert ratio <= 1.0  # (every row unmasked: the two rules are one)
    else:
        assert ratio > 100.0


@pytest.mark.parametrize("name", [c["name"] for c in dr.CASES if c["regime"] == "faint"])
def test_inputs_tell_the_dropped_epsilon(name):
    ratio, k = _moved(name, "no_epsilon")
    print(name, "no 1e-13 moves %s by %.3g bars" % (k, ratio))
    assert ratio > 100.0
