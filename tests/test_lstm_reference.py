"""The LSTM layer / stack / cell reference checked on the CPU (tests/helpers/lstm_reference.py): its backward against central
differences, the stack against torch.nn.LSTM(num_layers=2), and every case of the tables against the deliberately wrong rules
-- a case whose inputs cannot tell a wrong rule from the right one by 100 times its own error bar checks little on the GPU and
is not allowed in the table, unless the table of exemptions says why it cannot see that rule (then the two must agree).

What the wrong rules show.  ``stale_h`` and ``gate_order`` move the forward tensors from the first step they apply to;
``no_cell_carry`` and ``no_recurrent_grad`` leave the forward where it is and move dgates of every step but the last."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_reference as lr  # noqa: E402

NAMES = [c["name"] for c in lr.CASES]
STACK_NAMES = [c["name"] for c in lr.STACK_CASES]


def _small(remembering, seed):
    """Hidden 4, B = 3, T = 4, float64."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).double()  # noqa: E731
    h, B, T = 4, 3, 4
    xp = r(B, T, 4 * h, scale=0.7)
    if remembering:
        xp[..., :h] += 1.0
        xp[..., h:2 * h] += 4.0
    return xp, r(4 * h, h, scale=0.4), r(B, T, h)


@pytest.mark.parametrize("remembering,steps", [(False, None), (True, [4, 1, 3])])
def test_reference_backward_matches_central_differences(remembering, steps):
    """loss = sum(hs * dhs) over the valid steps: dgates (= d loss / d xp) against (loss(x + e) - loss(x - e)) / 2e of every
    element of xp."""
    xp, w_hh, dhs = _small(remembering, 7 + remembering)
    ref = lr.layer_reference(xp, w_hh, dhs, steps)
    valid = lr._valid(steps, 3, 4, torch.float64)

    def loss(x):
        return float((lr.layer_reference(x, w_hh)["hs"] * dhs * valid).sum())

    eps, num = 1e-6, torch.zeros_like(xp)
    for idx in np.ndindex(*xp.shape):
        hi, lo = xp.clone(), xp.clone()
        hi[idx] += eps
        lo[idx] -= eps
        num[idx] = (loss(hi) - loss(lo)) / (2 * eps)
    assert float(ref["dgates"].abs().max()) > 0.01
    assert float((num - ref["dgates"]).abs().max()) <= 1e-7 * max(1.0, float(ref["dgates"].abs().max()))
    if steps is not None:  # nothing flows back into the steps behind a row's last
        assert float((ref["dgates"] * (1 - valid)).abs().max()) == 0.0 and float(ref["dgates"][1, 0].abs().max()) > 0.0


def test_cell_reference_matches_central_differences_and_takes_absent_gradients():
    g = torch.Generator().manual_seed(3)
    gates, c_prev = torch.randn(2, 12, generator=g).double(), torch.randn(2, 3, generator=g).double()
    dh, dc = torch.randn(2, 3, generator=g).double(), torch.randn(2, 3, generator=g).double()
    ref = lr.cell_reference(gates, c_prev, dh, dc)

    def loss(gt, cp):
        out = lr.cell_reference(gt, cp)
        return float((out["h"] * dh).sum() + (out["c"] * dc).sum())

    eps = 1e-6
    for base, got, at in ((gates, ref["dgates"], 0), (c_prev, ref["dc_prev"], 1)):
        for idx in np.ndindex(*base.shape):
            hi, lo = base.clone(), base.clone()
            hi[idx] += eps
            lo[idx] -= eps
            num = (loss(hi, c_prev) - loss(lo, c_prev)) / (2 * eps) if at == 0 else (loss(gates, hi) - loss(gates, lo)) / (2 * eps)
            assert abs(num - float(got[idx])) <= 1e-7, (at, idx)
    only_dh, only_dc, none = lr.cell_reference(gates, c_prev, dh), lr.cell_reference(gates, c_prev, None, dc), lr.cell_reference(gates, c_prev)
    for k in ("dgates", "dc_prev"):  # the loss is linear in (dh, dc_in)
        assert torch.allclose(only_dh[k] + only_dc[k], ref[k], rtol=0, atol=1e-14)
        assert float(none[k].abs().max()) == 0.0
    assert float(only_dc["dgates"][:, 9:].abs().max()) == 0.0  # (without dh the output gate gets nothing)


def test_stack_reference_without_dropout_is_nn_lstm_with_two_layers():
    """float64, hidden 5: the first layer's input projection is the identity (input size 4h, W_ih = I, no bias), so that the
    module's input gradient is dg1; dg2 is held through the bias and W_hh gradients of the second layer."""
    h, B, T = 5, 3, 6
    g = torch.Generator().manual_seed(5)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).double()  # noqa: E731
    xp, w_hh1, w_ih2, b2, w_hh2, dhs2 = r(B, T, 4 * h), r(4 * h, h, scale=0.4), r(4 * h, h, scale=0.4), r(4 * h), r(4 * h, h, scale=0.4), r(B, T, h)
    ref = lr.stack_reference(xp, w_hh1, w_ih2, b2, w_hh2, dhs2)
    lstm = torch.nn.LSTM(4 * h, h, num_layers=2, batch_first=True).double()
    with torch.no_grad():
        for name, value in (("weight_ih_l0", torch.eye(4 * h)), ("weight_hh_l0", w_hh1), ("bias_ih_l0", torch.zeros(4 * h)),
                            ("bias_hh_l0", torch.zeros(4 * h)), ("weight_ih_l1", w_ih2), ("weight_hh_l1", w_hh2), ("bias_ih_l1", b2),
                            ("bias_hh_l1", torch.zeros(4 * h))):
            getattr(lstm, name).copy_(value)
    x = xp.clone().requires_grad_(True)
    out, (h_n, c_n) = lstm(x)
    (out * dhs2).sum().backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))  # noqa: E731
    assert close(ref["hs2"], out.detach()) and close(ref["hs1"][:, -1], h_n[0].detach()) and close(ref["cs1"][:, -1], c_n[0].detach())
    assert close(ref["cs2"][:, -1], c_n[1].detach()) and torch.equal(ref["hsd"], ref["hs1"])
    assert close(ref["dg1"], x.grad)
    assert close(ref["dg2"].sum((0, 1)), lstm.bias_ih_l1.grad)
    assert close(torch.einsum("btg,bth->gh", ref["dg2"], ref["hsd"]), lstm.weight_ih_l1.grad)
    assert close(torch.einsum("btg,bth->gh", ref["dg2"][:, 1:], ref["hs2"][:, :-1]), lstm.weight_hh_l1.grad)
    assert close(torch.einsum("btg,bth->gh", ref["dg1"][:, 1:], ref["hs1"][:, :-1]), lstm.weight_hh_l0.grad)


def test_the_tables_cover_what_they_must():
    col = lambda k: [c[k] for c in lr.CASES]  # noqa: E731
    assert len(lr.CASES) == 12 and len(set(NAMES)) == 12
    assert set(col("B")) == {1, 15, 16, 17, 33, 144, 260, 520} and set(col("T")) == {1, 2, 3, 9, 46}
    assert col("form").count("tokens") == 6 and col("ragged").count(True) == 7
    for regime in ("typical", "saturated", "remembering"):
        assert col("regime").count(regime) >= 3
    for c in lr.CASES:
        i = lr.case_inputs(c["name"])
        steps, T = i["steps"], c["T"]
        assert (len(set(steps.tolist())) > 1) == c["ragged"] and steps.max() == T
        valid = torch.arange(T)[None, :] < torch.as_tensor(steps)[:, None]
        assert float(i["dhs"][~valid].abs().max() if (~valid).any() else 0.0) == 0.0
        if c["ragged"]:
            assert steps[0] == T and steps[1] == 1
            tile_steps, of_row = lr.row_tile_steps(steps, T)[1:]
            assert c["B"] <= 16 or tile_steps.min() < T  # every multi-tile ragged case has a tile that stops early
            assert (steps < of_row).any()
        if c["form"] == "tokens":
            table, tokens = i["x"]
            assert table.shape == (lr.V, 4 * lr.H) and tokens.shape == (c["B"], T) and tokens.stride(0) == T + 3
            assert T == 1 or bool((tokens[:, -1] != tokens[:, -2]).all())
    assert [(c["B"], c["T"], c["form"], c["p"], c["row_offset"]) for c in lr.STACK_CASES] == [
        (1, 1, "xp", 0.0, 0), (17, 2, "tokens", 0.3, 5), (33, 9, "tokens", 0.0, 0), (16, 9, "xp", 1.0, 0), (40, 3, "tokens", 0.5, 2 ** 33)]


@pytest.mark.parametrize("name", [c["name"] for c in lr.CASES if c["regime"] != "typical"])
def test_regimes_are_what_they_say(name):
    """saturated: |c| passes 3 where the case has the steps for it (|c| <= T); remembering: c accumulates over the steps."""
    case, ref = next(c for c in lr.CASES if c["name"] == name), lr.case_reference(name)
    peak = float(ref["cs"].abs().max())
    print(name, "max |c| %.3g" % peak)
    if case["regime"] == "saturated":
        railed = ((ref["act"][..., :lr.H] - 0.5).abs() > 0.45).double().mean()  # input gates outside (0.05, 0.95)
        assert peak > min(3.0, 0.9 * case["T"]) and float(railed) > 0.25
    else:
        assert peak > 0.35 * case["T"] + 0.5


@pytest.mark.parametrize("name", [c["name"] for c in lr.CASES if c["ragged"]])
def test_ordered_reference_equals_the_plain_one_wherever_the_tile_runs(name):
    i = lr.case_inputs(name)
    T = i["dhs"].size(1)
    plain = lr.case_reference(name)
    cut = lr.layer_reference(i["x"], i["w_hh"], i["dhs"], i["steps"], ordered=True)
    ran = torch.arange(T)[None, :] < torch.as_tensor(lr.row_tile_steps(i["steps"], T)[2])[:, None]
    for k in lr.LAYER:
        assert torch.equal(cut[k][ran], plain[k][ran]), k
    for k in lr.ZEROED:
        assert (~ran).sum() == 0 or float(cut[k][~ran].abs().max()) == 0.0, k
    if (~ran).any():
        assert float(plain["hs"][~ran].abs().max()) > 0.0  # (the zeros are the order's, not the recurrence's)


def _no_bar_at_the_ceiling(name, bars):
    for k, (scale, bar) in bars.items():
        print("%s %s: scale %.3g, bar %.3g" % (name, k, scale, bar))
        assert lr.FLOOR <= bar < lr.CEILING, (name, k, bar)


@pytest.mark.parametrize("name", NAMES)
def test_no_layer_bar_sits_at_the_ceiling(name):
    _no_bar_at_the_ceiling(name, lr.case_bars(name))
    if next(c for c in lr.CASES if c["name"] == name)["ragged"]:
        _no_bar_at_the_ceiling(name + " ordered", lr.case_bars(name, ordered=True))


@pytest.mark.parametrize("name", STACK_NAMES)
def test_no_stack_bar_sits_at_the_ceiling(name):
    bars = lr.stack_case_bars(name)
    p = next(c for c in lr.STACK_CASES if c["name"] == name)["p"]
    assert [k for k, (scale, _) in bars.items() if scale == 0.0] == (["hsd", "dg1"] if p == 1.0 else [])
    _no_bar_at_the_ceiling(name, bars)


def _moved(ref, wrong, bars):
    """The largest move of a tensor under a wrong rule, in units of the case's error bar for that tensor."""
    moves = [(float((wrong[k] - ref[k]).abs().max()) / scale / bar, k) for k, (scale, bar) in bars.items() if scale > 0]
    return max(moves, key=lambda m: m[0])


def _tell(name, rule, exempt, ratio, k):
    print(name, "%s moves %s by %.3g bars" % (rule, k, ratio))
    if name in exempt[rule]:
        assert ratio == 0.0  # (the case cannot see the rule: the two are one)
    else:
        assert ratio > 100.0


@pytest.mark.parametrize("rule", lr.LAYER_RULES)
@pytest.mark.parametrize("name", NAMES)
def test_layer_inputs_tell_a_wrong_rule_from_the_right_one(name, rule):
    _tell(name, rule, lr.EXEMPT, *_moved(lr.case_reference(name), lr.case_reference(name, rule=rule), lr.case_bars(name)))


@pytest.mark.parametrize("rule", lr.LAYER_RULES + lr.STACK_RULES)
@pytest.mark.parametrize("name", STACK_NAMES)
def test_stack_inputs_tell_a_wrong_rule_from_the_right_one(name, rule):
    ref, wrong, bars = lr.stack_case_reference(name), lr.stack_case_reference(name, rule=rule), lr.stack_case_bars(name)
    pair = {k: v for k, v in bars.items() if k in lr.STACK}  # (the rider is a layer case of its own kind: judged on the pair)
    _tell(name, rule, lr.STACK_EXEMPT, *_moved(ref, wrong, pair))
