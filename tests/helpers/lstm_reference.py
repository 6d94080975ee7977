"""The LSTM layer over a padded sequence, the two-layer stack with dropout between the layers and the single cell step, forward
and backward, as plain torch on the host: the statement of the operation the recurrent layer kernels are held to
(include/probnmn_hip.h beside pnmn_lstm_seq_fwd, pnmn_lstm_stack_fwd, pnmn_lstm_dropout and pnmn_lstm_cell_fwd), the case
tables the CPU and the GPU test share, and the error bar (that of decoder_reference.py, imported).

Nothing here knows how the kernels compute: the backward is autograd through the forward with the gate pre-activations of
every step retained, in float64.  The same function in float32 gives the round-off a float32 evaluation of the recurrence
has on a case, from which the bar is derived."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/: lstm_dropout_ref, token_choice
import lstm_dropout_ref  # noqa: E402
from decoder_reference import CEILING, FACTOR, FLOOR, error_bars, row_tile_steps  # noqa: E402,F401

H, V = 256, 20
LAYER = ("hs", "cs", "act", "dgates")
STACK = ("hs1", "hsd", "cs1", "act1", "hs2", "cs2", "act2", "dg2", "dg1")
CELL = ("h", "c", "act", "dgates", "dc_prev")
ZEROED = ("hs", "dgates")   # zero from the tile's steps on under an order
UNWRITTEN = ("cs", "act")   # left unwritten there
# The right rule and the deliberately WRONG ones, there to show that a case's inputs can tell them from the right one:
#   stale_h            the recurrent product of step t >= 2 reads h_{t-2} (what a missed hand-off between steps looks like;
#                      step 1 has nothing staler than h_0 to read)
#   no_cell_carry      c_{t-1} is detached in the cell update: the backward loses dc_{t-1} = dc_t f_t
#   no_recurrent_grad  h_{t-1} is detached in the gate product: the backward loses dgates_t W_hh
#   gate_order         g and o change places
#   unscaled_mask      (stack) the dropout mask keeps without the 1 / (1 - p)
#   no_bias            (stack) the second layer drops b
LAYER_RULES = ("stale_h", "no_cell_carry", "no_recurrent_grad", "gate_order")
STACK_RULES = ("unscaled_mask", "no_bias")


def _cell(gates, c_prev, rule):
    """(h, c, act) of one step; act in the order i, f, g, o."""
    i, f, g, o = gates.chunk(4, 1)
    if rule == "gate_order":
        g, o = o, g
    act = torch.cat((torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)), 1)
    i, f, g, o = act.chunk(4, 1)
    c = f * (c_prev.detach() if rule == "no_cell_carry" else c_prev) + i * g
    return o * torch.tanh(c), c, act


def _layer(x, w_hh, rule):
    """The recurrence over x [B,T,4h] from h_0 = c_0 = 0: lists over the steps of h, c, act and the gate pre-activations."""
    B, T, hidden = x.size(0), x.size(1), w_hh.size(1)
    zero = x.new_zeros(B, hidden)
    h, c, out = [], zero, dict(hs=[], cs=[], act=[], gates=[])
    for t in range(T):
        prev = zero if t == 0 else h[max(t - 2, 0) if rule == "stale_h" else t - 1]
        gates = x[:, t] + (prev.detach() if rule == "no_recurrent_grad" else prev) @ w_hh.t()
        if gates.requires_grad:
            gates.retain_grad()
        h_t, c, act = _cell(gates, c, rule)
        h.append(h_t)
        for k, v in zip(("hs", "cs", "act", "gates"), (h_t, c, act, gates)):
            out[k].append(v)
    return out


def _valid(steps, B, T, dtype):
    st = np.full(B, T) if steps is None else np.asarray(steps)
    return (torch.arange(T)[None, :] < torch.as_tensor(st)[:, None])[:, :, None].to(dtype)


def zero_tails(ref, steps, T):
    """``ref`` as the ordered calls leave it: ZEROED tensors hold zeros from the step count of the row's tile on."""
    ran = torch.arange(T)[None, :] < torch.as_tensor(row_tile_steps(steps, T)[2])[:, None]
    return {k: v * ran[:, :, None].to(v.dtype) if k in ZEROED else v for k, v in ref.items()}


def layer_reference(x, w_hh, dhs=None, steps=None, ordered=False, dtype=torch.float64, rule="right"):
    """One layer.  ``x``: the step inputs xp [B,T,4h], or (table [V,4h], tokens [B,T]) for the rows ``table[tokens]``; w_hh
    [4h,h] row major; any hidden size h.  gates_t = x_t + h_{t-1} W_hh^T in the order i, f, g, o; c_t = sig(f) c_{t-1} + sig(i)
    tanh(g); h_t = sig(o) tanh(c_t).  Returns hs, cs, act (the activated gates) and, given ``dhs`` [B,T,h] (the gradient wrt
    every h_t), dgates (the gradient wrt the pre-activations), all in ``dtype`` on the CPU.  ``steps`` [B]: dhs counts as zero
    from steps[b] on.  ``ordered``: hs and dgates are zero from the step count of the row's tile on (``zero_tails``); cs and
    act are undefined there (they are returned as the plain recurrence gives them)."""
    x = (x[0][x[1]] if isinstance(x, tuple) else x).to(dtype).clone().requires_grad_(dhs is not None)
    B, T = x.size(0), x.size(1)
    out = _layer(x, w_hh.to(dtype), rule)
    ref = {k: torch.stack(out[k], 1).detach() for k in ("hs", "cs", "act")}
    if dhs is not None:
        (torch.stack(out["hs"], 1) * (dhs.to(dtype) * _valid(steps, B, T, dtype))).sum().backward()
        ref["dgates"] = torch.stack([v.grad for v in out["gates"]], 1)
    return zero_tails(ref, steps if steps is not None else np.full(B, T), T) if ordered else ref


def dropout_multiplier(seed, B, T, hidden, p, row_offset, rule="right"):
    """m [B,T,h] float32: lstm_dropout_ref.multiplier (keep / (1 - p), 0 where dropped), all ones for p = 0."""
    if p == 0:
        return torch.ones(B, T, hidden)
    if rule == "unscaled_mask":
        return torch.from_numpy(lstm_dropout_ref.keep_mask(seed, B, T, hidden, p, row_offset).astype(np.float32))
    return torch.from_numpy(lstm_dropout_ref.multiplier(seed, B, T, hidden, p, row_offset))


def stack_reference(x, w_hh1, w_ih2, b2, w_hh2, dhs2, p=0.0, seed=0, row_offset=0, dtype=torch.float64, rule="right"):
    """Two layers: the first as ``layer_reference`` takes ``x``; the second takes x2_t = b2 + (m * h1_t) W_ih2^T with m the
    ``dropout_multiplier``.  Returns STACK for the output gradient ``dhs2`` [B,T,h]: hsd = m * hs1, dg2 / dg1 the gradients wrt
    the second / first layer's pre-activations.  The layer rules apply to both layers."""
    x = (x[0][x[1]] if isinstance(x, tuple) else x).to(dtype).clone().requires_grad_(True)
    B, T, hidden = x.size(0), x.size(1), w_hh1.size(1)
    m = dropout_multiplier(seed, B, T, hidden, p, row_offset, rule).to(dtype)
    one = _layer(x, w_hh1.to(dtype), rule)
    hsd = torch.stack(one["hs"], 1) * m
    x2 = hsd @ w_ih2.to(dtype).t()
    if rule != "no_bias":
        x2 = x2 + b2.to(dtype)
    two = _layer(x2, w_hh2.to(dtype), rule)
    (torch.stack(two["hs"], 1) * dhs2.to(dtype)).sum().backward()
    ref = dict(hsd=hsd.detach())
    for n, lay, dg in (("1", one, "dg1"), ("2", two, "dg2")):
        for k in ("hs", "cs", "act"):
            ref[k + n] = torch.stack(lay[k], 1).detach()
        ref[dg] = torch.stack([v.grad for v in lay["gates"]], 1)
    return ref


def cell_reference(gates, c_prev, dh=None, dc_in=None, dtype=torch.float64):
    """One step from a given c_prev [B,h] (gates [B,4h], any h): h, c, act, and dgates / dc_prev for the gradients ``dh`` wrt h
    and ``dc_in`` wrt c, either of which may be absent (zero)."""
    g, cp = gates.to(dtype).clone().requires_grad_(True), c_prev.to(dtype).clone().requires_grad_(True)
    h, c, act = _cell(g, cp, "right")
    loss = (h * (0 if dh is None else dh.to(dtype))).sum() + (c * (0 if dc_in is None else dc_in.to(dtype))).sum()
    loss.backward()
    return dict(h=h.detach(), c=c.detach(), act=act.detach(), dgates=g.grad, dc_prev=cp.grad)


# ---------------------------------------------------------------------------------------------------------------------
# The layer cases.  Hidden is 256 (fixed by the kernels), rows come in tiles of 16.  A table, not a product: the smallest
# shapes at which each path can still go wrong.
# form: the step inputs as ``xp`` or as ``tokens`` (rows of a [V,4H] table, V = 20; the token rows are a view of T columns
#   into a [B, T + 3] tensor, and every row's last token differs from the one before it: the kernels fetch the token of
#   step min(t + 1, T - 1) ahead of time).
# regime:
#   typical      step inputs ~ 0.7 N(0, 1), W_hh ~ 0.06 N(0, 1): the scales of the kernel-against-kernel tests
#   saturated    step inputs x 4: gates on their rails, |c| grows past 3, tanh(c) flat
#   remembering  + 4 on the forget pre-activations, + 1 on the input gate's: c accumulates over all steps (|c| about 18 at
#                T = 46) and the gradient of a late h reaches the first steps' gates
# ``ragged``: rows of 1 .. T steps (row 0 has T, row 1 one), dhs zero from the row's steps on; else T steps each.
# ---------------------------------------------------------------------------------------------------------------------
_KEYS = ("name", "B", "T", "form", "regime", "ragged")
CASES = [dict(zip(_KEYS, c)) for c in [
    ("b1_t1", 1, 1, "xp", "typical", False),              # no recurrent step at all
    ("b16_t1_tok", 16, 1, "tokens", "typical", False),    # one exact tile, a token's single step
    ("b15_t2_tok", 15, 2, "tokens", "saturated", False),  # a partial tile, the first real hand-off
    ("b33_t2", 33, 2, "xp", "remembering", False),        # two tiles and a row behind them
    ("b16_t3", 16, 3, "xp", "remembering", True),         # both halves of the double buffers
    ("b17_t9_tok", 17, 9, "tokens", "typical", True),     # a one-row tile
    ("b33_t9", 33, 9, "xp", "saturated", True),
    ("b17_t46_tok", 17, 46, "tokens", "remembering", True),  # the longest question of the project
    ("b144_t3_tok", 144, 3, "tokens", "typical", True),   # 9 tiles: the second group of eight
    ("b260_t3_tok", 260, 3, "tokens", "saturated", True),  # 17 tiles, for the launches over row ranges
    ("b260_t3", 260, 3, "xp", "typical", True),           # the same with dense input: the tensor bases move with the range
    ("b520_t2", 520, 2, "xp", "typical", False),          # 33 tiles: four members per tile on the full chip
]]
# (case, rule) pairs a case cannot see: one step has no recurrence, two steps have nothing stale to read
EXEMPT = {rule: tuple(c["name"] for c in CASES if c["T"] == 1) for rule in ("stale_h", "no_cell_carry", "no_recurrent_grad")}
EXEMPT["stale_h"] += tuple(c["name"] for c in CASES if c["T"] == 2)
EXEMPT["gate_order"] = ()


def _step_inputs(B, T, form, regime, g):
    """xp [B,T,4H], or (table [V,4H], tokens: a [B,T] view of a [B,T+3] tensor), under the regime."""
    x = 0.7 * (torch.randn(B, T, 4 * H, generator=g) if form == "xp" else torch.randn(V, 4 * H, generator=g))
    if regime == "saturated":
        x = x * 4.0
    if regime == "remembering":
        x[..., :H] += 1.0
        x[..., H:2 * H] += 4.0
    if form == "xp":
        return x
    tokens = torch.randint(0, V, (B, T + 3), generator=g)
    if T > 1:
        same = tokens[:, T - 1] == tokens[:, T - 2]
        tokens[:, T - 1] = torch.where(same, (tokens[:, T - 1] + 1) % V, tokens[:, T - 1])
    return x, tokens[:, :T]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The float32 CPU tensors of a layer case: x (as ``layer_reference`` takes it), w_hh, dhs, steps."""
    case = next(c for c in CASES if c["name"] == name)
    B, T = case["B"], case["T"]
    g = torch.Generator().manual_seed(2000 + CASES.index(case))
    x = _step_inputs(B, T, case["form"], case["regime"], g)
    w_hh = 0.06 * torch.randn(4 * H, H, generator=g)
    steps = torch.full((B,), T, dtype=torch.int64)
    if case["ragged"]:
        steps = torch.randint(1, T + 1, (B,), generator=g)
        steps[0], steps[1] = T, 1
        tile_steps, of_row = row_tile_steps(steps.numpy(), T)[1:]
        assert B <= 16 or tile_steps.min() < T      # a tile stops early ...
        assert (steps.numpy() < of_row).any()       # ... and a row stops before its tile does
    dhs = torch.randn(B, T, H, generator=g) * (torch.arange(T)[None, :] < steps[:, None])[:, :, None]
    return dict(x=x, w_hh=w_hh, dhs=dhs, steps=steps.numpy())


@functools.lru_cache(maxsize=None)
def case_reference(name, dtype=torch.float64, rule="right"):
    i = case_inputs(name)
    return layer_reference(i["x"], i["w_hh"], i["dhs"], i["steps"], dtype=dtype, rule=rule)


@functools.lru_cache(maxsize=None)
def case_bars(name, ordered=False):
    i = case_inputs(name)
    T = i["dhs"].size(1)
    ref, f32 = case_reference(name), case_reference(name, torch.float32)
    return error_bars(zero_tails(ref, i["steps"], T), zero_tails(f32, i["steps"], T)) if ordered else error_bars(ref, f32)


# ---------------------------------------------------------------------------------------------------------------------
# The stack cases: a linked pair of layers (B, T, form of layer 1, p, row_offset), regimes of layer 1's inputs in rotation,
# the layers' W_hh, W_ih and b uniform in +-0.0625 (the scale of ``_layer`` in test_lstm_stack_gpu.py), every step of every
# row.  Each launch also carries ``RIDER``, an independent layer of 20 rows x 3 steps with dense input, held to
# ``layer_reference``.  p = 1 gives hsd = 0 and dg1 identically zero (``error_bars``: must be exactly zero).
# ---------------------------------------------------------------------------------------------------------------------
_SKEYS = ("name", "B", "T", "form", "p", "row_offset", "regime")
STACK_CASES = [dict(zip(_SKEYS, c)) for c in [
    ("s_b1_t1", 1, 1, "xp", 0.0, 0, "typical"),
    ("s_b17_t2_tok_p03", 17, 2, "tokens", 0.3, 5, "saturated"),
    ("s_b33_t9_tok", 33, 9, "tokens", 0.0, 0, "remembering"),
    ("s_b16_t9_p1", 16, 9, "xp", 1.0, 0, "typical"),
    ("s_b40_t3_tok_p05", 40, 3, "tokens", 0.5, 2 ** 33, "saturated"),
]]
RIDER = (20, 3)
DROPOUT_SEED = 0x2545_F491_4F6C_DD1D
# the mask of p = 0 is all ones and that of p = 1 all zeros, scaled or not
STACK_EXEMPT = dict(unscaled_mask=tuple(c["name"] for c in STACK_CASES if c["p"] in (0.0, 1.0)), no_bias=())
STACK_EXEMPT.update({rule: tuple(c["name"] for c in STACK_CASES if c["T"] == 1) for rule in LAYER_RULES[:3]})
STACK_EXEMPT["stale_h"] += tuple(c["name"] for c in STACK_CASES if c["T"] == 2)
STACK_EXEMPT["gate_order"] = ()


def _uniform(g, *shape):
    return (torch.rand(*shape, generator=g) - 0.5) * 0.125


@functools.lru_cache(maxsize=None)
def stack_inputs(name):
    case = next(c for c in STACK_CASES if c["name"] == name)
    B, T = case["B"], case["T"]
    k = STACK_CASES.index(case)
    g = torch.Generator().manual_seed(3000 + k)
    x = _step_inputs(B, T, case["form"], case["regime"], g)
    w = {n: _uniform(g, 4 * H, H) for n in ("w_hh1", "w_ih2", "w_hh2", "w_hh3")}
    rb, rt = RIDER
    return dict(w, x=x, b2=_uniform(g, 4 * H), dhs2=torch.randn(B, T, H, generator=g), p=case["p"], seed=DROPOUT_SEED + k,
                row_offset=case["row_offset"], x3=0.7 * torch.randn(rb, rt, 4 * H, generator=g), dhs3=torch.randn(rb, rt, H, generator=g))


@functools.lru_cache(maxsize=None)
def stack_case_reference(name, dtype=torch.float64, rule="right"):
    """STACK of the pair and, as hs3, cs3, act3, dg3, the rider's LAYER."""
    i = stack_inputs(name)
    ref = stack_reference(i["x"], i["w_hh1"], i["w_ih2"], i["b2"], i["w_hh2"], i["dhs2"], i["p"], i["seed"], i["row_offset"], dtype, rule)
    rider = layer_reference(i["x3"], i["w_hh3"], i["dhs3"], dtype=dtype, rule=rule if rule in LAYER_RULES else "right")
    ref.update(hs3=rider["hs"], cs3=rider["cs"], act3=rider["act"], dg3=rider["dgates"])
    return ref


@functools.lru_cache(maxsize=None)
def stack_case_bars(name):
    return error_bars(stack_case_reference(name), stack_case_reference(name, torch.float32))
