"""The teacher-forced attention-LSTM decoder, forward and backward, as plain torch on the host: the statement of the operation
the decoder kernels are held to (include/probnmn_hip.h beside pnmn_attn_lstm_fwd; the arithmetic of
``filtered_inputs.emulate_decoder_logits``), the case table the CPU and the GPU test share, and the error bar.

Nothing here knows how the kernels compute: the backward is autograd through the forward, in float64.  The same function in
float32 gives the round-off a float32 evaluation of the recurrence has on a case, from which the bar is derived."""
import functools

import numpy as np
import torch

import filtered_inputs as fi

H, V = fi.H, 20
FWD = ("hs", "cs", "act", "ctx", "probs")
BWD = ("dgates", "dctx", "dscore", "weights", "dh0", "denc")
ZEROED = ("hs", "ctx", "dgates", "dctx", "dscore", "weights")  # zero from the tile's steps on under an order
UNWRITTEN = ("cs", "act", "probs")                             # left unwritten there
RULES = ("masked", "plain_softmax", "no_epsilon")


def attention(scores, mask, rule="masked"):
    """(probs, weights) of one step.  ``masked``: allennlp's masked_softmax, softmax(score * mask) * mask / (sum + 1e-13) -- a
    masked position still puts exp(0) into the first normalisation.  The other two are deliberately WRONG rules, there to
    show that a case's inputs can tell them from the right one: ``plain_softmax`` sets masked scores to -inf and normalises
    once (its ``probs`` are its weights: it has no softmax before masking); ``no_epsilon`` drops the 1e-13."""
    if rule == "plain_softmax":
        w = torch.softmax(scores.masked_fill(mask == 0, float("-inf")), 1)
        return w, w
    p = torch.softmax(scores * mask, 1)
    q = p * mask
    return p, q / (q.sum(1, keepdim=True) + (0.0 if rule == "no_epsilon" else 1e-13))


def row_tile_steps(steps, T):
    """(order, tile_steps, steps of the tile every row sits in) as pnmn_length_order_steps groups rows of ``steps`` steps:
    steps clamped to [1, T], rows sorted longest first (stable), cut into tiles of 16, a tile runs its longest row's steps."""
    st = np.clip(np.asarray(steps, np.int64), 1, T)
    order = np.argsort(-st, kind="stable")
    tile_steps = st[order[::16]]
    of_row = np.empty_like(st)
    of_row[order] = np.repeat(tile_steps, 16)[:st.size]
    return order.astype(np.int32), tile_steps.astype(np.int32), of_row


def zero_tails(ref, steps, T):
    """``ref`` as the ordered calls leave it: ZEROED tensors hold zeros from the step count of the row's tile on."""
    of_row = torch.as_tensor(row_tile_steps(steps, T)[2])
    ran = torch.arange(T)[None, :] < of_row[:, None]
    return {k: v * ran[:, :, None].to(v.dtype) if k in ZEROED else v for k, v in ref.items()}


def decoder_reference(d, T, xe=None, in_tokens=None, dhs=None, steps=None, ordered=False, dtype=torch.float64, rule="masked"):
    """The recurrence over T steps and, given ``dhs`` [B,T,H] (the gradient wrt every h_t), its backward by autograd.
    ``d``: enc [B,S,H], mask [B,S], h0 [B,H], w_c / w_hh [4H,H] row major and, with ``in_tokens`` [B,T], etable [V,4H]; step
    inputs ``xe`` [B,T,4H] or the rows ``etable[in_tokens]``.  Any hidden size.  ``steps`` [B]: row b has steps[b] steps --
    its dhs counts as zero from there on; ``ordered``: the zeros of ``zero_tails`` on top.  Returns FWD (act in the order
    i, f, g, o), weights and, with dhs, the rest of BWD, all in ``dtype`` on the CPU."""
    f = {k: d[k].to(dtype) for k in ("enc", "mask", "h0", "w_c", "w_hh")}
    x = (xe if xe is not None else d["etable"][in_tokens]).to(dtype)
    grad = dhs is not None
    enc, h0 = f["enc"].clone().requires_grad_(grad), f["h0"].clone().requires_grad_(grad)
    h, c = h0, torch.zeros_like(h0)
    out = {k: [] for k in FWD + ("weights", "scores", "gates")}
    for t in range(T):
        scores = torch.einsum("bsh,bh->bs", enc, h)
        p, w = attention(scores, f["mask"], rule)
        ctx = torch.einsum("bs,bsh->bh", w, enc)
        gates = x[:, t] + ctx @ f["w_c"].t() + h @ f["w_hh"].t()
        if grad:
            for leaf in (scores, ctx, gates):
                leaf.retain_grad()
        i, fg, g, o = gates.chunk(4, 1)
        act = torch.cat((torch.sigmoid(i), torch.sigmoid(fg), torch.tanh(g), torch.sigmoid(o)), 1)
        i, fg, g, o = act.chunk(4, 1)
        c = fg * c + i * g
        h = o * torch.tanh(c)
        for k, v in zip(out, (h, c, act, ctx, p, w, scores, gates)):
            out[k].append(v)
    ref = {k: torch.stack(out[k], 1).detach() for k in FWD + ("weights",)}
    if grad:
        dh = dhs.to(dtype)
        if steps is not None:
            dh = dh * (torch.arange(T)[None, :] < torch.as_tensor(np.asarray(steps))[:, None])[:, :, None].to(dtype)
        (torch.stack(out["hs"], 1) * dh).sum().backward()
        for k, src in (("dgates", "gates"), ("dctx", "ctx"), ("dscore", "scores")):
            ref[k] = torch.stack([v.grad for v in out[src]], 1)
        ref["denc"], ref["dh0"] = enc.grad, h0.grad
    return zero_tails(ref, steps if steps is not None else np.full(enc.size(0), T), T) if ordered else ref


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  Hidden is 256 (fixed by the kernels).  A table, not a product:
#   S  1 2 7 9 33 58 59 60 63 64   both tail loops of the backward (S % 4, S % 8), the layout boundary 58/59/60, the full wave
#   B  1 15 16 17 33               a partial tile, an exact one, whole tiles and a partial one behind them
#   T  1 2 9 64                    (64 once)
# form: the step inputs as ``xe`` or as ``tokens`` (rows of etable).  Masks are prefixes; rows 0, 1, 2 have lengths S, 1 and
# S - 1, ``zero_row`` gives row 3 an all-zero mask.  ``ragged``: rows of 1 .. T steps (row 0 has T, row 1 one), else T each.
# regime:
#   saturated  fi.decoder_inputs as it is: enc, h0 ~ N(0, 1), the largest weight of a row is mostly near 1
#   diffuse    enc x 0.1, h0 x 0.3: weights spread out, masked positions hold about half of the mass before masking
#   faint      h0 x 0.3 and every valid enc row = -a_b h0 / |h0| + 0.5 N(0, 1), a_b |h0| from 13 to 31 over the rows (half of
#              them below 17.5, so that the median stays put while a few rows reach Z ~ 1e-12): at step 0
#              the valid positions score strongly negative, the masked ones (score * mask = 0) hold nearly all of the mass
#              before masking and Z = sum(p * mask) comes within reach of the 1e-13 (the median Z is checked on the CPU)
# ``exempt``: every row unmasked, so the plain softmax IS the masked one -- such a case cannot tell rule (a) apart.
# ---------------------------------------------------------------------------------------------------------------------
_KEYS = ("name", "B", "T", "S", "form", "regime", "zero_row", "ragged")
CASES = [dict(zip(_KEYS, c)) for c in [
    ("b1_t1_s1", 1, 1, 1, "xe", "saturated", False, False),
    ("b15_t2_s2", 15, 2, 2, "tokens", "diffuse", True, False),
    ("b17_t9_s7", 17, 9, 7, "xe", "faint", False, True),
    ("b33_t9_s9", 33, 9, 9, "tokens", "diffuse", True, True),
    ("b16_t2_s33", 16, 2, 33, "xe", "saturated", False, False),
    ("b17_t64_s64", 17, 64, 64, "tokens", "diffuse", False, True),
    ("b16_t9_s58", 16, 9, 58, "tokens", "faint", False, False),
    ("b15_t2_s59", 15, 2, 59, "xe", "diffuse", False, True),
    ("b33_t2_s60", 33, 2, 60, "tokens", "saturated", True, True),
    ("b17_t9_s63", 17, 9, 63, "xe", "faint", True, False),
    ("b1_t9_s64", 1, 9, 64, "tokens", "diffuse", False, False),
    ("b33_t1_s64", 33, 1, 64, "xe", "saturated", False, False),
    ("b16_t1_s7", 16, 1, 7, "tokens", "faint", False, False),
    ("b15_t9_s60", 15, 9, 60, "xe", "saturated", False, True),
]]
EXEMPT = ("b1_t1_s1",)
FAINT_Z = (1e-9, 1e-5)  # where the median Z of a faint case's rows lies at step 0


def case_lengths(case, g):
    B, S = case["B"], case["S"]
    hi = S if case["regime"] != "faint" else max(1, S - 1)  # (faint: masked positions in nearly every row)
    lens = torch.randint(1, hi + 1, (B,), generator=g)
    if B == 1:
        lens[0] = max(1, S - 1)
    for row, n in ((0, S), (1, 1), (2, max(1, S - 1))):
        if row < B and B > 1:
            lens[row] = n
    if case["zero_row"]:
        lens[3] = 0
    return lens


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The float32 CPU tensors of a case: what ``decoder_reference`` takes (``d``, and xe or in_tokens, dhs, steps)."""
    case = next(c for c in CASES if c["name"] == name)
    B, T, S, regime = case["B"], case["T"], case["S"], case["regime"]
    seed = 1000 + CASES.index(case)
    d = fi.decoder_inputs(B, S, V, seed)
    g = torch.Generator().manual_seed(seed + 500)
    lens = case_lengths(case, g)
    d["mask"] = (torch.arange(S)[None, :] < lens[:, None]).float()
    if regime != "saturated":
        d["h0"] = d["h0"] * 0.3
    if regime == "diffuse":
        d["enc"] = d["enc"] * 0.1
    if regime == "faint":
        norm = d["h0"].norm(dim=1, keepdim=True)
        target = (13.0 + 18.0 * torch.linspace(0.0, 1.0, B) ** 2)[torch.randperm(B, generator=g)][:, None]  # a_b |h0|
        valid = -(target / norm) * (d["h0"] / norm)
        d["enc"] = torch.where(d["mask"][:, :, None] > 0, valid[:, None, :] + 0.5 * d["enc"], d["enc"])
    inputs = dict(d=d, xe=None, in_tokens=None)
    if case["form"] == "xe":
        inputs["xe"] = torch.randn(B, T, 4 * H, generator=g)
    else:
        inputs["in_tokens"] = torch.randint(0, V, (B, T), generator=g)
    steps = torch.full((B,), T, dtype=torch.int64)
    if case["ragged"]:
        steps = torch.randint(1, T + 1, (B,), generator=g)
        steps[0], steps[1] = T, 1
    inputs["steps"] = steps.numpy()
    inputs["dhs"] = torch.randn(B, T, H, generator=g) * (torch.arange(T)[None, :] < steps[:, None])[:, :, None]
    return inputs


@functools.lru_cache(maxsize=None)
def case_reference(name, dtype=torch.float64, rule="masked"):
    i = case_inputs(name)
    return decoder_reference(i["d"], i["dhs"].size(1), i["xe"], i["in_tokens"], i["dhs"], i["steps"], dtype=dtype, rule=rule)


# ---------------------------------------------------------------------------------------------------------------------
# The error bar, from the reference alone.  Per case and tensor k: scale_k = max |ref_k|, e32_k = max |f32_k - ref_k| / scale_k
# with f32 the SAME function evaluated in float32 on the host, and
#     bar_k = min(1e-4, max(16 e32_k, 2e-6))
# 16: the kernels associate their sums over 256 columns and up to 64 positions differently and use the hardware's exp and
# reciprocal; 2e-6 is about 16 ulp of the scale; 1e-4 is the bar of test_persistent_decoder_matches_stepwise_torch.
# ---------------------------------------------------------------------------------------------------------------------
FACTOR, FLOOR, CEILING = 16.0, 2e-6, 1e-4


def error_bars(ref, f32):
    """{k: (scale_k, bar_k)}; a tensor whose reference is identically zero has scale 0 (it must then be exactly zero)."""
    bars = {}
    for k, want in ref.items():
        scale = float(want.abs().max())
        e32 = float((f32[k].double() - want).abs().max()) / scale if scale > 0 else 0.0
        bars[k] = (scale, min(CEILING, max(FACTOR * e32, FLOOR)))
    return bars


def case_bars(name, ordered=False):
    i = case_inputs(name)
    T = i["dhs"].size(1)
    ref, f32 = case_reference(name), case_reference(name, torch.float32)
    return error_bars(zero_tails(ref, i["steps"], T), zero_tails(f32, i["steps"], T)) if ordered else error_bars(ref, f32)
