"""Plain float64 reference of the grouped convolution, forward and data-gradient (include/probnmn_hip.h, pnmn_conv_nhwc):

    x[p][c]  = in[p * in_stride + c]             chunk k of 128 input channels at in + 128 k, or from in2 for k >= 1
    x       *= mask[p]                           if mask
    x        = gate[p * in_stride + c] > 0 ? x : 0    if gate
    res[p][n] = sum_{tap, c} x[shift(p, tap, dil)][c] * W[n][tap][c]
    out[p * out_stride + n] = act(bias[n] + res[p][n])            (+= with PNMN_CONV_ACCUMULATE, atomically or not)
    PNMN_CONV_DATTN:    out stored as above;  mb_dattn[p] += sum_c res[p][c] * mb_feats[p][c]   if mb_attn
    PNMN_CONV_MASKBWD:  out not written;      mb_dfeats[p][c] += res[p][c] * mb_attn[p] (1 if NULL);  mb_dattn as above

with shift(p, tap, dil) = (y + (tap // 3 - 1) dil, x + (tap % 3 - 1) dil), zero outside the image (1x1: no shift).

`reference()` is written from that statement -- one matrix product per tap over explicitly shifted maps -- and calls
neither the library nor autograd.  The data gradient is the same routine: the caller hands it `transposed(w)`, the
[Cin][taps reversed][Cout] operand, built here with torch.  tests/test_conv_reference.py holds the reference against
F.conv2d and float64 autograd, and shows that it tells the rule above from six near misses (`rule=`).

`plan` / `units_of` restate the launch planner (csrc/conv_plan.h, plan_launch) and the order in which a persistent
workgroup visits the launch's units (csrc/conv_stream.h, Walker::decode); test_conv_reference.py holds `plan` against the
compiled header.  They choose and label the cases of tests/test_conv_stream_gpu.py and never enter an expected value.

A `Launch` describes one call the way the kernel sees it: items that point into small pools of maps and weights.
"""
import os
from dataclasses import dataclass
from typing import List, Optional

import torch

CB = 128
ACCUMULATE, ATOMIC, MASKBWD, MB_SOLE, DATTN = 1, 2, 4, 8, 16
PX, PM, PG, NWT, PF = 5, 3, 3, 3, 3       # pool sizes: inputs, masks / attentions, gates, weights, mb_feats maps
SPLITS_3X3 = (1, 2, 4, 6, 8, 14, 26)
SPLITS_1X1 = (1, 2, 4, 8)
RULES = ("dilation_row_off", "taps_reversed", "mask_after", "gate_ge", "in2_for_chunk0", "bias_per_chunk")


@dataclass
class Item:
    x: int                    # input map (pool index)
    w: int = 0                # weight (pool index); its bias goes with it
    dil: int = 1
    x2: int = -1              # second source for the chunks >= 1 (x2 pool), or -1
    mask: int = -1
    gate: int = -1
    bias: bool = True
    flags: int = 0
    out: int = -1             # output map, or -1 (MASKBWD)
    feats: int = -1           # mb_feats
    attn: int = -1            # mb_attn (mask pool), or -1 = NULL
    dfeats: int = -1
    dattn: int = -1


@dataclass
class Launch:
    H: int
    ntaps: int
    cin_chunks: int
    cout_blocks: int
    in_stride: int
    out_stride: int
    relu: int
    items: List[Item]
    x_pool: Optional[torch.Tensor] = None     # [PX][HW][128 with a second source, else cin]
    x2_pool: Optional[torch.Tensor] = None    # [PX][HW][128]
    m_pool: Optional[torch.Tensor] = None     # [PM][HW]   masks and mb_attn
    g_pool: Optional[torch.Tensor] = None     # [PG][HW][cin]
    w_pool: Optional[torch.Tensor] = None     # [NWT][cout][ntaps][cin]
    b_pool: Optional[torch.Tensor] = None     # [NWT][cout]
    f_pool: Optional[torch.Tensor] = None     # [PF][HW][128]
    out_pre: Optional[torch.Tensor] = None    # [n_out][HW][cout]: contents before the call (NaN where only plain stores go)
    df_pre: Optional[torch.Tensor] = None     # [n_dfeats][HW][128]
    da_pre: Optional[torch.Tensor] = None     # [n_dattn][HW]
    note: str = ""

    @property
    def W(self):
        return self.H

    @property
    def HW(self):
        return self.H * self.H

    @property
    def cin(self):
        return self.cin_chunks * CB

    @property
    def cout(self):
        return self.cout_blocks * CB

    @property
    def bands(self):
        return 1 if self.H == 14 else 4

    @property
    def two_sources(self):
        return any(it.x2 >= 0 for it in self.items)

    def count(self, what):
        return 1 + max([getattr(it, what) for it in self.items] + [-1])


def transposed(w):
    """[Cout][taps][Cin] -> [Cin][taps reversed][Cout]: the operand of the data gradient."""
    return w.permute(2, 1, 0).flip(1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def fill(L, kind="int", seed=0, dgrad=False):
    """Pools and prefills of a launch.  kind "int": small integers as float32 (x, w, feats in [-2, 2]; masks and mb_attn in
    {0, 1, 2}; gates in {-1, -0.0, 0, 1}; bias and prefills in [-3, 3]): every product and partial sum `exact_ok` admits
    is exact in float32 in any order.  kind "normal": the data of tests/test_hip_kernels.py (ReLU'd normal inputs --
    plain normal for a data gradient --, sigmoid masks, He-scaled weights, 0.1-scaled bias, ReLU'd normal gates)."""
    g = torch.Generator().manual_seed(1234 + seed)
    HW, cx = L.HW, (CB if L.two_sources else L.cin)
    n_out, n_df, n_da = L.count("out"), L.count("dfeats"), L.count("dattn")
    if kind == "int":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
        L.x_pool, L.x2_pool = ri(-2, 2, PX, HW, cx), ri(-2, 2, PX, HW, CB)
        L.m_pool = ri(0, 2, PM, HW)
        L.g_pool = torch.tensor([-1.0, -0.0, 0.0, 1.0])[torch.randint(0, 4, (PG, HW, L.cin), generator=g)]
        L.w_pool, L.b_pool = ri(-2, 2, NWT, L.cout, L.ntaps, L.cin), ri(-3, 3, NWT, L.cout)
        L.f_pool = ri(-2, 2, PF, HW, CB)
        pre = lambda *s: ri(-3, 3, *s)  # noqa: E731
    else:
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        L.x_pool = rn(PX, HW, cx) if dgrad else torch.relu(rn(PX, HW, cx))
        L.x2_pool = torch.relu(rn(PX, HW, CB))
        L.m_pool = torch.sigmoid(rn(PM, HW))
        L.g_pool = torch.relu(rn(PG, HW, L.cin))
        L.w_pool = rn(NWT, L.cout, L.ntaps, L.cin) * (2.0 / (L.ntaps * L.cin)) ** 0.5
        L.b_pool = rn(NWT, L.cout) * 0.1
        L.f_pool = torch.relu(rn(PF, HW, CB))
        pre = lambda *s: rn(*s)  # noqa: E731
    L.out_pre = pre(n_out, HW, L.cout)
    plain = {it.out for it in L.items if it.out >= 0 and (not (it.flags & ACCUMULATE) or (it.flags & DATTN))}
    for o in plain:  # a plain store must not depend on what was there
        L.out_pre[o] = float("nan")
    L.df_pre, L.da_pre = pre(n_df, HW, CB), pre(n_da, HW)
    for it in L.items:  # (DATTN without attention: the map must stay exactly zero)
        if (it.flags & DATTN) and it.attn < 0 and it.dattn >= 0:
            L.da_pre[it.dattn] = 0.0
    return L


def exact_ok(L):
    """The largest magnitude any partial sum of the launch can reach -- a result, the 128-channel mb_dattn sum, the sum
    over all items that add into one map, prefill included -- is below 2^24, so that float32 holds every one exactly."""
    amax = lambda t: float(t.abs().max()) if t is not None and t.numel() else 0.0  # noqa: E731
    mx = max(amax(L.x_pool), amax(L.x2_pool) if L.two_sources else 0.0)
    mm = max(1.0, amax(L.m_pool))
    res = L.ntaps * L.cin * mx * mm * amax(L.w_pool)
    outs, dfs, das = {}, {}, {}
    for it in L.items:
        if it.flags & MASKBWD:
            dfs[it.dfeats] = dfs.get(it.dfeats, amax(L.df_pre)) + res * (mm if it.attn >= 0 else 1.0)
        else:
            r = res + (amax(L.b_pool) if it.bias else 0.0)
            keep = (it.flags & ACCUMULATE) and not (it.flags & DATTN)
            outs[it.out] = (outs.get(it.out, amax(torch.nan_to_num(L.out_pre))) if keep else 0.0) + r
        if (it.flags & (MASKBWD | DATTN)) and it.attn >= 0:
            das[it.dattn] = das.get(it.dattn, amax(L.da_pre)) + CB * res * amax(L.f_pool)
    most = max([res] + list(outs.values()) + list(dfs.values()) + list(das.values()))
    assert most < 2 ** 24, "the integer sums of this launch could round in float32 (%g)" % most
    return most


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def shifted(x, H, W, oy, ox):
    """x [HW][C] -> the map read at offset (oy, ox) of each pixel, zero outside the image."""
    xi = x.reshape(H, W, -1)
    out = torch.zeros_like(xi)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = xi[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out.reshape(H * W, -1)


def result_of(L, it, P, rule=None, dtype=torch.float64):
    """(res [HW][cout] before bias and activation, the loaded and prepared input x [HW][cin]) of one item.  `rule`: one
    of RULES, a deliberately wrong statement (tests/test_conv_reference.py)."""
    x = P["x"][it.x].to(dtype)
    if it.x2 >= 0:
        x2 = P["x2"][it.x2].to(dtype)
        x = torch.cat([x2 if rule == "in2_for_chunk0" else x[:, :CB]] + [x2] * (L.cin_chunks - 1), 1)
    if it.mask >= 0 and rule != "mask_after":
        x = x * P["m"][it.mask].to(dtype).unsqueeze(1)
    if it.gate >= 0:
        g = P["g"][it.gate]
        x = torch.where((g >= 0) if rule == "gate_ge" else (g > 0), x, torch.zeros_like(x))
    w = P["w"][it.w].to(dtype)
    res = torch.zeros(L.HW, L.cout, dtype=dtype, device=x.device)
    for t in range(L.ntaps):
        tw = L.ntaps - 1 - t if rule == "taps_reversed" else t
        if L.ntaps == 9:
            ky = (t // 3 + 1) % 3 if rule == "dilation_row_off" else t // 3
            xs = shifted(x, L.H, L.W, (ky - 1) * it.dil, (t % 3 - 1) * it.dil)
        else:
            xs = x
        res += xs @ w[:, tw, :].t()
    if it.mask >= 0 and rule == "mask_after":
        res = res * P["m"][it.mask].to(dtype).unsqueeze(1)
    return res, x


def pools_on(L, device):
    return {k: (t.to(device) if t is not None else None) for k, t in
            (("x", L.x_pool), ("x2", L.x2_pool), ("m", L.m_pool), ("g", L.g_pool), ("w", L.w_pool), ("b", L.b_pool), ("f", L.f_pool))}


def reference(L, device="cpu", rule=None, dtype=torch.float64):
    """{"out": [n_out][HW][cout], "dfeats": [n][HW][128], "dattn": [n][HW]} in float64 (or `dtype`: the float32 yardstick
    of the round-off tests): every tensor the launch writes, prefill included."""
    P = pools_on(L, device)
    out, df, da = (t.to(device=device, dtype=dtype).clone() for t in (L.out_pre, L.df_pre, L.da_pre))
    for it in L.items:
        res, _ = result_of(L, it, P, rule, dtype)
        if it.flags & (MASKBWD | DATTN):
            assert not it.bias and not L.relu, "the fused mask backward is stated for a data gradient: no bias, no activation"
        if it.flags & MASKBWD:
            a = P["m"][it.attn].to(dtype).unsqueeze(1) if it.attn >= 0 else 1.0
            df[it.dfeats] += res * a
        else:
            y = res
            if it.bias:
                y = y + P["b"][it.w].to(dtype) * (L.cin_chunks if rule == "bias_per_chunk" else 1)
            if L.relu:
                y = torch.relu(y)
            if (it.flags & ACCUMULATE) and not (it.flags & DATTN):
                out[it.out] += y
            else:
                out[it.out] = y
        if (it.flags & (MASKBWD | DATTN)) and it.attn >= 0:
            da[it.dattn] += (res * P["f"][it.feats].to(dtype)).sum(1)
    return {"out": out, "dfeats": df, "dattn": da}


U32 = 2.0 ** -24  # unit round-off of float32


def ulp32(v):
    """Spacing of float32 at magnitude v (float64 tensor, v >= 0)."""
    return torch.exp2(torch.floor(torch.log2(v.clamp_min(2.0 ** -126))) - 23)


def contraction_order(L, it):
    """The (tap, first input channel) of the 32-channel blocks an output's accumulator takes in, in the kernel's order
    (csrc/conv_stream.h, Walker::next_stage): a stage is 32 channels; a whole 14x14 map, a 1x1 and dilation 1 contract all
    taps of a stage, a 28x28 band at dilation 2, 4 or 8 goes tap row by tap row."""
    banded = L.H == 28 and L.ntaps == 9 and it.dil != 1
    order = []
    for chunk in range(L.cin_chunks):
        for row in (range(3) if banded else [None]):
            for kq in range(4):
                for t in (range(3 * row, 3 * row + 3) if banded else range(L.ntaps)):
                    order.append((t, chunk * CB + kq * 32))
    return order


def chain_sigma(L, device="cpu"):
    """{"out", "dfeats"}: standard deviation (largest over the entries) of the round-off of ONE float32 accumulator per output
    that takes in all K = ntaps * cin products behind each other, as the kernel's MFMA chain does, where a CPU sums in
    blocks.  An addition rounds its partial sum S to nearest: an error uniform over one ulp(S), variance ulp(S)^2 / 12,
    independent between additions; one rounding is counted per NON-ZERO product (an upper count: an MFMA adds four products
    per accumulation; adding an exact zero -- padding, a ReLU'd or gated input -- rounds nothing).  The partial sums are the
    float64 reference's, block by block in `contraction_order`; inside a block of 32 channels no partial sum leaves
    max(|S_before|, |S_after|) + T with T the block's sum of |products|.  Behind the chain: one rounding for the bias, or
    two for mb_dfeats (the product with the attention and the addition), at the size of the result.  Computed from the
    inputs alone."""
    P = pools_on(L, device)
    worst = {"out": 0.0, "dfeats": 0.0}
    for it in L.items:
        _, x = result_of(L, it, P)
        w = P["w"][it.w].double()
        s = torch.zeros(L.HW, L.cout, dtype=torch.float64, device=x.device)
        q = torch.zeros_like(s)
        for (t, c0) in contraction_order(L, it):
            xs = x[:, c0:c0 + 32]
            if L.ntaps == 9:
                xs = shifted(xs, L.H, L.W, (t // 3 - 1) * it.dil, (t % 3 - 1) * it.dil)
            wb = w[:, t, c0:c0 + 32].t()
            after = s + xs @ wb
            tmag = xs.abs() @ wb.abs()
            nnz = (xs != 0).double() @ (wb != 0).double()
            q += nnz * ulp32(torch.maximum(s.abs(), after.abs()) + tmag) ** 2
            s = after
        if it.flags & MASKBWD:
            a = P["m"][it.attn].double().unsqueeze(1) if it.attn >= 0 else 1.0
            final = (L.df_pre[it.dfeats].double().to(x.device).abs() + (s * a).abs())
            var = (q * a * a + 2 * ulp32(final) ** 2) / 12.0
            worst["dfeats"] = max(worst["dfeats"], float(var.max().sqrt()))
        else:
            b = P["b"][it.w].double().abs() if it.bias else 0.0
            var = (q + ulp32(s.abs() + b) ** 2) / 12.0
            worst["out"] = max(worst["out"], float(var.max().sqrt()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# launch planner and unit walk, restated
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    splits: tuple
    counts: tuple

    @property
    def n_seg(self):
        return len(self.splits)


def default_cus():
    e = os.environ.get("PNMN_CONV_CUS")
    try:
        c = int(e) if e else 256
    except ValueError:
        c = 0
    return (c & ~7) if 8 <= c <= 256 else 256


def plan(n_units, cout_blocks, cin_chunks, ntaps, cus=0, forced=0):
    """plan_launch of csrc/conv_plan.h: up to three segments of non-decreasing split.  `forced`: pnmn_conv_force_split's
    value (a 3x3-only split on a 1x1 launch falls back to the planner)."""
    if forced and not ((forced == 6 or forced > 8) and ntaps != 9):
        return Plan((forced,), (n_units,))
    work = float(ntaps) * cin_chunks
    seg_cost, overhead = 0.3, 0.25
    pairs = {1: 26.0, 2: 13.0, 4: 7.0, 6: 5.0, 8: 4.0, 14: 2.0, 26: 1.0}
    cost = lambda s: work * pairs[s] / 26.0 + overhead  # noqa: E731
    splits = list(SPLITS_3X3) if ntaps == 9 else list(SPLITS_1X1)
    cus = cus if 8 <= cus <= 256 else default_cus()
    rounds = lambda n, s: (n * cout_blocks * s + cus - 1) // cus  # noqa: E731

    def full(n, s):
        per = cout_blocks * s
        return min(n, (n * per // cus) * cus // per)

    best, best_t = Plan((1,), (n_units,)), 1e30

    def consider(p, t):
        nonlocal best, best_t
        if t < best_t * 0.97:
            best, best_t = p, t

    for i0, s0 in enumerate(splits):
        consider(Plan((s0,), (n_units,)), float(rounds(n_units, s0)) * cost(s0))
        m0 = full(n_units, s0)
        if m0 <= 0 or m0 >= n_units:
            continue
        t0 = float(rounds(m0, s0)) * cost(s0)
        r0 = n_units - m0
        for i1 in range(i0, len(splits)):
            s1 = splits[i1]
            consider(Plan((s0, s1), (m0, r0)), t0 + float(rounds(r0, s1)) * cost(s1) + seg_cost)
            if s1 == s0:
                continue
            m1 = full(r0, s1)
            if m1 <= 0 or m1 >= r0:
                continue
            t1 = t0 + float(rounds(m1, s1)) * cost(s1) + seg_cost
            r1 = r0 - m1
            for s2 in splits[i1 + 1:]:
                consider(Plan((s0, s1, s2), (m0, m1, r1)), t1 + float(rounds(r1, s2)) * cost(s2) + seg_cost)
    return best


def grid_of(p, cout_blocks, cus=0):
    """Workgroups the launch side starts for a plan (launch_stream of csrc/conv_nhwc.hip)."""
    total = sum(((c + 7) // 8) * 8 * s for s, c in zip(p.splits, p.counts) if c > 0) * cout_blocks
    return min((cus & ~7) if 8 <= cus <= 256 else default_cus(), total)


def units_of(p, grid, cout_blocks=1, bands=1):
    """Walker::decode of csrc/conv_stream.h: per workgroup, the (segment, split, item, band, sub, cb) it visits, in order."""
    segs, wgs, u = [], 0, 0
    for s, c in zip(p.splits, p.counts):
        if c <= 0:
            continue
        per = (c + 7) // 8
        segs.append((wgs, s, u, c, per))
        wgs += per * 8 * s
        u += c
    total = wgs * cout_blocks
    walks = []
    for wg in range(grid):
        seen = []
        for vid in range(wg, total, grid):
            s8 = vid >> 3
            cb, x = s8 % cout_blocks, (s8 // cout_blocks) * 8 + (vid & 7)
            k = max(i for i, sg in enumerate(segs) if x >= sg[0])
            wb, sp, u0, nu, per = segs[k]
            local = x - wb
            slot = local >> 3
            j = slot // sp
            unit = (local & 7) * per + j
            if unit >= nu or j >= per:
                continue
            seen.append((k, sp, (u0 + unit) // bands, (u0 + unit) % bands, slot - j * sp, cb))
        walks.append(seen)
    return walks


def kind_of(L, it, split):
    """The body run_unit takes (csrc/conv_stream.h, conv_stream): 2 = 1x1, 1 = dilation 8 on a whole 14x14 map at split 1 / 2."""
    if L.ntaps == 1:
        return 2
    return 1 if (L.H == 14 and it.dil == 8 and split <= 2) else 0


def walk_facts(L, cus=0, forced=0):
    """What a launch reaches, from `plan` and `units_of`: the plan, the (split, KIND) set, whether a segment has holes,
    the longest run of units with pairwise different (band, dilation) geometry in a row that one workgroup walks, and
    whether some workgroup walks a gated and an ungated item back to back."""
    p = plan(len(L.items) * L.bands, L.cout_blocks, L.cin_chunks, L.ntaps, cus, forced)
    grid = grid_of(p, L.cout_blocks, cus)
    walks = units_of(p, grid, L.cout_blocks, L.bands)
    kinds, geo_run, gate_flip, visited = set(), 0, False, []
    for seen in walks:
        run, prev = 0, None
        for (k, sp, item, band, sub, cb) in seen:
            it = L.items[item]
            kinds.add((sp, kind_of(L, it, sp)))
            visited.append((item, band, sub, cb))
            geo = (band, it.dil if L.ntaps == 9 else 1)
            run = run + 1 if (prev is not None and geo != prev[0]) else 1
            geo_run = max(geo_run, run)
            if prev is not None and (it.gate >= 0) != prev[1]:
                gate_flip = True
            prev = (geo, it.gate >= 0)
    want = sorted((i, b, s, c) for k, (sp, n) in enumerate(zip(p.splits, p.counts)) for u in range(sum(p.counts[:k]), sum(p.counts[:k]) + n)
                  for i, b in [(u // L.bands, u % L.bands)] for s in range(sp) for c in range(L.cout_blocks))
    assert sorted(visited) == want, "the restated walk does not visit every (unit, sub, block) exactly once"
    return {"plan": p, "grid": grid, "kinds": kinds, "holes": any(c % 8 for c in p.counts), "geo_run": geo_run,
            "gate_flip": gate_flip, "longest_walk": max(len(s) for s in walks)}


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_conv_stream_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
DIL12 = (1, 2, 4, 8, 8, 1, 4, 2, 1, 8, 2, 4)


def mix_launch(H, ntaps, variant):
    """Exact group (a): a dozen items of mixed dilation (every band of a 28x28 item meets every pass pattern), masked
    and not, with and without bias, three weights in an order that returns to earlier ones.
    variant: fwd | fwd_relu (strides wider than the channels) | dgrad | acc | atomic."""
    wide = variant == "fwd_relu"
    items = []
    for i in range(12):
        it = Item(x=i % PX, w=(0, 1, 0, 2, 1, 2)[i % 6], dil=DIL12[i], mask=(i % PM if i % 3 != 1 else -1), bias=i % 4 != 2, out=i)
        if variant == "dgrad":
            it.gate = i % PG
        if variant == "acc":
            it.flags = ACCUMULATE
        if variant == "atomic":
            it.flags, it.out = ACCUMULATE | ATOMIC, i // 2
        items.append(it)
    return Launch(H, ntaps, 1, 1, 256 if wide else CB, 256 if wide else CB, 1 if wide else 0, items, note="mix " + variant)


def epilogue_launch(H, variant):
    """Exact group (b): six gated data-gradient items alternating dilation 8 with a second one.
    variant: sole | shared3 | noattn | dattn."""
    d2 = {"sole": 1, "shared3": 2, "noattn": 4, "dattn": 2}[variant]
    items = []
    for i in range(6):
        it = Item(x=i % PX, w=i % NWT, dil=8 if i % 2 == 0 else d2, gate=i % PG, bias=False, feats=i % PF)
        if variant == "sole":
            it.flags, it.attn, it.dfeats, it.dattn = MASKBWD | MB_SOLE, i % PM, i, i
        elif variant == "shared3":
            it.flags, it.attn, it.dfeats, it.dattn = MASKBWD, i % PM, i // 3, i
        elif variant == "noattn":
            it.flags, it.dfeats = MASKBWD | (MB_SOLE if i % 2 else 0), i
        else:
            it.flags, it.out, it.dattn = DATTN, i, i
            it.attn = i % PM if i % 3 != 1 else -1
        items.append(it)
    return Launch(H, 9, 1, 1, CB, CB, 0, items, note="epilogue " + variant)


def shape_launch(H, shape):
    """Exact group (c).  shape: stem | two_sources | two_sources_mask | classifier8 | classifier4 | cout2."""
    if shape == "stem":
        items = [Item(x=i, w=i % NWT, dil=(1, 4, 8)[i], mask=(-1, 0, 1)[i], out=i) for i in range(3)]
        return Launch(H, 9, 8, 1, 1024, CB, 1, items, note=shape)
    if shape.startswith("two_sources"):
        m = shape.endswith("mask")
        items = [Item(x=i % PX, x2=(i + 2) % PX, w=i % NWT, mask=(i % PM if m and i != 2 else -1), bias=i != 1, out=i) for i in range(5)]
        return Launch(H, 1, 2, 1, CB, CB, 1, items, note=shape)
    if shape.startswith("classifier"):
        cb = int(shape[-1])
        items = [Item(x=i, w=i % 2, out=i, bias=i != 1) for i in range(3)]
        return Launch(H, 1, 1, cb, CB, CB * cb, 0, items, note=shape)
    assert shape == "cout2"
    items = [Item(x=i, w=i, dil=(2, 8, 1)[i], mask=(0, -1, 2)[i], out=i) for i in range(3)]
    return Launch(H, 9, 1, 2, CB, 2 * CB, 1, items, note=shape)


def walk_launch(H, n, ntaps=9, sort=False, gates="none"):
    """Exact groups (d) and (e): n items under the planner.  Dilations cycle so that every segment holds every dilation;
    gates: none | alternate (a gated and an ungated item take turns: one and two ring slots per stage)."""
    cyc = (1, 8, 2, 8, 4, 1, 8)
    items = []
    for i in range(n):
        w = i * NWT // n if sort else (0, 1, 0, 2, 1, 2)[i % 6]
        it = Item(x=i % PX, w=w, dil=cyc[i % 7], mask=(i % PM if i % 3 != 2 else -1), bias=i % 5 != 3, out=i)
        if gates == "alternate" and i % 2 == 0:
            it.gate = i % PG
        items.append(it)
    return Launch(H, ntaps, 1, 1, CB, CB, 1 if gates == "none" else 0, items, note="walk %d%s" % (n, " sorted" if sort else ""))


# (cus, items, sorted by weight) of the planner launches at each map size, picked with `plan`; what they reach is asserted
# in tests/test_conv_reference.py::test_coverage
WALKS = {14: [(8, 13, False), (8, 14, True), (16, 13, False), (40, 53, True), (16, 25, False), (8, 53, False), (24, 19, True),
               (0, 3, False), (0, 12, True), (0, 22, False), (0, 40, False), (0, 50, True)],
         28: [(8, 3, False), (8, 13, True), (16, 7, False), (24, 10, True), (40, 13, False), (40, 26, True), (0, 1, False),
              (0, 3, False), (0, 5, True), (0, 10, False), (0, 11, True), (0, 22, False), (0, 49, True), (0, 53, False)]}
WALKS_1X1 = {14: [(8, 9), (8, 10), (8, 12), (0, 33)], 28: [(40, 11), (40, 12), (16, 6), (0, 17), (0, 33)]}
MIXED_SLOTS = {14: [(8, 21), (0, 21)], 28: [(8, 7), (0, 7)]}
MIX_VARIANTS = ("fwd", "fwd_relu", "dgrad", "acc", "atomic")
EPILOGUES = ("sole", "shared3", "noattn", "dattn")
SHAPES = ("stem", "two_sources", "two_sources_mask", "classifier8", "classifier4", "cout2")


@dataclass(frozen=True)
class Case:
    group: str
    name: str         # of the launch: cases of one (name, H) share a launch and so a reference
    H: int
    make: object      # () -> Launch without data
    forced: int = 0
    cus: int = 0
    entry: str = "cus"   # "plain": through pnmn_conv_nhwc, which is cus = 0

    @property
    def id(self):
        return "%dx%d-%s-split%d-cus%d%s" % (self.H, self.H, self.name.replace(" ", "_"), self.forced, self.cus,
                                             "-plain" if self.entry == "plain" else "")


def cases():
    """Every exact launch of tests/test_conv_stream_gpu.py, groups (a) to (e)."""
    from functools import partial
    out = []
    for H in (14, 28):
        for v in MIX_VARIANTS:
            for s in SPLITS_3X3:
                out.append(Case("a", "3x3 " + v, H, partial(mix_launch, H, 9, v), forced=s))
        out.append(Case("a", "3x3 fwd", H, partial(mix_launch, H, 9, "fwd"), entry="plain"))
        for v in ("fwd_relu", "dgrad", "atomic"):
            for s in SPLITS_1X1 + (6, 14, 26):
                out.append(Case("a", "1x1 " + v, H, partial(mix_launch, H, 1, v), forced=s))
        for v in EPILOGUES:
            for s in SPLITS_3X3:
                out.append(Case("b", "epilogue " + v, H, partial(epilogue_launch, H, v), forced=s))
        out.append(Case("b", "epilogue sole", H, partial(epilogue_launch, H, "sole"), entry="plain"))
        for sh in SHAPES:
            big = 26 if sh in ("stem", "cout2") else 8
            for s in (0, 1, big):
                out.append(Case("c", sh, H, partial(shape_launch, H, sh), forced=s))
        out.append(Case("c", "classifier4", H, partial(shape_launch, H, "classifier4"), entry="plain"))
        for (cus, n, srt) in WALKS[H]:
            out.append(Case("d", "walk %d%s" % (n, " sorted" if srt else ""), H, partial(walk_launch, H, n, 9, srt), cus=cus))
        for (cus, n) in WALKS_1X1[H]:
            out.append(Case("d", "walk 1x1 %d" % n, H, partial(walk_launch, H, n, 1, False), cus=cus))
        out.append(Case("d", "walk 13", H, partial(walk_launch, H, 13, 9, False), entry="plain"))
        for (cus, n) in MIXED_SLOTS[H]:
            out.append(Case("e", "mixed slots %d" % n, H, partial(walk_launch, H, n, 9, False, "alternate"), cus=cus))
    return out


def facts_of(case):
    return walk_facts(case.make(), case.cus, case.forced)
