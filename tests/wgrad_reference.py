"""Plain float64 reference of the grouped convolution weight gradient (include/probnmn_hip.h, pnmn_conv_wgrad):

    dW[n][tap][c] += sum_items sum_p dy[p][n] * (gate[p][n] > 0) * (x * xmask)[shift(p, tap, dil)][c]
    dbias[n]      += sum_items sum_p dy[p][n] * (gate[p][n] > 0)

with shift(p, tap, dil) = (y + (tap // 3 - 1) dil, x + (tap % 3 - 1) dil), zero outside the image (1x1: no shift).

`reference()` is written from that formula -- one matrix product per tap over explicitly shifted maps -- and calls
neither the library under test nor autograd.  `autograd_wgrad()` is the other road to the same numbers (F.conv2d's
weight gradient on the CPU): tests/test_wgrad_reference.py holds the two against each other in float64, and the GPU tests
use its float32 run as the yardstick of what float32 round-off costs on the same inputs.

A `Launch` describes one call of the entry point the way the kernels see it: items that point into small POOLS of maps
(an item is three indices: which x, which mask, which dy / gate map; the pools' sizes are pairwise coprime, so no two of
the first 1001 items are the same triple), jobs = runs of items that add into one of a few weights.
"""
from dataclasses import dataclass, field, replace
from typing import List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

CB = 128            # channels of a block
PX, PM, PD = 13, 7, 11  # pool sizes: x maps, masks, dy / gate maps


@dataclass
class Launch:
    H: int
    W: int
    taps: int                 # 9 or 1
    cin_blocks: int
    cout_blocks: int
    two_sources: bool         # input block 1 comes from a second tensor (x2)
    x_pool: torch.Tensor      # [PX][HW][cin_total] float32
    m_pool: torch.Tensor      # [PM][HW] float32
    dy_pool: torch.Tensor     # [PD][HW][cout_total] float32
    g_pool: torch.Tensor      # [PD][HW][cout_total] float32 (the ReLU gate map that goes with a dy map)
    ix: np.ndarray            # per item: x map
    im: np.ndarray            # per item: mask, or -1 (xmask == NULL)
    idy: np.ndarray           # per item: dy map
    use_gate: np.ndarray      # per item: bool (gate == NULL where False)
    dil: np.ndarray           # per item
    jobs: List[Tuple[int, int, int]]      # (item_begin, item_end, weight)
    n_weights: int
    has_bias: List[bool] = field(default_factory=list)

    @property
    def n_items(self):
        return len(self.ix)

    @property
    def cin(self):
        return self.cin_blocks * CB

    @property
    def cout(self):
        return self.cout_blocks * CB

    def items_of(self, weight):
        """Item indices that add into `weight`, job by job."""
        idx = [np.arange(b, e) for (b, e, w) in self.jobs if w == weight and e > b]
        return np.concatenate(idx) if idx else np.zeros(0, np.int64)


def integer_pools(seed, HW, cin, cout):
    """Small integers as float32: x, dy in [-3, 3], masks in {0, 1, 2}, gates in {-1, -0.0, 0, 1}.  Every product
    (at most 3 * 2 * 3 = 18) and every partial sum of fewer than 2^24 / 18 of them is exact in float32, in any order."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (PX, HW, cin), generator=g).float()
    m = torch.randint(0, 3, (PM, HW), generator=g).float()
    dy = torch.randint(-3, 4, (PD, HW, cout), generator=g).float()
    k = torch.randint(0, 4, (PD, HW, cout), generator=g)
    gate = torch.tensor([-1.0, -0.0, 0.0, 1.0])[k]
    return x, m, dy, gate


def normal_pools(seed, H, W, taps, cin, cout):
    """The data of tests/test_hip_kernels.py: ReLU'd normal x, sigmoid mask, normal dy, gate = a forward output
    (ReLU of a convolution of pool inputs with a random weight)."""
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    x = torch.relu(torch.randn(PX, HW, cin, generator=g))
    m = torch.sigmoid(torch.randn(PM, HW, generator=g))
    dy = torch.randn(PD, HW, cout, generator=g)
    k = 3 if taps == 9 else 1
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (taps * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xin = (x[:PD] * m[torch.arange(PD) % PM].unsqueeze(-1)).reshape(PD, H, W, cin).permute(0, 3, 1, 2)
    with torch.no_grad():
        y = torch.relu(F.conv2d(xin, w, b, padding=k // 2))
    gate = y.permute(0, 2, 3, 1).reshape(PD, HW, cout).contiguous()
    return x, m, dy, gate


def make_launch(H, taps, cin_blocks, cout_blocks, counts, weights, dils, *, two_sources=False, mask=True, gate=True,
                no_bias=(), pools=None, seed=0):
    """counts[j] items in job j, which adds into weights[j]; dils: per item, or one number, or a callable
    (job, item within the job) -> dilation.  mask / gate: True, False, or "some" (NULL for every third item)."""
    W = H
    counts = [int(c) for c in counts]
    n = int(sum(counts))
    if pools is None:
        pools = integer_pools(seed, H * W, cin_blocks * CB, cout_blocks * CB)
    i = np.arange(n)
    jobs, b = [], 0
    dil = np.ones(n, np.int32)
    for j, c in enumerate(counts):
        jobs.append((b, b + c, int(weights[j])))
        for k in range(c):
            dil[b + k] = dils(j, k) if callable(dils) else (dils if np.isscalar(dils) else dils[b + k])
        b += c
    im = (i % PM).astype(np.int64)
    ug = np.ones(n, bool)
    if mask is False:
        im[:] = -1
    elif mask == "some":
        im[i % 3 == 1] = -1
    if gate is False:
        ug[:] = False
    elif gate == "some":
        ug[i % 3 == 2] = False
    n_weights = int(max(weights)) + 1 if len(weights) else 1
    return Launch(H, W, taps, cin_blocks, cout_blocks, two_sources, *pools, ix=i % PX, im=im, idy=i % PD, use_gate=ug,
                  dil=dil, jobs=jobs, n_weights=n_weights, has_bias=[k not in no_bias for k in range(n_weights)])


def _operands(L, sel, dtype, device):
    """(x * xmask) [n][HW][cin] and dy * (gate > 0) [n][HW][cout] of items `sel`."""
    pick = lambda pool, idx: pool[torch.as_tensor(idx, dtype=torch.long, device=pool.device)].to(device=device, dtype=dtype)  # noqa: E731
    x = pick(L.x_pool, L.ix[sel])
    has_mask = torch.as_tensor(L.im[sel] >= 0, device=device).reshape(-1, 1)
    m = pick(L.m_pool, np.maximum(L.im[sel], 0))
    x = x * torch.where(has_mask, m, torch.ones_like(m)).unsqueeze(-1)
    dy = pick(L.dy_pool, L.idy[sel])
    open_ = (pick(L.g_pool, L.idy[sel]) > 0) | ~torch.as_tensor(L.use_gate[sel], device=device).reshape(-1, 1, 1)
    return x, dy * open_.to(dtype)


def shifted(x, H, W, tap, dil):
    """x [n][HW][C] -> the map tap `tap` of a 3x3 convolution of dilation `dil` reads at each pixel, zero outside."""
    n, _, C = x.shape
    xi = x.reshape(n, H, W, C)
    out = torch.zeros_like(xi)
    oy, ox = (tap // 3 - 1) * dil, (tap % 3 - 1) * dil
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y1 > y0 and x1 > x0:
        out[:, y0:y1, x0:x1] = xi[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out.reshape(n, H * W, C)


def reference(L, device="cpu", chunk=32):
    """([dW of every weight: [cout][taps][cin] float64], [dbias: [cout] float64])."""
    dws, dbs = [], []
    if torch.device(device).type != "cpu":  # (the pools travel once, not chunk by chunk)
        L = replace(L, x_pool=L.x_pool.to(device), m_pool=L.m_pool.to(device), dy_pool=L.dy_pool.to(device), g_pool=L.g_pool.to(device))
    for k in range(L.n_weights):
        dw = torch.zeros(L.cout, L.taps, L.cin, dtype=torch.float64, device=device)
        db = torch.zeros(L.cout, dtype=torch.float64, device=device)
        items = L.items_of(k)
        for c0 in range(0, len(items), chunk):
            sel = items[c0:c0 + chunk]
            x, dyg = _operands(L, sel, torch.float64, device)
            db += dyg.sum((0, 1))
            for d in np.unique(L.dil[sel]) if L.taps == 9 else [0]:
                pick = torch.as_tensor(np.nonzero(L.dil[sel] == d)[0] if L.taps == 9 else np.arange(len(sel)), device=device)
                xd, dd = x[pick], dyg[pick].reshape(-1, L.cout)
                for t in range(L.taps):
                    xs = shifted(xd, L.H, L.W, t, int(d)) if L.taps == 9 else xd
                    dw[:, t, :] += dd.t() @ xs.reshape(-1, L.cin)
        dws.append(dw)
        dbs.append(db)
    return dws, dbs


def autograd_wgrad(L, dtype, through_relu=None):
    """The same gradients from CPU autograd of F.conv2d(x * xmask, w, b, padding=d, dilation=d) in `dtype`, one backward
    pass per (weight, dilation); the ReLU's backward is dy * (gate > 0).  With `through_relu` = [(w, b) per weight] the
    ReLU is autograd's own (F.relu of the forward with those parameters) and the launch's gate maps must be that forward."""
    ksz = 3 if L.taps == 9 else 1
    dws, dbs = [], []
    for k in range(L.n_weights):
        if through_relu is None:
            w = torch.zeros(L.cout, L.cin, ksz, ksz, dtype=dtype, requires_grad=True)
            b = torch.zeros(L.cout, dtype=dtype, requires_grad=True)
        else:
            w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in through_relu[k])
        items = L.items_of(k)
        for d in (np.unique(L.dil[items]) if L.taps == 9 else [1]):
            sel = items[L.dil[items] == d] if L.taps == 9 else items
            if len(sel) == 0:
                continue
            x, dyg = _operands(L, sel, dtype, "cpu")
            n = len(sel)
            xin = x.reshape(n, L.H, L.W, L.cin).permute(0, 3, 1, 2)
            y = F.conv2d(xin, w, b, padding=int(d) * (ksz // 2), dilation=int(d))
            if through_relu is None:
                y.backward(dyg.reshape(n, L.H, L.W, L.cout).permute(0, 3, 1, 2))
            else:
                dy = L.dy_pool[torch.as_tensor(L.idy[sel], dtype=torch.long)].to(dtype)
                F.relu(y).backward(dy.reshape(n, L.H, L.W, L.cout).permute(0, 3, 1, 2))
        gw = w.grad if w.grad is not None else torch.zeros_like(w)
        gb = b.grad if b.grad is not None else torch.zeros_like(b)
        dws.append(gw.permute(0, 2, 3, 1).reshape(L.cout, L.taps, L.cin).contiguous())
        dbs.append(gb.clone())
    return dws, dbs


U32 = 2.0 ** -24  # unit round-off of float32


def ulp32(v):
    """Spacing of float32 at magnitude v (float64 tensor, v >= 0)."""
    return torch.exp2(torch.floor(torch.log2(v.clamp_min(2.0 ** -126))) - 23)


def chain_sigma(L, weight, device="cpu", chunk=16, unit_px=None, chain_starts=None):
    """Standard deviation (largest over the entries of dW) of the round-off of a kernel that CHAINS its float32 additions:
    one accumulator per entry runs from zero over a run of UNITS (an item's block of `unit_px` pixels; default: the whole
    item) of the weight's items in job order, and every chain's result is added into dW, one rounding each, in any order.
    `chain_starts`: the unit indices at which an accumulator starts (default: every job's first unit).  An addition
    rounds its partial sum S to nearest: an error uniform over one ulp(S) = 2^(floor(log2 |S|) - 23), variance
    ulp(S)^2 / 12, independent between additions, one rounding counted per product (an upper count: an MFMA adds four
    products per accumulation).  So per entry

        var <= 1 / 12 * ( sum over units u:  unit_px * ulp(max(|S_{u-1}|, |S_u|) + T_u)^2   +   n_chains * ulp(sum over chains |C|)^2 )

    with S_u the chain's partial sum behind unit u, T_u = sum over the unit's pixels of |dy x| (no partial sum inside the
    unit leaves S_{u-1} +- T_u), C a chain's result.  Computed from the inputs alone, in float64."""
    if torch.device(device).type != "cpu":
        L = replace(L, x_pool=L.x_pool.to(device), m_pool=L.m_pool.to(device), dy_pool=L.dy_pool.to(device), g_pool=L.g_pool.to(device))
    HW = L.H * L.W
    px = unit_px or HW
    nb = HW // px
    assert nb * px == HW
    items = L.items_of(weight)
    if chain_starts is None:
        starts, u = set(), 0
        for (b, e, w) in L.jobs:
            if w == weight and e > b:
                starts.add(u)
                u += (e - b) * nb
    else:
        starts = {int(k) for k in chain_starts if 0 <= k < len(items) * nb}
    starts.add(0)
    q = torch.zeros(L.cout, L.taps, L.cin, dtype=torch.float64, device=device)
    jsum, s = torch.zeros_like(q), torch.zeros_like(q)
    for c0 in range(0, len(items), chunk):
        sel = items[c0:c0 + chunk]
        n, u0 = len(sel), c0 * nb
        x, dyg = _operands(L, sel, torch.float64, device)
        cuts = [0] + sorted(k - u0 for k in starts if u0 < k < u0 + n * nb) + [n * nb]
        d4 = dyg.reshape(n, nb, px, L.cout)
        for t in range(L.taps):
            xs = x
            if L.taps == 9:
                xs = torch.zeros_like(x)
                for d in np.unique(L.dil[sel]):
                    pick = torch.as_tensor(np.nonzero(L.dil[sel] == d)[0], device=device)
                    xs[pick] = shifted(x[pick], L.H, L.W, t, int(d))
            x4 = xs.reshape(n, nb, px, L.cin)
            p = torch.einsum("ibpn,ibpc->ibnc", d4, x4).reshape(n * nb, L.cout, L.cin)
            tmag = torch.einsum("ibpn,ibpc->ibnc", d4.abs(), x4.abs()).reshape(n * nb, L.cout, L.cin)
            for a, b in zip(cuts[:-1], cuts[1:]):
                if u0 + a in starts and u0 + a > 0:  # the chain before this one ends here
                    jsum[:, t] += s[:, t].abs()
                    s[:, t] = 0
                after = s[:, t].unsqueeze(0) + p[a:b].cumsum(0)
                before = torch.cat((s[:, t].unsqueeze(0), after[:-1]), 0)
                q[:, t] += px * (ulp32(torch.maximum(before.abs(), after.abs()) + tmag[a:b]) ** 2).sum(0)
                s[:, t] = after[-1]
    jsum += s.abs()
    var = (q + len(starts) * ulp32(jsum) ** 2) / 12.0
    return float(var.max().sqrt())
