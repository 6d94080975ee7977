"""Float64 references of the point-wise NMN kernels (csrc/pointwise.hip, csrc/pointwise_body.h), written from the formulas
of include/probnmn_hip.h with plain torch operations and independent of the library; the case lists of
tests/test_pointwise_gpu.py; and a restatement of the launch-shape rules of csrc/pointwise_plan.h, from which
tests/test_pointwise_reference.py asserts what the case lists reach.

Every reference takes a dtype: float64 is the reference, float32 on the CPU gives err32, the yardstick of the round-off
cases.  EXACT cases hold small integers as float32; exact_ok asserts that the largest magnitude any order of additions
can reach stays below 2^24, so float32 sums, atomics included, are exact and the comparison is torch.equal.
"""
import math

import torch

C = 128
F64 = torch.float64


def exact_ok(bound, what=""):
    """The largest magnitude a partial sum of this case can reach, in any order, is an integer (or half-integer) float32
    holds exactly."""
    assert bound < 2 ** 24, "%s: sums may reach %g >= 2^24: not exact in float32" % (what, bound)
    return bound


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def rint(g, lo, hi, *shape):
    """Integers in [lo, hi] as float32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


# ---------------------------------------------------------------------------------------------------------------------
# conv1x1 (128 -> 1) + sigmoid
# ---------------------------------------------------------------------------------------------------------------------
DOT1_HW = [1, 56, 57, 104, 105, 196, 209, 784]   # rounds of 104 pixels forward, 56 backward: one short, full, full + 1
DOT1_ITEMS = 3


def dot1_data(HW, seed=0):
    """dout has mean 2 (a fortieth of it negative) and the dw / db prefills are positive: dw and db, sums over every pixel of
    every item, then do not cancel.  The round-off figure is relative to max|ref| of a tensor, and db is a tensor of one
    element: with dout of mean 0 it came out as -0.056 from item sums of magnitude 2, and two float32 roundings at that
    magnitude -- no defect -- were 32 err32 on that scale."""
    g = gen(1000 + HW + seed)
    n = DOT1_ITEMS
    return dict(x=torch.relu(torch.randn(n, HW, C, generator=g)), w=torch.randn(C, generator=g) * 0.2, b=torch.randn(1, generator=g),
                dout=torch.randn(n, HW, generator=g) + 2, dw_pre=torch.randn(C, generator=g).abs(), db_pre=torch.randn(1, generator=g).abs())


def dot1_reference(d, dtype=F64):
    """out[p] = sigmoid(b + sum_c in[p][c] w[c]); dz = dout out (1 - out); din = dz w; dw += sum_p dz in; db += sum_p dz
    (all items add into the one dw / db)."""
    x, w, b, dout = (d[k].to(dtype) for k in ("x", "w", "b", "dout"))
    out = sigmoid((x * w).sum(-1) + b)
    dz = dout * out * (1 - out)
    return dict(out=out, din=dz.unsqueeze(-1) * w, dw=d["dw_pre"].to(dtype) + (dz.unsqueeze(-1) * x).sum((0, 1)),
                db=d["db_pre"].to(dtype) + dz.sum().reshape(1))


# ---------------------------------------------------------------------------------------------------------------------
# SameModule
# ---------------------------------------------------------------------------------------------------------------------
SAME_HW = [1, 7, 196, 784]
# attention of an item: random; the maximum at the last pixel; equal maxima at two pixels; all equal (pixel 0 wins);
# "nodattn": random, and the item's dattn is NULL
SAME_TIES = {"tie255_256": (255, 256), "tie0_783": (0, 783)}


def same_kinds(HW):
    return ["random", "last", "allequal", "nodattn"] + [k for k, (a, b) in SAME_TIES.items() if b < HW]


def same_data(HW, seed=0):
    g = gen(2000 + HW + seed)
    kinds = same_kinds(HW)
    n = len(kinds)
    attn = torch.sigmoid(torch.randn(n, HW, generator=g) * 2)
    for i, k in enumerate(kinds):
        if k == "last":
            attn[i, HW - 1] = 1.5
        elif k == "allequal":
            attn[i] = 0.25
        elif k in SAME_TIES:
            attn[i, SAME_TIES[k][0]] = attn[i, SAME_TIES[k][1]] = 1.5
    return dict(kinds=kinds, feats=torch.relu(torch.randn(n, HW, C, generator=g)), attn=attn, w=torch.randn(C + 1, generator=g) * 0.1,
                b=torch.randn(1, generator=g), dout=torch.randn(n, HW, generator=g) + 2, dfeats_pre=torch.randn(n, HW, C, generator=g),
                dattn_pre=torch.randn(n, HW, generator=g), dw_pre=torch.randn(C + 1, generator=g).abs(), db_pre=torch.randn(1, generator=g).abs())


def first_argmax(v):
    """Index of the first maximum of a vector, in scan order."""
    return int(torch.nonzero(v == v.max()).flatten()[0])


def same_expected_argmax(kind, HW):
    return {"last": HW - 1, "allequal": 0, "tie255_256": 255, "tie0_783": 0}.get(kind)


def same_reference(d, dtype=F64):
    """j = first arg-max of attn; v = feats[j]; out[p] = sigmoid(b + sum_c w[c] feats[p][c] v[c] + w[128] attn[p]).
    Backward, dz = dout out (1 - out), s[c] = sum_p dz[p] feats[p][c]:
      dfeats[p][c] += dz[p] w[c] v[c], and dfeats[j][c] += s[c] w[c] (through v);  dattn[p] += dz[p] w[128];
      dw[c] += s[c] v[c]; dw[128] += sum_p dz[p] attn[p]; db += sum_p dz[p]  (every item adds into the one dw / db)."""
    feats, attn, w, b, dout = (d[k].to(dtype) for k in ("feats", "attn", "w", "b", "dout"))
    n, HW = attn.shape
    out = torch.empty(n, HW, dtype=dtype)
    dfeats, dattn = d["dfeats_pre"].to(dtype).clone(), d["dattn_pre"].to(dtype).clone()
    dw, db = d["dw_pre"].to(dtype).clone(), d["db_pre"].to(dtype).clone()
    js = []
    for i in range(n):
        j = first_argmax(d["attn"][i])
        js.append(j)
        v = feats[i, j]
        out[i] = sigmoid((feats[i] * (w[:C] * v)).sum(-1) + w[C] * attn[i] + b)
        dz = dout[i] * out[i] * (1 - out[i])
        s = (dz.unsqueeze(-1) * feats[i]).sum(0)
        dfeats[i] += dz.unsqueeze(-1) * (w[:C] * v)
        dfeats[i, j] += s * w[:C]
        if d["kinds"][i] != "nodattn":
            dattn[i] += dz * w[C]
        dw[:C] += s * v
        dw[C] += (dz * attn[i]).sum()
        db += dz.sum()
    rowj = torch.stack([dfeats[i, j] for i, j in enumerate(js)])
    return dict(out=out, dfeats=dfeats, dfeats_row_j=rowj, dattn=dattn, dw=dw, db=db, j=js)


# ---------------------------------------------------------------------------------------------------------------------
# And / Or
# ---------------------------------------------------------------------------------------------------------------------
MINMAX_HW = [1, 97, 98, 99, 196, 784]   # forward rounds of 98 pixels (448 threads x 7 pieces of 4 channels)
MINMAX_ITEMS = [(ac, bc, is_max) for is_max in (0, 1) for (ac, bc) in ((1, 1), (1, C), (C, 1), (C, C))]
MINMAX_NULLS = ["none", "alternate"]    # "alternate": item i has da == NULL (i even) or db == NULL (i odd)


def minmax_data(HW, seed=0, nan=False):
    """Integers in [-2, 2]: a fifth of all positions tie, broadcast or not.  dout is even, so the halves of a tie are whole."""
    g = gen(3000 + HW + seed)
    items = []
    for (ac, bc, is_max) in MINMAX_ITEMS:
        oc = max(ac, bc)
        a, b = rint(g, -2, 2, HW, ac), rint(g, -2, 2, HW, bc)
        if nan:
            pm, ch = HW // 2, 5
            a.view(-1)[0] = float("nan")                                  # NaN in a alone
            b.view(-1)[-1] = float("nan")                                 # in b alone (or in both, where HW * channels == 1)
            a[pm, ch if ac == C else 0] = b[pm, ch if bc == C else 0] = float("nan")   # in both
        items.append(dict(ac=ac, bc=bc, is_max=is_max, a=a, b=b, dout=2 * rint(g, -2, 2, HW, oc), da_pre=rint(g, -3, 3, HW, ac),
                          db_pre=rint(g, -3, 3, HW, bc)))
    return items


def minmax_fwd_reference(it, dtype=F64):
    """Elementwise min / max with 1 <-> C broadcast; NaN in either operand gives NaN (as torch.min / torch.max)."""
    a, b = it["a"].to(dtype), it["b"].to(dtype)
    r = torch.where(a > b, a, b) if it["is_max"] else torch.where(a < b, a, b)
    return torch.where(torch.isnan(a) | torch.isnan(b), torch.full_like(r, float("nan")), r)


def minmax_bwd_reference(it, nulls=(False, False), dtype=F64):
    """The gradient goes to the selected operand, half to each at a tie, summed over channels for a broadcast operand;
    da / db are added into.  A NULL side keeps its prefill (nothing is read or written there)."""
    a, b, g = it["a"].to(dtype), it["b"].to(dtype), it["dout"].to(dtype)
    wins = (a > b) if it["is_max"] else (a < b)
    tie = a == b
    zero = torch.zeros_like(g)
    ga = torch.where(tie, 0.5 * g, torch.where(wins, g, zero))
    gb = torch.where(tie, 0.5 * g, torch.where(wins, zero, g))
    if it["ac"] == 1:
        ga = ga.sum(-1, keepdim=True)
    if it["bc"] == 1:
        gb = gb.sum(-1, keepdim=True)
    exact_ok(amax(it["da_pre"]) + C * amax(g), "minmax")
    da = it["da_pre"].to(dtype) + (0 if nulls[0] else ga)
    db = it["db_pre"].to(dtype) + (0 if nulls[1] else gb)
    return da, db


def minmax_nulls(variant, i):
    return (False, False) if variant == "none" else (i % 2 == 0, i % 2 == 1)


# ---------------------------------------------------------------------------------------------------------------------
# backward of feats * attn: pnmn_mask_bwd (atomics) and pnmn_feat_grad_gather (one writer per example)
# ---------------------------------------------------------------------------------------------------------------------
MASKBWD_HW = [1, 9, 196, 784]
# (dfeats map, dattn map or -1 for attn == NULL): five items add into dfeats map 0, two into dattn map 0
MASKBWD_ITEMS = [(0, 0), (0, 0), (0, -1), (0, 1), (0, -1), (1, 2), (1, -1)]


def maskbwd_data(HW, seed=0):
    g = gen(4000 + HW + seed)
    n = len(MASKBWD_ITEMS)
    return dict(dx=rint(g, -2, 2, n, HW, C), feats=rint(g, -2, 2, n, HW, C), attn=rint(g, 0, 2, n, HW),
                dfeats_pre=rint(g, -3, 3, 2, HW, C), dattn_pre=rint(g, -3, 3, 3, HW))


def maskbwd_reference(d, dtype=F64):
    """dattn[p] += sum_c dx[p][c] feats[p][c]; dfeats[p][c] += dx[p][c] attn[p]; attn == NULL: dfeats += dx, no dattn."""
    dfeats, dattn = d["dfeats_pre"].to(dtype).clone(), d["dattn_pre"].to(dtype).clone()
    for i, (f, a) in enumerate(MASKBWD_ITEMS):
        dx = d["dx"][i].to(dtype)
        if a < 0:
            dfeats[f] += dx
        else:
            dfeats[f] += dx * d["attn"][i].to(dtype).unsqueeze(-1)
            dattn[a] += (dx * d["feats"][i].to(dtype)).sum(-1)
    exact_ok(amax(d["dfeats_pre"]) + len(MASKBWD_ITEMS) * amax(d["dx"]) * amax(d["attn"]), "mask_bwd dfeats")
    exact_ok(amax(d["dattn_pre"]) + len(MASKBWD_ITEMS) * C * amax(d["dx"]) * amax(d["feats"]), "mask_bwd dattn")
    return dfeats, dattn


def sparse_counts(n, where):
    c = [0] * n
    for e, k in where.items():
        c[e] = k
    return c


# (name, n_examples, HW, items per example)
GATHER_CASES = [("one example", 1, 196, [5]), ("counts 0..9", 7, 196, [0, 1, 3, 4, 5, 8, 9])]
GATHER_CASES += [("ends empty HW %d" % hw, 7, hw, [0, 9, 4, 0, 1, 8, 0]) for hw in (47, 48, 96, 196, 784)]
GATHER_CASES += [("128 examples", 128, 196, sparse_counts(128, {3: 4, 64: 5, 127: 1})),
                 ("256 examples", 256, 196, sparse_counts(256, {1: 3, 255: 8})),
                 ("512 examples", 512, 196, sparse_counts(512, {0: 1, 300: 9, 510: 4}))]
GATHER_DX_POOL, GATHER_ATTN_POOL = 5, 3


def gather_items(counts):
    """(example, dx map, attn map or -1) per item, sorted by example; every third item has attn == NULL, so groups of four
    mix both kinds."""
    items, i = [], 0
    for e, k in enumerate(counts):
        for _ in range(k):
            items.append((e, i % GATHER_DX_POOL, -1 if i % 3 == 1 else i % GATHER_ATTN_POOL))
            i += 1
    return items


def gather_data(n_examples, HW, seed=0):
    g = gen(5000 + HW + 7 * n_examples + seed)
    return dict(dx=rint(g, -2, 2, GATHER_DX_POOL, HW, C), attn=rint(g, 0, 2, GATHER_ATTN_POOL, HW), pre=rint(g, -3, 3, n_examples, HW, C))


def gather_reference(d, counts, device="cpu", dtype=F64):
    """gfeat[e][p][c] += sum over the items of example e of dx[p][c] attn[p] (attn == NULL: ones); an example without
    items keeps its prefill."""
    out = d["pre"].to(device=device, dtype=dtype).clone()
    dx, attn = d["dx"].to(device=device, dtype=dtype), d["attn"].to(device=device, dtype=dtype)
    for (e, x, a) in gather_items(counts):
        out[e] += dx[x] if a < 0 else dx[x] * attn[a].unsqueeze(-1)
    exact_ok(amax(d["pre"]) + max(counts) * amax(d["dx"]) * amax(d["attn"]), "gather")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# accumulate / set_rows
# ---------------------------------------------------------------------------------------------------------------------
AXPY_N = [1, 3, 4, 5, 1023, 25088, 25091]


def axpy_data(seed=0):
    g = gen(6000 + seed)
    return [dict(n=n, src=rint(g, -1000, 1000, n), dst=rint(g, -1000, 1000, n)) for n in AXPY_N]


def accumulate_reference(it, dtype=F64):
    exact_ok(amax(it["src"]) + amax(it["dst"]), "accumulate")
    return it["dst"].to(dtype) + it["src"].to(dtype)


def set_rows_reference(it, null_src, dtype=F64):
    return torch.zeros(it["n"], dtype=dtype) if null_src else it["src"].to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# weight transposition, layout
# ---------------------------------------------------------------------------------------------------------------------
WTRANS_SHAPES = [(128, 9, 128), (1024, 1, 128), (128, 1, 256), (5, 9, 3), (33, 2, 65), (256, 9, 128)]   # [cout][taps][cin]


def wtrans_data(shape):
    """Every element its own value (an index swapped between cout and cin shows wherever it lands)."""
    cout, taps, cin = shape
    exact_ok(cout * taps * cin, "transpose")
    return torch.arange(cout * taps * cin, dtype=torch.float32).reshape(cout, taps, cin) + 1


def wtrans_reference(src):
    """[cout][t][cin] -> [cin][taps - 1 - t][cout]"""
    return src.permute(2, 1, 0).flip(1).contiguous()


LAYOUT_C = [1, 3, 64, 66, 68, 128, 132]
LAYOUT_HW = [1, 3, 4, 49, 196, 447, 448, 452, 785, 900]   # (452: HW a multiple of 4 whose second chunk starts at 226)
LAYOUT_N = 2
LAYOUT_ROWS = {"repeated": [1, 1], "descending": [4, 2, 0], "two of five": [3, 1]}   # out of a source batch of 5
LAYOUT_ROWS_SHAPES = [(3, 49), (66, 196), (128, 448), (132, 900), (64, 785)]


def layout_data(n, Cn, HW, seed=0):
    g = gen(7000 + 13 * Cn + HW + seed)
    return torch.randn(n, Cn, HW, generator=g)


def to_nhwc_reference(x, rows=None):
    x = x if rows is None else x[torch.tensor(rows)]
    return x.permute(0, 2, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# ReLU-gated MaxPool2d(2, 2) + Flatten
# ---------------------------------------------------------------------------------------------------------------------
POOL_MAPS = [(2, 2), (3, 3), (2, 5), (5, 2), (4, 6), (14, 14), (15, 15), (16, 16), (18, 18), (28, 28), (29, 29), (29, 15), (4, 74), (14, 74)]
POOL_C = [64, 128]
POOL_N = 2


def pool_data(H, W, Cn, seed=0):
    """Integers in [-2, 3]: windows with positive ties, all-zero and all-negative windows all over the map, and three
    forced ones in window (0, 0): channel 0 all zero, channel 1 all negative, channel 2 four equal positives."""
    g = gen(8000 + 100 * H + W + Cn + seed)
    x = rint(g, -2, 3, POOL_N, H, W, Cn)
    x[:, :2, :2, 0] = 0.0
    x[:, :2, :2, 1] = -1.0
    x[:, 1, 1, 1] = -2.0
    x[:, :2, :2, 2] = 3.0
    return dict(x=x, dout=rint(g, -3, 3, POOL_N, Cn * (H // 2) * (W // 2)))


def pool_scan(x):
    """(best, index) of every 2x2 window in scan order (0: top left, 1: top right, 2: bottom left, 3: bottom right), the first
    maximum winning: [n][PH][PW][C] each."""
    n, H, W, Cn = x.shape
    PH, PW = H // 2, W // 2
    q = [x[:, dy:2 * PH:2, dx:2 * PW:2] for dy in (0, 1) for dx in (0, 1)]
    best, bi = q[0].clone(), torch.zeros(q[0].shape, dtype=torch.long)
    for k in (1, 2, 3):
        better = q[k] > best
        best = torch.where(better, q[k], best)
        bi = torch.where(better, torch.full_like(bi, k), bi)
    return best, bi


def pool_fwd_reference(x, dtype=F64):
    """in [n][H][W][C] -> out [n][C * PH * PW] in NCHW-flatten order (the ReLU was applied by the producer: a plain maximum)."""
    best, _ = pool_scan(x.to(dtype))
    return best.permute(0, 3, 1, 2).reshape(x.shape[0], -1)


def pool_bwd_reference(x, dout, dtype=F64):
    """dout goes to the first maximum of its window where that maximum is positive (the ReLU gate); everything else,
    the odd row and column included, is zero."""
    n, H, W, Cn = x.shape
    PH, PW = H // 2, W // 2
    best, bi = pool_scan(x.to(dtype))
    g = dout.to(dtype).reshape(n, Cn, PH, PW).permute(0, 2, 3, 1)
    gv = torch.where(best > 0, g, torch.zeros_like(g))
    din = torch.zeros(n, H, W, Cn, dtype=dtype)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        din[:, dy:2 * PH:2, dx:2 * PW:2] = torch.where(bi == k, gv, torch.zeros_like(gv))
    return din


# ---------------------------------------------------------------------------------------------------------------------
# answer loss
# ---------------------------------------------------------------------------------------------------------------------
LOSS_N = [1, 64, 65]
LOSS_A = [1, 2, 28]
LOSS_NULLS = ["none", "valid", "predictions", "answers", "dlogits"]
LOSS_INVALID = 3.33


def loss_data(n, A, seed=0):
    """Rows b % 4 == 1 carry two equal maxima (the first must be predicted), rows b % 4 == 2 logits of +-80 (several equal
    maxima again); every fifth row is invalid.  Answers stay in range."""
    g = gen(9000 + 31 * n + A + seed)
    z = torch.randn(n, A, generator=g) * 3
    for b in range(n):
        if b % 4 == 1 and A >= 2:
            k = sorted(torch.randperm(A, generator=g)[:2].tolist())
            z[b, k[0]] = z[b, k[1]] = float(z[b].max()) + 0.5
        if b % 4 == 2 or (n == 1 and A > 2):
            z[b] = 80.0 * (2.0 * torch.randint(0, 2, (A,), generator=g).float() - 1.0)
    valid = torch.tensor([0 if b % 5 == 3 else 1 for b in range(n)], dtype=torch.int32)
    return dict(logits=z, answers=torch.randint(0, A, (n,), generator=g), valid=valid, scale=1.0 / n, unknown=A)


def loss_reference(d, nulls="none", dtype=F64):
    """logprobs = log_softmax(logits[b]); pred[b] = first arg-max; loss[b] = -logprobs[answer[b]] (answers == NULL: minus the
    largest logprob, and no gradient); invalid rows: pred = unknown_index, loss = 3.33, gradient 0;
    dlogits[b] = (softmax - onehot) * scale."""
    z = d["logits"].to(dtype)
    n, A = z.shape
    mx = z.max(1).values
    idx = torch.arange(A).expand(n, A)
    am = torch.where(d["logits"] == d["logits"].max(1, keepdim=True).values, idx, torch.full_like(idx, A)).min(1).values
    lse = mx + torch.log(torch.exp(z - mx.unsqueeze(1)).sum(1))
    ok = torch.ones(n, dtype=torch.bool) if nulls == "valid" else d["valid"] != 0
    pred = torch.where(ok, am, torch.full_like(am, d["unknown"]))
    if nulls == "answers":
        l, dl = lse - mx, torch.zeros(n, A, dtype=dtype)
    else:
        l = lse - z.gather(1, d["answers"].unsqueeze(1)).squeeze(1)
        onehot = torch.zeros(n, A, dtype=dtype).scatter_(1, d["answers"].unsqueeze(1), 1.0)
        dl = (torch.exp(z - lse.unsqueeze(1)) - onehot) * d["scale"]
        dl = torch.where(ok.unsqueeze(1), dl, torch.zeros_like(dl))
    loss = torch.where(ok, l, torch.full_like(l, LOSS_INVALID))
    return dict(loss=loss, dlogits=dl, predictions=pred)


# ---------------------------------------------------------------------------------------------------------------------
# clamp + Adam
# ---------------------------------------------------------------------------------------------------------------------
ADAM_N = [1, 3, 4, 5, 1031, 100003]
ADAM_FIRST_STEP = [1, 2, 5, 10, 100, 1000]    # the Adam step count of each item at the first of the three steps
ADAM_STEPS = 3
ADAM_CLAMP = [0.0, 5.0]
ADAM_WD = [0.0, 0.01]
ADAM_BLOCKS = [1, 3, 2048]
ADAM_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def f32(v):
    """A hyperparameter as the kernel holds it: pnmn_clamp_adam rounds lr, the betas, eps, weight_decay and clamp to float32
    on entry (include/probnmn_hip.h), and 1 - beta is formed from the rounded beta."""
    return float(torch.tensor(v, dtype=torch.float32))


def adam_data(seed=0):
    g = gen(10000 + seed)
    return [dict(n=n, first=s, param=torch.randn(n, generator=g), exp_avg=torch.randn(n, generator=g) * 0.1,
                 exp_avg_sq=torch.rand(n, generator=g) * 0.1, grads=[torch.randn(n, generator=g) * 4 for _ in range(ADAM_STEPS)])
            for n, s in zip(ADAM_N, ADAM_FIRST_STEP)]


def adam_bias_corrections(step, beta1=ADAM_HYPER["beta1"], beta2=ADAM_HYPER["beta2"]):
    """(bc1, bc2_sqrt) of a step count, in double as torch.optim.Adam forms them on the host."""
    return 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)


def adam_reference(it, clamp, wd, dtype=F64, bc_betas=None):
    """torch.optim.Adam (no amsgrad) after clamp: g = clamp(g) + wd p; m += (g - m)(1 - beta1); v = beta2 v + (1 - beta2) g^2;
    p -= lr / bc1 * m / (sqrt(v) / bc2_sqrt + eps), three steps from the item's first step count -- at the hyperparameters
    the kernel holds, ADAM_HYPER rounded to float32 (f32).  The bias corrections are an input of their own (fields of the
    item, formed by the caller from the unrounded betas); `bc_betas` forms them from other betas."""
    lr, beta1, beta2, eps = (f32(ADAM_HYPER[k]) for k in ("lr", "beta1", "beta2", "eps"))
    clamp, wd = f32(clamp), f32(wd)
    p, m, v = (it[k].to(dtype).clone() for k in ("param", "exp_avg", "exp_avg_sq"))
    for k in range(ADAM_STEPS):
        bc1, bc2s = adam_bias_corrections(it["first"] + k, *(bc_betas or (ADAM_HYPER["beta1"], ADAM_HYPER["beta2"])))
        g = it["grads"][k].to(dtype)
        if clamp > 0:
            g = g.clamp(-clamp, clamp)
        g = g + wd * p
        m = m + (g - m) * (1.0 - beta1)
        v = v * beta2 + (1.0 - beta2) * g * g
        p = p - (lr / bc1) * (m / (v.sqrt() / bc2s + eps))
    return dict(param=p, exp_avg=m, exp_avg_sq=v)


# ---------------------------------------------------------------------------------------------------------------------
# the launch-shape rules of csrc/pointwise_plan.h, restated
# ---------------------------------------------------------------------------------------------------------------------
LDS_BUDGET = 112 * 1024
LDS_NO_OPT_IN = 64 * 1024


def cdiv(a, b):
    return -(-a // b)


def layout_chunk(HW):
    parts = 1
    while 64 * (cdiv(HW, parts) + 1) * 4 > LDS_BUDGET:
        parts += 1
    return cdiv(HW, parts)


def pool_band(H, W):
    rb = (H + 1) & ~1
    while rb > 2 and rb * W * 65 * 4 > LDS_BUDGET:
        rb = ((rb // 2) + 1) & ~1
    return rb


def pool_bwd_even_rows(H, W):
    PH, PW = H // 2, W // 2
    return PH if PH * PW <= 64 else min(PH, 7)


def pool_bwd_even_lds(H, W):
    return pool_bwd_even_rows(H, W) * (W // 2) * 65 * 4


def pool_bwd_takes_even(H, W):
    return H % 2 == 0 and W % 2 == 0 and pool_bwd_even_lds(H, W) <= LDS_NO_OPT_IN


def gather_parts(n_examples, HW):
    parts = 1
    while n_examples * parts < 512 and parts < 8 and HW // (parts * 2) >= 24:
        parts *= 2
    return parts


def wtrans_tiles(cout, cin, ntaps):
    return cdiv(cin, 32) * cdiv(cout, 32) * ntaps


WTRANS_GRID = 256


def layout_facts(Cn, HW):
    """The branches of layout_kernel the workgroups of one launch take (both directions share the conditions)."""
    PT = layout_chunk(HW)
    facts = {"chunks %d" % cdiv(HW, PT)}
    for z in range(cdiv(HW, PT)):
        p0 = z * PT
        npx = min(PT, HW - p0)
        facts.add("load16" if ((HW | p0 | npx) & 3) == 0 else "load4")
        if HW % 4 == 0 and ((p0 | npx) & 3):
            facts.add("load4 at HW % 4 == 0")
        for c0 in range(0, Cn, 64):
            cw = min(64, Cn - c0)
            facts.add("vector channels" if cw == 64 and Cn % 4 == 0 else "scalar channels, cw < 64" if cw < 64 else "scalar channels, C % 4 != 0")
    return facts


def pool_facts(H, W, bwd):
    """Which kernel a max-pool launch takes and what its bands look like."""
    if bwd and pool_bwd_takes_even(H, W):
        prb = pool_bwd_even_rows(H, W)
        return {"even kernel", "even bands %d" % cdiv(H // 2, prb)} | ({"even short last band"} if (H // 2) % prb else set()) \
            | ({"even PRB below 7 at more than 64 positions"} if (H // 2) * (W // 2) > 64 and prb < 7 else set())
    rb = pool_band(H, W)
    facts = {"generic kernel", "generic bands %d" % min(cdiv(H, rb), 3)}
    if H % rb:
        facts.add("generic short last band")
    if H % 2:
        facts.add("row left over")
    if W % 2:
        facts.add("column left over")
    if bwd and H % 2 == 0 and W % 2 == 0:
        facts.add("even map on the generic kernel")
    return facts


def gather_facts(n_examples, HW, counts):
    facts = {"parts %d" % gather_parts(n_examples, HW)}
    facts |= {"count %d" % k for k in counts}
    if any(k >= 4 for k in counts):
        facts.add("four in flight")
    if any(k >= 4 and k % 4 for k in counts):
        facts.add("tail after four")
    if counts[0] == 0 and counts[-1] == 0 and any(counts):
        facts.add("first and last empty")
    its = gather_items(counts)
    for e in range(n_examples):
        mine = [a for (x, _, a) in its if x == e]
        for k in range(0, len(mine) - 3, 4):
            if any(a < 0 for a in mine[k:k + 4]) and any(a >= 0 for a in mine[k:k + 4]):
                facts.add("NULL and non-NULL attn in one group of four")
    return facts
