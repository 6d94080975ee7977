"""The inputs the prior-sampling tests share (``pnmn_prior_sample``), on the CPU: the GPU tests draw from them, and the CPU test
holds the reference's own share of ambiguous rows on them to half of what the GPU tests excuse."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filtered_inputs as fi  # noqa: E402

PAD, UNK, START, END = fi.PAD, fi.UNK, fi.START, 3
H = 256
IDENTITY = (1.0, 0, 1.0)
# (B, T, V): one row of one step; a partial tile; two tiles, one of them with a single row; the reference configuration's
# length at the largest vocabulary; nine tiles, the last with two rows; one sampled token (V = 4: index 3 alone is allowed)
SHAPES = [(1, 1, 44), (7, 5, 44), (17, 12, 100), (64, 27, 128), (130, 9, 44), (16, 64, 4)]
# weight -> (shape with V, scale), drawn as randn in this order.  The logits z = p W_out^T then spread by about 2.0 to 4.9 per
# row; at a W_out scale of 0.3 the rows are too flat (spread about 1.5) and the reference itself marks 6 % of the (64, 27, 128)
# case under two of the filters.
_WEIGHTS = [("table0", ("V", 4 * H), 1.0), ("w_hh0", (4 * H, H), 0.05), ("w_ih1", (4 * H, H), 0.05), ("w_hh1", (4 * H, H), 0.05),
            ("b1", (4 * H,), 0.5), ("w_proj", (H, H), 0.1), ("w_out", ("V", H), 0.8)]
# the (B, T) of the constrained cases at the real program vocabulary (V = 44); T = None: ``shortest_steps`` of the automaton
CONSTRAINED_SHAPES = [(17, 27), (33, None)]


def shortest_steps(min_left):
    """The fewest steps a constrained launch can have: min_left[0], and at least the one step every launch has (the program
    grammar accepts the empty string, so its min_left[0] is 0)."""
    return max(1, int(min_left[0]))


def prior_weights(B, T, V):
    """{name: fp32 tensor} of one case, row major, from ``torch.Generator().manual_seed(B + T + V)``."""
    g = torch.Generator().manual_seed(B + T + V)
    return {name: torch.randn(*[V if s == "V" else s for s in shape], generator=g) * scale for name, shape, scale in _WEIGHTS}


def prior_filter_cases(V):
    """(filter, seed, row_offset) of every case at vocabulary V: the identity and the first four of ``fi.FILTERS`` everywhere,
    (2.0, 40, 0.8) at V = 44 only (at V = 128 the reference marks 95 of 1728 rows under it, at V = 100 3 of 204); seeds and
    offsets go round the three corners of ``fi.decoder_filter_cases``, the identity on the 2**32 - 5 offset."""
    cases = fi.decoder_filter_cases()
    return [(IDENTITY, *cases[2][1:])] + [c for c in cases if c[0] != fi.FILTERS[4] or V == 44]


def constrained_cases():
    """(filter or None = greedy, seed, row_offset) of every constrained case."""
    cases = fi.decoder_filter_cases()
    return [(IDENTITY, 99, 16), cases[0], cases[2], (None, 0, 0)]


def emulate_prior_logits(w, B, T, choose):
    """The free-running prior in fp64 on the host (the per-step arithmetic stated in include/probnmn_hip.h beside
    pnmn_prior_sample): (z [B * T, V], p [B * T, 256], tokens [B, T]) when step t's token is ``choose(z_t, t)``.  What the
    device computes from the same inputs up to round-off."""
    f = {k: v.double() for k, v in w.items()}
    h0, c0, h1, c1 = (torch.zeros(B, H, dtype=torch.float64) for _ in range(4))
    tok = torch.full((B,), START, dtype=torch.long)

    def cell(gates, c):
        i, fg, g, o = gates.chunk(4, 1)
        c = torch.sigmoid(fg) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c

    zs, ps, toks = [], [], []
    for t in range(T):
        h0, c0 = cell(f["table0"][tok] + h0 @ f["w_hh0"].t(), c0)
        h1, c1 = cell(f["b1"] + h0 @ f["w_ih1"].t() + h1 @ f["w_hh1"].t(), c1)
        p = h1 @ f["w_proj"].t()
        z = p @ f["w_out"].t()
        tok = torch.as_tensor(choose(z.numpy(), t), dtype=torch.long)
        zs.append(z)
        ps.append(p)
        toks.append(tok)
    return torch.stack(zs, 1).reshape(B * T, -1).numpy(), torch.stack(ps, 1).reshape(B * T, -1).numpy(), torch.stack(toks, 1).numpy()


def uniforms(seed, row_offset, B, T):
    """u [B * T] of every (row, step), row major: the kernel's Philox counter (row_offset + row, t)."""
    from filtered_choice import kernel_uniform

    rows = row_offset + np.arange(B, dtype=np.uint64)[:, None]
    return kernel_uniform(seed, rows, np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
