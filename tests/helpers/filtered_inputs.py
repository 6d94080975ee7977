"""The inputs the filtered-sampling tests share: the GPU tests draw from them, and the CPU test holds the reference's own
share of ambiguous rows on them to half of what the GPU tests excuse."""
import numpy as np
import torch

PAD, UNK, START = 0, 1, 2
FILTERS = [(0.7, 5, 1.0), (1.0, 0, 0.9), (1.3, 10, 0.5), (0.25, 0, 0.95), (2.0, 40, 0.8)]
STANDALONE_V = [1, 3, 4, 5, 44, 64, 65, 128, 129, 512]
# (B, seed, step, row_offset): a row offset of 2**32 - 5 puts the batch across the counter's 32-bit word
STANDALONE_CASES = [(1, 0, 0, 0), (5, 2 ** 32 + 7, 39, 2 ** 32 - 5), (5, 2 ** 62 - 1, 2 ** 31, 0), (1000, 0, 39, 2 ** 32 - 5)]
STANDALONE_DELTA, DECODER_DELTA = 1e-5, 1e-4
# Scale of the decoders' output projection W_p (logits = h W_p^T + b_p, |h| < 1 over 256 units).  At 1.0 a row of logits
# spreads by about 3.7 (standard deviation, from the host emulation below): inside the range of scales the standalone
# rows use.  At the 0.3 of the unfiltered decoder tests the rows are nearly flat (spread 1.5) and the reference itself finds
# 5 % of them within 1e-4 of the top-p boundary at V = 128 -- as many as the GPU tests may excuse at all.
DECODER_W_P_SCALE = 1.0
DECODER_SHAPES = [(1, 1, 1, 44), (7, 5, 3, 44), (17, 12, 20, 100), (64, 12, 20, 128), (130, 9, 27, 44)]  # (B, T, S, V)


def standalone_logits(B, V, seed):
    """[B, V] fp32: a different vector in every row, at scales 1 / 2 / 5 / 20 (nearly flat rows, scale 0.1, sit on the top-p
    boundary too often for a test that excuses few rows)."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([1.0, 2.0, 5.0, 20.0])[torch.arange(B) % 4]
    return torch.randn(B, V, generator=g) * scale[:, None]


def standalone_inputs(V):
    """[(logits fp32 [B, V], seed, step, row_offset)] of every standalone case at vocabulary V."""
    return [(standalone_logits(B, V, 100 * V + case), seed, step, row_offset)
            for case, (B, seed, step, row_offset) in enumerate(STANDALONE_CASES)]


H = 256


def decoder_inputs(B, S, V, seed):
    """The tensors of one decoder case, on the CPU (the GPU test moves them to the device as they are)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: torch.randn(*shape, generator=g) * scale  # noqa: E731
    enc, h0 = r(B, S, H), r(B, H)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None, :] < lens[:, None]).float()
    return dict(etable=r(V, 4 * H), enc=enc, mask=mask, h0=h0, w_c=r(4 * H, H, scale=0.05), w_hh=r(4 * H, H, scale=0.05),
                w_p=r(V, H, scale=DECODER_W_P_SCALE), b_p=r(V))


def decoder_filter_cases():
    """(filter, seed, row_offset) of every decoder case: the corner cases of the counter go round the filters."""
    corners = ((2 ** 62 - 1, 0), (2 ** 32 + 7, 16), (12345, 2 ** 32 - 5))
    return [(filt, *corners[i % 3]) for i, filt in enumerate(FILTERS)]


def emulate_decoder_logits(d, T, choose):
    """The free-running decoder in fp64 on the host (the per-step arithmetic stated in include/probnmn_hip.h beside
    pnmn_attn_lstm_fwd): logits [B * T, V] of every (row, step), row major, when step t's token is ``choose(logits_t, t)``.
    What the device computes from the same inputs up to round-off -- the rows the GPU test hands the reference."""
    f = {k: v.double() for k, v in d.items()}
    B = f["enc"].size(0)
    h, c = f["h0"], torch.zeros_like(f["h0"])
    tok = torch.full((B,), START, dtype=torch.long)
    out = []
    for t in range(T):
        scores = torch.einsum("bsh,bh->bs", f["enc"], h)
        p = torch.softmax(scores * f["mask"], 1) * f["mask"]  # (allennlp masked_softmax)
        wgt = p / (p.sum(1, keepdim=True) + 1e-13)
        ctx = torch.einsum("bs,bsh->bh", wgt, f["enc"])
        gates = f["etable"][tok] + ctx @ f["w_c"].t() + h @ f["w_hh"].t()
        i, fg, g, o = gates.chunk(4, 1)
        c = torch.sigmoid(fg) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        logits = h @ f["w_p"].t() + f["b_p"]
        out.append(logits)
        tok = torch.as_tensor(choose(logits.numpy(), t), dtype=torch.long)
    return torch.stack(out, 1).reshape(B * T, -1).numpy()


NO_TABLES = (0, 0, 0, 0, 0, 0)  # (end index, token_class, next_state, min_left, n_states, n_classes): unconstrained


def decoder_entry_calls(jobs, sides, ws, filters, tail=NO_TABLES):
    """Every decoder forward entry on the job records ``jobs`` (``sides[k]``: what ``_prepare_decoder_side`` returned for
    ``jobs[k]``): ``pnmn_attn_lstm_fwd`` on ``jobs[0]`` and, with a workspace ``ws``, ``pnmn_attn_lstm_fwd_group`` with
    n = 1 .. len(jobs).  ``filters``: a ``SAMPLING_FILTER`` array, or None for a null pointer; ``tail``: the automaton
    arguments.  hs, cs and tokens of every job are set to -7 before each call.  Returns [(entry, return code, [copies of
    hs, cs, tokens of each job])], every job listed whether the call covers it or not: one it does not stays at -7."""
    from probnmn import _hip

    lib, stream = _hip.lib(), _hip.stream_ptr(sides[0][0][0].device)
    fptr = 0 if filters is None else filters.ctypes.data
    calls = [("fwd", lambda: lib.pnmn_attn_lstm_fwd(jobs[0:1].ctypes.data, H, fptr, *tail, stream))]
    if ws is not None:
        calls += [("group n=%d" % n, lambda n=n: lib.pnmn_attn_lstm_fwd_group(jobs.ctypes.data, fptr, *tail, n, H, ws.data_ptr(), stream))
                  for n in range(1, len(jobs) + 1)]
    out = []
    for entry, call in calls:
        outputs = [t for sd in sides for t in (sd[0][0], sd[1][1], sd[0][1])]
        for t in outputs:
            t.fill_(-7)
        rc = call()
        torch.cuda.synchronize()
        out.append((entry, rc, [t.clone() for t in outputs]))
    return out


def excused_cap(rows):
    """Rows of a case that may differ from the reference (each still inside the kept set widened by one rank)."""
    return int(np.floor(0.05 * rows)) + 5
