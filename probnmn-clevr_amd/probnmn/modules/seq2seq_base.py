"""``Seq2SeqBase`` -- class surface of the reference's ``probnmn.modules.seq2seq_base`` (reference:
probnmn/modules/seq2seq_base.py:19-375), without AllenNLP.

The reference subclasses ``allennlp.models.encoder_decoders.SimpleSeq2Seq`` (AllenNLP 0.9.0, not
part of this build); the pieces it inherits are restated here from the reference's call sites
and SURVEY.md App. A: token embedder with a zero padding row, a 2-layer LSTM encoder over packed
sequences, dot-product attention with AllenNLP's ``masked_softmax``, an ``LSTMCell`` decoder fed
``cat(attended, embedded)``, a linear output projection.  Parameter names follow the reference's
``state_dict`` so released checkpoints load.

On the MI355X the recurrences are persistent hand-written kernels: one launch per LSTM layer over
the whole padded sequence (``pnmn_lstm_seq_{fwd,bwd}``) and one per decoding loop -- attention,
gates, cell and token choice of every step (``pnmn_attn_lstm_{fwd,bwd}[_multi]``), four or eight
workgroups sharing each 16-row tile (csrc/seq2seq.hip, decoder_multi.hip).  What can be batched over
time (input / output projections, losses, weight gradients) is library GEMMs over all steps; other
hidden sizes fall back to a GEMM per step plus the cell kernel (``pnmn_lstm_cell_{fwd,bwd}``,
``pnmn_sample_tokens``).  Everything that the reference does with per-row Python loops and ``.cpu()``
round trips (sentence boundaries, trimming at ``@end@``) is vectorised on the device: a forward pass
performs no host synchronisation.

Not in the reference: ``decoding_strategy="beam"`` (``Seq2SeqBase.decode_beam``), beam search for inference as one launch
of a persistent kernel that keeps the K hypotheses of a question in one workgroup (``pnmn_attn_lstm_beam``,
csrc/decoder_beam.hip), and ``decoding_strategy="stochastic_beam"`` (``Seq2SeqBase.decode_stochastic_beam``), the same
kernel's stochastic candidate stage: K programs sampled without replacement (``pnmn_attn_lstm_beam_stochastic``).
"""
import math
import os
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from probnmn import _hip
from probnmn.running_metrics import BLEU, Average


class _LSTMCellPointwise(torch.autograd.Function):
    """(gate pre-activations [B,4H], c_prev [B,H]) -> (h, c) on the gfx950 kernel."""

    @staticmethod
    def forward(ctx, gates, c_prev):
        if gates.device.type != "cuda":
            raise _hip.HipLibraryError("LSTM cell on %s: the HIP path needs a ROCm device (no CPU fallback)" % gates.device)
        gates, c_prev = gates.contiguous(), c_prev.contiguous()
        B, H4 = gates.shape
        Hd = H4 // 4
        h = torch.empty_like(c_prev)
        c = torch.empty_like(c_prev)
        act = torch.empty_like(gates)
        _hip.check(_hip.lib().pnmn_lstm_cell_fwd(gates.data_ptr(), c_prev.data_ptr(), h.data_ptr(), c.data_ptr(),
                                                 act.data_ptr(), B, Hd, _hip.stream_ptr(gates.device)), "lstm_cell_fwd")
        ctx.save_for_backward(act, c_prev, c)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        act, c_prev, c = ctx.saved_tensors
        B, H4 = act.shape
        dgates = torch.empty_like(act)
        dc_prev = torch.empty_like(c)
        dh = dh.contiguous() if dh is not None else None  # (kept alive until after the launch)
        dc = dc.contiguous() if dc is not None else None
        dh_p = dh.data_ptr() if dh is not None else None
        dc_p = dc.data_ptr() if dc is not None else None
        _hip.check(_hip.lib().pnmn_lstm_cell_bwd(act.data_ptr(), c_prev.data_ptr(), c.data_ptr(), dh_p, dc_p,
                                                 dgates.data_ptr(), dc_prev.data_ptr(), B, H4 // 4,
                                                 _hip.stream_ptr(act.device)), "lstm_cell_bwd")
        return dgates, dc_prev


def pack_fragments(w: torch.Tensor) -> torch.Tensor:
    """[N][K] row-major -> MFMA-fragment order [N/16][K/16][64][4] (see include/probnmn_hip.h): one wave-wide
    operand load of the persistent LSTM / decoder kernels then reads 1 KiB contiguous."""
    n, k = w.shape
    return w.detach().reshape(n // 16, 16, k // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


def lstm_cell_pointwise(gates, c_prev):
    return _LSTMCellPointwise.apply(gates, c_prev)


def wgrad_gemm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``a.t() @ b`` for tall operands (a [K, M], b [K, N], K = rows x time steps >> M, N).  A weight
    gradient has few output tiles (1024 x 256 -> 32 workgroups on 256 CUs) and a very long reduction;
    splitting K into chunks run as one batched GEMM fills the chip, the partial sums add up after."""
    K = a.size(0)
    if a.size(1) <= 128:
        # few output rows (an output projection's V = 44-100): more, shorter chunks -- the largest count up to 64 that divides
        # K and leaves >= 256 rows per chunk (no remainder GEMM: at 128 questions a call costs ~20 us of host time)
        chunks = max((c for c in range(1, 65) if K % c == 0 and K // c >= 256), default=1)
        if chunks < 4:
            chunks = min(64, K // 512)
    else:
        chunks = min(16, K // 2048)
        if chunks > 1 and K % chunks:  # (a count near it that divides K: no remainder GEMM + addition)
            chunks = max((c for c in range(chunks - 3, 17) if c > 1 and K % c == 0 and K // c >= 1024), default=chunks)
    if chunks <= 1 or not (a.is_contiguous() and b.is_contiguous()):
        return a.t() @ b
    kc = K // chunks
    main = kc * chunks
    out = torch.bmm(a[:main].view(chunks, kc, -1).transpose(1, 2), b[:main].view(chunks, kc, -1)).sum(0)
    if main < K:
        out = out + a[main:].t() @ b[main:]
    return out


class DerivedParams:
    """Per-model cache of what the recurrent kernels read instead of the raw parameters: MFMA-fragment copies
    of W_hh / W_c (and of their transposes, for the backward kernels) and the bias sums b_ih + b_hh.  All of
    them are produced by ONE ``pnmn_derive_params`` launch per model and optimiser step, where the straight-line
    code issued a permute + copy per weight and pass and an add per bias and pass (~25 launches per step).
    The cache is keyed on the parameters' storage, their version counters and ``probnmn.optim.parameter_epoch()``
    (the fused optimiser updates parameters through their pointers, which bumps no version counter).  Anything
    that changes a parameter behind autograd's back the same way -- writes through ``p.data`` or a raw pointer --
    must call ``probnmn.optim.parameters_changed()``; ``load_state_dict``, ``torch.optim`` steps, ``copy_`` /
    in-place ops under ``no_grad`` and ``.to(device)`` are all seen through the version counters / storage."""

    def __init__(self):
        self._key = None
        self._where = None
        self._out: Dict[str, torch.Tensor] = {}

    def get(self, params, make_specs) -> Dict[str, torch.Tensor]:
        """``params``: the parameters everything is derived from (the cache key is their storage, version
        counters and the fused optimiser's step count -- a dozen attribute reads per call);
        ``make_specs()``: list of (name, kind, a, b) -- kind "pack" (fragment order of the [N][K] matrix ``a``),
        "packT" (of its transpose), "sum" (a + b) -- built only when the cache misses."""
        from probnmn.optim import parameter_epoch

        flat = [parameter_epoch()]
        for p in params:
            flat.append(p._version)
            flat.append(p.data_ptr())
        key = tuple(flat)
        if key == self._key:
            return self._out
        where = key[2::2]
        if where == self._where:
            # same storage, new values (every optimiser step): the job list still describes the work -- run it
            # again into the same buffer (launches on this stream that read the old copies are ordered before it)
            _hip.check(_hip.lib().pnmn_derive_params(self._jobs.data_ptr(), self._n_jobs, self._max_quads,
                                                     _hip.stream_ptr(self._device)), "derive_params")
            self._key = key
            return self._out
        specs = make_specs()
        dev = specs[0][2].device
        import numpy as np

        total = sum(a.numel() for _, _, a, _ in specs)
        buf = torch.empty(total, dtype=torch.float32, device=dev)
        rec = np.zeros(len(specs), _hip.DERIVE_JOB)
        out, off, max_quads = {}, 0, 0
        for i, (name, kind, a, b) in enumerate(specs):
            dst = buf[off:off + a.numel()]
            rec[i]["src"], rec[i]["dst"] = a.data_ptr(), dst.data_ptr()
            if kind == "sum":
                if not (a.is_contiguous() and b.is_contiguous()):
                    raise _hip.HipLibraryError("bias vectors must be contiguous")
                rec[i]["src2"], rec[i]["n"], rec[i]["kind"] = b.data_ptr(), a.numel(), 2
                out[name] = dst
            else:
                n, k = a.shape
                if a.stride(1) != 1 or n % 16 or k % 16:
                    raise _hip.HipLibraryError("recurrent weight of shape %s / strides %s" % (tuple(a.shape), a.stride()))
                if kind == "pack":
                    rec[i]["n"], rec[i]["k"], rec[i]["kind"] = n, k, 0
                else:  # fragment order of a.t(): logical [k][n]
                    rec[i]["n"], rec[i]["k"], rec[i]["kind"] = k, n, 1
                rec[i]["ld"] = a.stride(0)
                out[name] = dst
            max_quads = max(max_quads, a.numel() // 4)
            off += a.numel()
        jobs = _hip.to_device(rec, dev)
        _hip.check(_hip.lib().pnmn_derive_params(jobs.data_ptr(), len(specs), max_quads, _hip.stream_ptr(dev)), "derive_params")
        self._key, self._out, self._jobs = key, out, jobs
        self._where, self._n_jobs, self._max_quads, self._device, self._buf = where, len(specs), max_quads, dev, buf
        return out


class _Alias(torch.autograd.Function):
    """``value`` (computed elsewhere from ``a`` and ``b`` as a + b) enters the graph as if it were ``a + b``."""

    @staticmethod
    def forward(ctx, a, b, value):
        return value.view_as(value)

    @staticmethod
    def backward(ctx, g):
        return g, g, None


class _SplitRows(torch.autograd.Function):
    """``(x[:n], x[n:])`` as views whose backward is ONE concatenation (a missing side: zeros).  For an encoder state that
    two decodes share (``Seq2SeqBase.split_rows``): gathering the two row sets with ``index_select`` costs a copy per tensor
    and set forward, and a zero-filled full-size gradient, an ``index_add_`` and an addition each backward."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.rest = n, x.size(0) - n
        ctx.tail, ctx.kind = tuple(x.shape[1:]), (x.dtype, x.device)
        return x.narrow(0, 0, n), x.narrow(0, n, x.size(0) - n)

    @staticmethod
    def backward(ctx, da, db):
        dtype, device = ctx.kind
        if da is None:
            da = torch.zeros((ctx.n,) + ctx.tail, dtype=dtype, device=device)
        if db is None:
            db = torch.zeros((ctx.rest,) + ctx.tail, dtype=dtype, device=device)
        return torch.cat((da, db), 0), None


class _SplitColumns(torch.autograd.Function):
    """``(w[:, :k], w[:, k:])`` whose backward is ONE concatenation: two slices of a parameter otherwise cost two
    zero-filled full-size gradients, two copies into them and an addition per use."""

    @staticmethod
    def forward(ctx, w, k):
        ctx.k, ctx.n = k, w.size(1)
        return w[:, :k], w[:, k:]

    @staticmethod
    def backward(ctx, da, db):
        if da is None and db is None:
            return None, None
        ref = da if da is not None else db
        if da is None:
            da = ref.new_zeros(ref.size(0), ctx.k)
        if db is None:
            db = ref.new_zeros(ref.size(0), ctx.n - ctx.k)
        return torch.cat((da, db), 1), None


class _TokenTable(torch.autograd.Function):
    """``F.linear(embedding.weight, weight, bias)`` ([V, 4H]) where the embedding's padding row receives no
    gradient (nn.Embedding(padding_idx=...) never updates it; its value is zero, so the table row is the bias).
    One launch each way for the vocabularies here (``pnmn_token_table_fwd`` / ``_bwd``); library GEMMs otherwise."""

    @staticmethod
    def _fused(emb, weight):
        return (emb.device.type == "cuda" and emb.size(0) <= 128 and emb.size(1) % 16 == 0 and weight.size(0) % 64 == 0
                and emb.is_contiguous() and weight.stride(1) == 1 and weight.stride(0) % 4 == 0)

    @staticmethod
    def forward(ctx, emb, weight, bias, padding_idx):
        ctx.save_for_backward(emb, weight)
        ctx.padding_idx = padding_idx
        emb_d, weight_d = emb.detach(), weight.detach()
        if not _TokenTable._fused(emb_d, weight_d) or not bias.is_contiguous():
            return torch.addmm(bias, emb_d, weight_d.t())
        V, K = emb_d.shape
        N = weight_d.size(0)
        table = torch.empty(V, N, dtype=emb_d.dtype, device=emb_d.device)
        _hip.check(_hip.lib().pnmn_token_table_fwd(emb_d.data_ptr(), weight_d.data_ptr(), weight_d.stride(0), bias.data_ptr(),
                                                   V, K, N, table.data_ptr(), _hip.stream_ptr(emb_d.device)), "token_table_fwd")
        return table

    @staticmethod
    def backward(ctx, dtable):
        emb, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        if _TokenTable._fused(emb, weight):
            dtable = dtable.contiguous()
            V, K = emb.shape
            N = weight.size(0)
            f = dict(dtype=emb.dtype, device=emb.device)
            demb = torch.empty(V, K, **f) if need[0] else None
            dweight = torch.empty(N, K, **f) if need[1] else None
            dbias = torch.empty(N, **f) if need[2] else None
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            _hip.check(_hip.lib().pnmn_token_table_bwd(dtable.data_ptr(), emb.data_ptr(), weight.data_ptr(), weight.stride(0),
                                                       V, K, N, -1 if ctx.padding_idx is None else ctx.padding_idx,
                                                       ptr(demb), ptr(dweight), 0, ptr(dbias), None, _hip.stream_ptr(emb.device)),
                       "token_table_bwd")
            return demb, dweight, dbias, None
        demb = dweight = dbias = None
        if need[0]:
            demb = dtable @ weight
            if ctx.padding_idx is not None:
                demb[ctx.padding_idx].zero_()
        if need[1]:
            dweight = dtable.t() @ emb
        if need[2]:
            dbias = dtable.sum(0)
        return demb, dweight, dbias, None


class _TokenPrep(object):
    """``pnmn_token_prep`` (see include/probnmn_hip.h): sentence boundaries, mask and last-token index of a
    right-padded token matrix in one launch."""

    @staticmethod
    def run(tokens: torch.Tensor, pad: int, bos: int, eos: int, drop_first: bool, want_mask: bool):
        if tokens.device.type != "cuda":
            raise _hip.HipLibraryError("token input on %s: the HIP path needs a ROCm device" % tokens.device)
        if tokens.dtype != torch.long:
            tokens = tokens.long()
        if tokens.stride(1) != 1:
            tokens = tokens.contiguous()
        B, T = tokens.shape
        W = T + 2 - int(drop_first)
        out = torch.empty(B, W, dtype=torch.long, device=tokens.device)
        fmask = torch.empty(B, W, dtype=torch.float32, device=tokens.device) if want_mask else None
        last = torch.empty(B, dtype=torch.int32, device=tokens.device) if want_mask else None
        _hip.check(_hip.lib().pnmn_token_prep(tokens.data_ptr(), tokens.stride(0), B, T, pad, bos, eos, int(drop_first),
                                              out.data_ptr(), fmask.data_ptr() if want_mask else None,
                                              last.data_ptr() if want_mask else None, _hip.stream_ptr(tokens.device)),
                   "token_prep")
        return out, fmask, last


class _MaskAndLast(torch.autograd.Function):
    """(hs [B,T,H], fmask [B,T], last [B]) -> (hs * fmask[..., None], its row ``last[b]`` per example): the
    zeroed padded steps of ``PytorchSeq2SeqWrapper`` and ``get_final_encoder_states`` in one launch each way."""

    @staticmethod
    def forward(ctx, hs, fmask, last):
        hs = hs.contiguous()
        B, T, H = hs.shape
        enc = torch.empty_like(hs)
        hlast = torch.empty(B, H, dtype=hs.dtype, device=hs.device)
        _hip.check(_hip.lib().pnmn_mask_last_fwd(hs.data_ptr(), fmask.data_ptr(), last.data_ptr(), B, T, H, enc.data_ptr(),
                                                 hlast.data_ptr(), _hip.stream_ptr(hs.device)), "mask_last_fwd")
        ctx.save_for_backward(fmask, last)
        ctx.shape = (B, T, H)
        return enc, hlast

    @staticmethod
    def backward(ctx, denc, dhlast):
        fmask, last = ctx.saved_tensors
        B, T, H = ctx.shape
        denc = denc.contiguous() if denc is not None else None
        dhlast = dhlast.contiguous() if dhlast is not None else None
        dhs = torch.empty(B, T, H, dtype=fmask.dtype, device=fmask.device)
        _hip.check(_hip.lib().pnmn_mask_last_bwd(denc.data_ptr() if denc is not None else None,
                                                 dhlast.data_ptr() if dhlast is not None else None, fmask.data_ptr(),
                                                 last.data_ptr(), B, T, H, dhs.data_ptr(), _hip.stream_ptr(fmask.device)),
                   "mask_last_bwd")
        return dhs, None, None


def embedding_grad(dy: torch.Tensor, tokens: torch.Tensor, vocab: int, shift: bool = False, start: int = 0,
                   skip: int = -1) -> torch.Tensor:
    """dW[v] = sum of the rows of ``dy`` ([B, T, C]) whose token is v (``pnmn_embedding_grad``)."""
    B, T = tokens.shape
    C = dy.size(-1)
    dy = dy.contiguous()
    if tokens.stride(1) != 1:
        tokens = tokens.contiguous()
    dw = torch.empty(vocab, C, dtype=dy.dtype, device=dy.device)
    ws = torch.empty(int(_hip.lib().pnmn_embedding_grad_workspace_bytes(B, T, vocab)), dtype=torch.uint8, device=dy.device)
    _hip.check(_hip.lib().pnmn_embedding_grad(dy.data_ptr(), tokens.data_ptr(), tokens.stride(0), B, T, C, vocab, int(shift),
                                              start, skip, 0, dw.data_ptr(), ws.data_ptr(), _hip.stream_ptr(dy.device)),
               "embedding_grad")
    return dw


class _LinearRows(torch.autograd.Function):
    """``F.linear`` over B x T rows whose weight gradient goes through ``wgrad_gemm`` (autograd's
    plain ``dy.t() @ x`` has 32 output tiles and a 47 000-long reduction at these shapes)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.size(-1))
        dx = (dy2 @ weight).view_as(x) if ctx.needs_input_grad[0] else None
        dw = wgrad_gemm(dy2.contiguous(), x.reshape(-1, x.size(-1)).contiguous()) if ctx.needs_input_grad[1] else None
        db = dy2.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db


def linear_rows(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    if x.device.type != "cuda" or not torch.is_grad_enabled():
        return F.linear(x, weight, bias)
    return _LinearRows.apply(x, weight, bias)


class _EmbeddingLookup(torch.autograd.Function):
    """``F.embedding`` whose weight gradient is one kernel: the vocabularies here have < 100 entries, so the
    scatter-add of B x T rows into them that torch's backward does (sort + segmented reduction, ~0.4 ms per
    call) is ``pnmn_embedding_grad`` (rows bucketed by token, summed chunk by chunk; larger vocabularies: a
    one-hot GEMM)."""

    @staticmethod
    def forward(ctx, weight, tokens, padding_idx):
        ctx.save_for_backward(tokens)
        ctx.vocab, ctx.padding_idx = weight.size(0), padding_idx
        return F.embedding(tokens, weight)

    @staticmethod
    def backward(ctx, dy):
        (tokens,) = ctx.saved_tensors
        return _table_grad(dy, tokens, ctx.vocab, ctx.padding_idx), None, None


def embedding_lookup(module: nn.Embedding, tokens: torch.Tensor) -> torch.Tensor:
    if tokens.device.type != "cuda" or not torch.is_grad_enabled() or not module.weight.requires_grad:
        return module(tokens)
    return _EmbeddingLookup.apply(module.weight, tokens, module.padding_idx)


def _lstm_workspace(batch: int, backward: bool, device) -> Optional[torch.Tensor]:
    """Scratch for the multi-CU LSTM kernels (step counters + the backward's exchange buffer); ``None``
    when the library keeps one workgroup per row tile (batch large enough to fill the chip, or
    PNMN_LSTM_CLUSTER=0).  A fresh allocation per launch: the caching allocator orders its reuse on
    the launch stream."""
    if os.environ.get("PNMN_LSTM_CLUSTER", "1") == "0":
        return None
    n = int(_hip.lib().pnmn_lstm_seq_workspace_bytes(batch, 1 if backward else 0))
    return torch.empty(n, dtype=torch.uint8, device=device) if n > 0 else None


def _decoder_workspace_bytes(rows, backward: bool) -> int:
    """Bytes of scratch the multi-CU decoder kernels want for passes of ``rows[i]`` rows each in one call (the library's fit /
    fall-back rule: include/probnmn_hip.h); 0 = a single pass runs on the one-workgroup-per-tile kernels
    (PNMN_DECODER_CLUSTER=0, or a device too small for eight resident workgroups per tile)."""
    if len(rows) == 1 and os.environ.get("PNMN_DECODER_CLUSTER", "1") == "0":
        return 0
    return _hip.decoder_workspace_bytes(rows, backward)


def _decoder_workspace(rows, backward: bool, device) -> Optional[torch.Tensor]:
    """That scratch, or ``None`` for 0 bytes.  A fresh allocation per launch, as ``_lstm_workspace``."""
    n = _decoder_workspace_bytes(rows, backward)
    return torch.empty(n, dtype=torch.uint8, device=device) if n > 0 else None


def lstm_length_order_enabled() -> bool:
    """PNMN_LSTM_LENGTH_ORDER=0: the layer kernels run every row over all T steps (the unordered entry points), for A/B
    runs; by default rows with a known length are grouped by it and a tile stops at its longest row."""
    return os.environ.get("PNMN_LSTM_LENGTH_ORDER", "1") != "0"


def length_order(last: torch.Tensor, T: int):
    """``pnmn_length_order``: (order [B], tile_steps [ceil(B/16)]), both int32, of the rows whose last valid step is
    ``last`` ([B] int32, as ``pnmn_token_prep`` writes it) in a pass of ``T`` steps; no host synchronisation."""
    B = last.size(0)
    order = torch.empty(B, dtype=torch.int32, device=last.device)
    tile_steps = torch.empty((B + 15) // 16, dtype=torch.int32, device=last.device)
    _hip.check(_hip.lib().pnmn_length_order(last.data_ptr(), B, T, order.data_ptr(), tile_steps.data_ptr(),
                                            _hip.stream_ptr(last.device)), "length_order")
    return order, tile_steps


class _LSTMLayerSeq(torch.autograd.Function):
    """The recurrent half of one LSTM layer over a whole padded sequence, as ONE persistent kernel
    launch (``pnmn_lstm_seq_fwd`` / ``_bwd``): (xp [B,T,4H] = input projection + biases, W_hh) -> all
    hidden states [B,T,H].  The weight gradient of W_hh is one GEMM over the saved states.
    With ``tokens`` ([B,T] int64): ``xp`` is the [V,4H] per-token table of ``_TokenTable`` and the kernel reads
    row ``tokens[b,t]`` of it -- ``F.embedding(tokens, table)`` is never written out; its gradient is the
    per-token sum of ``pnmn_embedding_grad`` over the gate gradients.
    With ``order`` / ``tile_steps`` (``length_order``): the ``_ordered`` entry points -- row tiles grouped by length, each
    run to its longest row; the output is zero from there on, and the caller's gradient must be zero past each row's
    length (what ``_MaskAndLast`` gives)."""

    @staticmethod
    def forward(ctx, xp, w_hh, wp=None, w_t=None, tokens=None, order=None, tile_steps=None):
        if xp.device.type != "cuda":
            raise _hip.HipLibraryError("LSTM layer on %s: the HIP path needs a ROCm device (no CPU fallback)" % xp.device)
        xp, w = xp.contiguous(), w_hh.detach()
        if tokens is not None:
            if tokens.dtype != torch.long or tokens.stride(1) != 1:
                tokens = tokens.long().contiguous()
            (B, T), H4 = tokens.shape, xp.size(1)
        else:
            B, T, H4 = xp.shape
        Hd = H4 // 4
        hs = torch.empty(B, T, Hd, dtype=xp.dtype, device=xp.device)
        cs = torch.empty_like(hs)
        act = torch.empty(B, T, H4, dtype=xp.dtype, device=xp.device)
        if wp is None:
            wp = pack_fragments(w)
        ctx.w_t = w_t  # (fragment order of W_hh^T from the model's DerivedParams, else packed in backward)
        ctx.tokens, ctx.vocab = tokens, xp.size(0)
        ctx.order = (order, tile_steps) if order is not None else None
        ws = _lstm_workspace(B, False, xp.device)
        args = (xp.data_ptr(), tokens.data_ptr() if tokens is not None else None, tokens.stride(0) if tokens is not None else 0,
                wp.data_ptr(), hs.data_ptr(), cs.data_ptr(), act.data_ptr(), B, T, Hd)
        tail = (ws.data_ptr() if ws is not None else None, _hip.stream_ptr(xp.device))
        if order is not None:
            _hip.check(_hip.lib().pnmn_lstm_seq_fwd_ordered(*args, order.data_ptr(), tile_steps.data_ptr(), *tail),
                       "lstm_seq_fwd_ordered")
        else:
            _hip.check(_hip.lib().pnmn_lstm_seq_fwd(*args, *tail), "lstm_seq_fwd")
        ctx.save_for_backward(hs, cs, act, w)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        hs, cs, act, w = ctx.saved_tensors
        B, T, Hd = hs.shape
        dhs = dhs.contiguous()
        w_t = ctx.w_t if ctx.w_t is not None else pack_fragments(w.t())  # W_hh^T [H][4H], fragment order
        dgates = torch.empty_like(act)
        ws = _lstm_workspace(B, True, hs.device)
        args = (dhs.data_ptr(), act.data_ptr(), cs.data_ptr(), w_t.data_ptr(), dgates.data_ptr(), B, T, Hd)
        tail = (ws.data_ptr() if ws is not None else None, _hip.stream_ptr(hs.device))
        if ctx.order is not None:
            _hip.check(_hip.lib().pnmn_lstm_seq_bwd_ordered(*args, ctx.order[0].data_ptr(), ctx.order[1].data_ptr(), *tail),
                       "lstm_seq_bwd_ordered")
        else:
            _hip.check(_hip.lib().pnmn_lstm_seq_bwd(*args, *tail), "lstm_seq_bwd")
        dw_hh = None
        if ctx.needs_input_grad[1]:
            hprev = torch.cat((hs.new_zeros(B, 1, Hd), hs[:, :-1]), 1).reshape(B * T, Hd)  # h_{t-1} per (row, step)
            dw_hh = wgrad_gemm(dgates.reshape(B * T, 4 * Hd), hprev)
        dxp = dgates
        if ctx.tokens is not None:
            dxp = _table_grad(dgates, ctx.tokens, ctx.vocab) if ctx.needs_input_grad[0] else None
        return dxp, dw_hh, None, None, None, None, None


class _LSTMDropout(torch.autograd.Function):
    """``nn.LSTM(dropout=p)``'s mask between two layers, in training mode (``pnmn_lstm_dropout``): y = x * keep * scale over
    [B,T,H] with keep(row, t, u) drawn from Philox under ``seed`` (row = ``row_offset`` + the row's index; the stream is
    documented beside the entry point in include/probnmn_hip.h).  Backward regenerates the same mask on the gradient."""

    @staticmethod
    def forward(ctx, x, p, seed, row_offset):
        x = x.contiguous()
        B, T, Hd = x.shape
        y = torch.empty_like(x)
        _hip.check(_hip.lib().pnmn_lstm_dropout(x.data_ptr(), y.data_ptr(), B, T, Hd, p, seed, row_offset, _hip.stream_ptr(x.device)),
                   "lstm_dropout")
        ctx.args = (p, seed, row_offset)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, row_offset = ctx.args
        dy = dy.contiguous()
        B, T, Hd = dy.shape
        dx = torch.empty_like(dy)
        _hip.check(_hip.lib().pnmn_lstm_dropout(dy.data_ptr(), dx.data_ptr(), B, T, Hd, p, seed, row_offset, _hip.stream_ptr(dy.device)),
                   "lstm_dropout backward")
        return dx, None, None, None


def lstm_dropout_seed(lstm: nn.LSTM) -> Optional[int]:
    """The seed of one encoder pass's dropout masks: drawn from torch's CPU generator (as ``decode`` draws its sampler
    seeds) only when the pass drops anything -- training mode and p > 0; None otherwise, drawing nothing."""
    if lstm.training and lstm.dropout > 0 and lstm.num_layers > 1:
        return int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
    return None


def _table_grad(dy: torch.Tensor, tokens: torch.Tensor, vocab: int, padding_idx: Optional[int] = None) -> torch.Tensor:
    """Gradient of ``F.embedding(tokens, table)`` wrt the table, from the gradient ``dy`` [B,T,C] of its output."""
    if vocab <= 128 and dy.size(-1) % 64 == 0 and tokens.dim() == 2:
        return embedding_grad(dy, tokens, vocab, skip=padding_idx if padding_idx is not None else -1)
    flat = tokens.reshape(-1)
    onehot = torch.zeros(flat.numel(), vocab, dtype=dy.dtype, device=dy.device)
    onehot.scatter_(1, flat.unsqueeze(1), 1.0)
    dw = wgrad_gemm(onehot, dy.reshape(flat.numel(), -1).contiguous())
    if padding_idx is not None:
        dw[padding_idx].zero_()
    return dw


_SIDE_SAVED = 11  # tensors a decoder pass saves: hs, cs, act, cx, probs, enc, mask, h0, w_c, w_hh, step tokens


class _DecoderLaunch(NamedTuple):
    """What the forward launch of some decoder passes leaves behind.  Per pass: two ``outs`` (hidden states [B,T,H] and the
    chosen tokens [B,T], empty when teacher forced), ``_SIDE_SAVED`` tensors in ``saved`` and one entry of ``side_meta``
    (vocab, (W_c^T, W_hh^T) in fragment order or None, mode, start index, fed projected inputs?)."""

    outs: tuple
    saved: tuple
    side_meta: tuple


def _prepare_decoder_side(jobs, k, source, enc, mask, h0, w_c, w_hh, m):
    """Everything one decoder pass needs before its launch; fills row ``k`` of ``jobs`` (``DECODER_FWD_JOB``).
    Tensor inputs: ``source``, enc [B,S,H], mask [B,S] float, h0 [B,H], W_c [4H,H], W_hh [4H,H]; ``m`` carries the rest:
    ``mode`` 0 teacher forced -- ``source`` is the per-token table [V,4H] and step t's input its row ``in_tokens[b,t]``, or
    (no ``in_tokens``) ``source`` is the projected inputs xe [B,T,4H] themselves; 1 sampling / 2 greedy: free running, the
    kernel picks each step's token (``source`` = the projected embedding table; ``w_p`` [V,H], ``b_p``, ``pad``, ``unk``,
    ``seed``, ``row_offset``); ``T``, ``start``, ``packs`` = (W_c, W_hh, W_c^T, W_hh^T) in fragment order from the model's
    DerivedParams, or None.  Returns (outs, saved, side meta) as ``_DecoderLaunch`` lists them, and the tensors that must
    outlive the launch call."""
    dev = enc.device
    if dev.type != "cuda":
        raise _hip.HipLibraryError("decoder on %s: the HIP path needs a ROCm device (no CPU fallback)" % dev)
    source, enc, mask, h0 = source.contiguous(), enc.contiguous(), mask.contiguous(), h0.contiguous()
    w_c, w_hh = w_c.detach(), w_hh.detach()
    packs = m.get("packs")
    if packs is None:
        packs = (pack_fragments(w_c), pack_fragments(w_hh), None, None)
    mode, T = m["mode"], m["T"]
    B, S, Hd = enc.shape
    f = dict(dtype=torch.float32, device=dev)
    hs, cs, cx = torch.empty(B, T, Hd, **f), torch.empty(B, T, Hd, **f), torch.empty(B, T, Hd, **f)
    act, probs = torch.empty(B, T, 4 * Hd, **f), torch.empty(B, T, S, **f)
    in_tokens = tokens = w_p = b_p = None
    projected = mode == 0 and m.get("in_tokens") is None
    if mode != 0:
        w_p, b_p = m["w_p"].detach().contiguous(), m["b_p"].detach().contiguous()
        tokens = torch.empty(B, T, dtype=torch.long, device=dev)
    elif not projected:
        in_tokens = m["in_tokens"]
        if in_tokens.dtype != torch.long or in_tokens.stride(1) != 1:
            in_tokens = in_tokens.long().contiguous()
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    jobs[k] = (source.data_ptr() if projected else 0, 0 if projected else source.data_ptr(), enc.data_ptr(), mask.data_ptr(),
               h0.data_ptr(), packs[0].data_ptr(), packs[1].data_ptr(), ptr(w_p), ptr(b_p), hs.data_ptr(), cs.data_ptr(),
               act.data_ptr(), cx.data_ptr(), probs.data_ptr(), ptr(tokens), ptr(in_tokens),
               0 if in_tokens is None else in_tokens.stride(0), m.get("seed", 0), m.get("row_offset", 0), B, T, S,
               0 if w_p is None else w_p.size(0), mode, m.get("pad", 0), m.get("unk", 0), m["start"])
    empty = torch.empty(0, dtype=torch.long, device=dev)
    step_tokens = tokens if mode != 0 else in_tokens
    saved = (hs, cs, act, cx, probs, enc, mask, h0, w_c, w_hh, step_tokens if step_tokens is not None else hs.new_empty(0))
    side_meta = (0 if projected else source.size(0), (packs[2], packs[3]) if packs[2] is not None else None, mode, m["start"],
                 projected)
    return (hs, tokens if tokens is not None else empty), saved, side_meta, (source, packs, w_p, b_p)


def _decoder_forward(tensors, metas) -> _DecoderLaunch:
    """The forward of one or two decoder passes as ONE launch (``pnmn_attn_lstm_fwd_group``: side by side when they fit the
    chip together, else one after the other -- bit for bit the same either way, the kernels' bodies are shared).
    ``tensors[k]`` / ``metas[k]``: pass k's inputs as ``_prepare_decoder_side`` takes them.  A single pass without the
    multi-CU kernels (``_decoder_workspace``) runs on ``pnmn_attn_lstm_fwd``."""
    n = len(metas)
    jobs = np.zeros(n, _hip.DECODER_FWD_JOB)
    sides = [_prepare_decoder_side(jobs, k, *tensors[k], metas[k]) for k in range(n)]  # (alive until the launch is queued)
    hs = sides[0][0][0]
    dev, Hd = hs.device, hs.size(2)
    ws = _decoder_workspace([sd[0][0].size(0) for sd in sides], False, dev)
    lib = _hip.lib()
    # ``meta["filter"]``: the pass's sampling filter (``sampling_filter``), honoured when it samples; with none anywhere the
    # library gets a null ``filters``
    filters = None
    if any(m.get("filter") is not None for m in metas):
        filters = np.zeros(n, _hip.SAMPLING_FILTER)
        for k, m in enumerate(metas):
            filters[k] = (*(m.get("filter") or IDENTITY_FILTER), 0)
    # ``meta["constraint"]``: (token_class, next_state, min_left, end index) of a free-running pass that decodes under a token
    # automaton (``constraint_tables``).  The library applies ONE automaton to every free-running pass of the launch, so
    # passes side by side name the same one, or none
    constraint = None
    for m in metas:
        c = m.get("constraint")
        if c is not None and m["mode"] == 0:
            raise ValueError("a teacher-forced decoder pass takes no constraint")
        if c is not None and constraint is not None and c is not constraint:
            raise ValueError("decoder passes side by side decode under one token automaton")
        constraint = c if c is not None else constraint
    automaton = (0, 0, 0, 0, 0, 0)  # (end index, three tables, n_states, n_classes): null tables = unconstrained
    if constraint is not None:
        if any(m["mode"] != 0 and m.get("constraint") is None for m in metas):
            raise ValueError("a constrained and an unconstrained free-running pass cannot share a launch")
        tc, ns, ml, end = constraint  # (host arrays: the library checks every entry and passes them by value)
        automaton = (end, tc.ctypes.data, ns.ctypes.data, ml.ctypes.data, ns.shape[0], ns.shape[1])
    options = (0 if filters is None else filters.ctypes.data, *automaton)
    if ws is not None:
        _hip.check(lib.pnmn_attn_lstm_fwd_group(jobs.ctypes.data, *options, n, Hd, ws.data_ptr(), _hip.stream_ptr(dev)),
                   "attn_lstm_fwd_group")
    elif n == 1:
        _hip.check(lib.pnmn_attn_lstm_fwd(jobs.ctypes.data, Hd, *options, _hip.stream_ptr(dev)), "attn_lstm_fwd")
    else:
        raise _hip.HipLibraryError("decoder passes side by side need the multi-CU decoder kernels (none on this device)")
    return _DecoderLaunch(tuple(t for sd in sides for t in sd[0]), tuple(t for sd in sides for t in sd[1]),
                          tuple(sd[2] for sd in sides))


def _decoder_sides_backward(saved, side_meta, dhs_list, needs_input_grad):
    """Backward of 1-3 decoder passes whose forward saved ``_SIDE_SAVED`` tensors each (``_DecoderLaunch``): ONE launch for
    all of them (``pnmn_attn_lstm_bwd_group``), then per pass the encoder-output gradient, the two weight-gradient GEMMs
    and the gradient of what fed the steps (the table, or the projected inputs).  Returns six gradients per pass, in the
    order of ``_prepare_decoder_side``'s tensor inputs (source, enc, mask, h0, w_c, w_hh); ``needs_input_grad`` likewise.
    A single pass without the multi-CU kernels runs on ``pnmn_attn_lstm_bwd``, which accumulates ``denc`` itself."""
    dev = saved[0].device
    n = len(dhs_list)
    lib, Hd = _hip.lib(), saved[0].size(2)
    ws = _decoder_workspace([saved[_SIDE_SAVED * k].size(0) for k in range(n)], True, dev)
    if ws is None and n > 1:
        raise _hip.HipLibraryError("decoder passes side by side need the multi-CU decoder kernels (none on this device)")
    jobs = np.zeros(n, _hip.DECODER_BWD_JOB)
    sides = []
    for k, dhs in enumerate(dhs_list):
        hs, cs, act, cx, probs, enc, mask, h0, w_c, w_hh, step_tokens = saved[_SIDE_SAVED * k: _SIDE_SAVED * (k + 1)]
        packs_t = side_meta[k][1]
        B, T, S = hs.size(0), hs.size(1), enc.size(1)
        # (named temporaries: a tensor that dies right after .data_ptr() may be recycled by the next allocation)
        dhs_c = torch.zeros_like(hs) if dhs is None else dhs.contiguous()
        w_c_t, w_hh_t = packs_t if packs_t is not None else (pack_fragments(w_c.t()), pack_fragments(w_hh.t()))
        dgates, dh0 = torch.empty_like(act), torch.empty_like(h0)
        if ws is not None:
            dctx, dscore, weights, denc = torch.empty_like(hs), torch.empty_like(probs), torch.empty_like(probs), None
            jobs[k] = (dhs_c.data_ptr(), act.data_ptr(), cs.data_ptr(), hs.data_ptr(), probs.data_ptr(), enc.data_ptr(),
                       mask.data_ptr(), h0.data_ptr(), w_c_t.data_ptr(), w_hh_t.data_ptr(), dgates.data_ptr(), dctx.data_ptr(),
                       dscore.data_ptr(), weights.data_ptr(), dh0.data_ptr(), B, T, S, 0)
        else:
            dctx = dscore = weights = None
            denc = torch.zeros_like(enc)
            _hip.check(lib.pnmn_attn_lstm_bwd(
                dhs_c.data_ptr(), act.data_ptr(), cs.data_ptr(), hs.data_ptr(), cx.data_ptr(), probs.data_ptr(),
                enc.data_ptr(), mask.data_ptr(), h0.data_ptr(), w_c_t.data_ptr(), w_hh_t.data_ptr(), dgates.data_ptr(),
                denc.data_ptr(), dh0.data_ptr(), B, T, S, Hd, _hip.stream_ptr(dev)), "attn_lstm_bwd")
        sides.append(dict(hs=hs, cx=cx, enc=enc, h0=h0, step_tokens=step_tokens, dgates=dgates, dh0=dh0, dctx=dctx, dscore=dscore,
                          weights=weights, denc=denc, keep=(dhs_c, w_c_t, w_hh_t), B=B, T=T, S=S))
    if ws is not None:
        _hip.check(lib.pnmn_attn_lstm_bwd_group(jobs.ctypes.data, n, Hd, ws.data_ptr(), _hip.stream_ptr(dev)), "attn_lstm_bwd_group")
    grads = []
    for k, sd in enumerate(sides):
        B, T, S = sd["B"], sd["T"], sd["S"]
        vocab, _, mode, start, projected = side_meta[k]
        need = needs_input_grad[6 * k: 6 * k + 6]
        hprev = None
        if need[5] or (need[1] and sd["denc"] is None and T > 64):
            hprev = torch.cat((sd["h0"].unsqueeze(1), sd["hs"][:, :-1]), 1)  # h_{t-1} of every (row, step)
        denc = sd["denc"] if need[1] else None
        if need[1] and denc is None:
            # encoder-output gradient as two GEMMs per row over the T steps: enc_s enters step t through
            # the context (weight w_ts = masked, renormalised attention, written out by the kernel) and through the
            # score (gradient dscore_ts, times h_{t-1})
            if T <= 64:
                denc = torch.empty_like(sd["enc"])
                _hip.check(lib.pnmn_attn_denc(sd["weights"].data_ptr(), sd["dscore"].data_ptr(), sd["dctx"].data_ptr(),
                                              sd["hs"].data_ptr(), sd["h0"].data_ptr(), denc.data_ptr(), B, T, S, Hd,
                                              _hip.stream_ptr(dev)), "attn_denc")
            else:
                denc = torch.baddbmm(torch.bmm(sd["weights"].transpose(1, 2), sd["dctx"]), sd["dscore"].transpose(1, 2), hprev)
        flat = sd["dgates"].reshape(B * T, 4 * Hd)
        dw_c = wgrad_gemm(flat, sd["cx"].reshape(B * T, Hd)) if need[4] else None
        dw_hh = wgrad_gemm(flat, hprev.reshape(B * T, Hd)) if need[5] else None
        dsource = None
        if need[0]:
            if projected:
                dsource = sd["dgates"]
            elif mode == 0:
                dsource = _table_grad(sd["dgates"], sd["step_tokens"], vocab)
            elif vocab <= 128:  # step t's input is the token chosen at step t - 1 (@start@ first)
                dsource = embedding_grad(sd["dgates"], sd["step_tokens"], vocab, shift=True, start=start)
            else:
                tok_in = torch.cat((sd["step_tokens"].new_full((B, 1), start), sd["step_tokens"][:, :-1]), 1).reshape(-1)
                dsource = torch.zeros(vocab, 4 * Hd, dtype=flat.dtype, device=dev).index_add_(0, tok_in, flat)
        grads += [dsource, denc, None, sd["dh0"], dw_c, dw_hh]
    return grads


class _AttnLSTMDecoder(torch.autograd.Function):
    """One decoding loop as one persistent kernel launch each way, with every input positional.

    inputs : xe [B,T,4H] (teacher forcing) or etable [V,4H] (free running; teacher forcing with ``in_tokens``), enc [B,S,H],
             mask [B,S] float, h0 [B,H], W_c [4H,H], W_hh [4H,H], W_p [V,H], b_p [V]
    outputs: hidden states [B,T,H], tokens [B,T] (free running only)
    An adaptor over ``_decoder_forward`` / ``_decoder_sides_backward``, which say what runs."""

    @staticmethod
    def forward(ctx, xe, etable, enc, mask, h0, w_c, w_hh, w_p, b_p, mode, T, seed, row_offset, pad, unk, start,
                packs=None, in_tokens=None, filter=None, constraint=None):
        m = dict(mode=mode, T=T, seed=seed, row_offset=row_offset, pad=pad, unk=unk, start=start, packs=packs, w_p=w_p, b_p=b_p,
                 in_tokens=in_tokens if mode == 0 else None, filter=filter, constraint=constraint)
        ctx.projected = mode == 0 and in_tokens is None
        got = _decoder_forward([(xe if ctx.projected else etable, enc, mask, h0, w_c, w_hh)], [m])
        ctx.save_for_backward(*got.saved)
        ctx.side_meta = got.side_meta
        ctx.mark_non_differentiable(got.outs[1])
        return got.outs

    @staticmethod
    def backward(ctx, dhs, _):
        need = ctx.needs_input_grad
        d = _decoder_sides_backward(ctx.saved_tensors, ctx.side_meta, (dhs,), (need[0 if ctx.projected else 1], *need[2:7]))
        return ((d[0], None) if ctx.projected else (None, d[0])) + tuple(d[1:]) + (None,) * 13


class _AttnLSTMDecoderGroup(torch.autograd.Function):
    """ONE graph node for up to three independent decoder passes, so that their BACKWARD is one launch
    (``pnmn_attn_lstm_bwd_group``): the persistent decoder kernels are bound by their per-step hand-off latency, so side by
    side they take as long as the longest pass.  A pass is launched here -- those that are, side by side in one forward
    launch per two (``_decoder_forward``) -- or was launched earlier (``decode_pair_launch``).  In a training iteration the
    generator's two decodes run first (their samples are the reconstructor's input), the reconstructor's decode later -- but
    backward the three are independent, and on one stream they add their step counts on the iteration's critical chain (at
    128 questions per GPU the seq2seq backward IS that chain: 275 + 470 us of decoder kernels become 470).  Inputs: per pass
    the six tensors of ``_prepare_decoder_side``, then ``meta`` (its dict per pass; ``meta[k]["pre"]`` = index of the pass in
    ``pre``, or None / absent: launched here) and ``pre`` (the ``_DecoderLaunch`` of the earlier launch, or None).  Outputs:
    per pass the hidden states and the tokens.  Same arithmetic as one ``_AttnLSTMDecoder`` per pass, bit for bit."""

    @staticmethod
    def forward(ctx, *args):
        meta, pre = args[-2], args[-1]
        tens = args[:-2]
        now = [k for k, m in enumerate(meta) if m.get("pre") is None]
        where = {k: (pre, m["pre"]) for k, m in enumerate(meta) if m.get("pre") is not None}
        for i in range(0, len(now), 2):
            ks = now[i: i + 2]
            got = _decoder_forward([tens[6 * k: 6 * k + 6] for k in ks], [meta[k] for k in ks])
            where.update((k, (got, j)) for j, k in enumerate(ks))
        saved, side_meta, outs = [], [], []
        for k in range(len(meta)):
            launch, j = where[k]
            saved += launch.saved[_SIDE_SAVED * j: _SIDE_SAVED * (j + 1)]
            side_meta.append(launch.side_meta[j])
            outs += launch.outs[2 * j: 2 * j + 2]
        ctx.save_for_backward(*saved)
        ctx.side_meta = side_meta
        ctx.mark_non_differentiable(*outs[1::2])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        return (*_decoder_sides_backward(ctx.saved_tensors, ctx.side_meta, grads[0::2], ctx.needs_input_grad), None, None)


IDENTITY_FILTER = (1.0, 0, 1.0)


def sampling_filter(temperature=1.0, top_k=0, top_p=1.0):
    """(temperature, top_k, top_p) as the kernels take them (the rule: include/probnmn_hip.h, beside
    ``pnmn_sample_tokens``), or None for the identity filter (1, 0, 1).  ``ValueError`` for a temperature that is not
    finite or not positive, a negative or non-integer ``top_k``, a ``top_p`` outside (0, 1]."""
    try:
        t, p = float(temperature), float(top_p)
    except (TypeError, ValueError):
        raise ValueError("temperature and top_p must be numbers, got %r and %r" % (temperature, top_p))
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 0 or top_k > 2 ** 31 - 1:
        raise ValueError("top_k must be an integer >= 0 (0: no truncation), got %r" % (top_k,))
    if not (0.0 < p <= 1.0):
        raise ValueError("top_p must lie in (0, 1], got %r" % (top_p,))
    f = (t, int(top_k), p)
    return None if f == IDENTITY_FILTER else f


def constraint_tables(constraint, n_vocab: int, end_index: int):
    """``meta["constraint"]`` of a decoder pass, and what ``decode_beam`` hands its kernel: (token_class [V], next_state
    [n_states, n_classes], min_left [n_states], end index) from a token automaton (``ProgramCompiler.decoding_automaton``) as
    contiguous uint8 numpy arrays.  ``ValueError`` for tables of another shape or another vocabulary size."""
    tables = [np.ascontiguousarray(getattr(constraint, name), dtype=np.uint8) for name in ("token_class", "next_state", "min_left")]
    if tables[0].ndim != 1 or tables[0].shape[0] != n_vocab:
        raise ValueError("constraint: token_class covers %s tokens, the target vocabulary has %d" % (tables[0].shape, n_vocab))
    if tables[1].ndim != 2 or tables[2].shape != (tables[1].shape[0],):
        raise ValueError("constraint: next_state must be [n_states, n_classes] and min_left [n_states]")
    return (*tables, int(end_index))


def choose_tokens(logits: torch.Tensor, greedy: bool, seed: int, row_offset: int, step: int,
                  pad: int, unk: int, start: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
    """One decoding step's token choice on the device; returns (tokens int64 [B], logprob [B] no grad).  ``temperature``,
    ``top_k``, ``top_p``: the sampling filter (``sampling_filter``; a greedy choice ignores it); the log-probabilities stay
    those of the unmodified distribution."""
    filt = sampling_filter(temperature, top_k, top_p)
    logits = logits.detach().contiguous()
    B, V = logits.shape
    tokens = torch.empty(B, dtype=torch.long, device=logits.device)
    lp = torch.empty(B, dtype=torch.float32, device=logits.device)
    rec = None if filt is None else np.array([(*filt, 0)], _hip.SAMPLING_FILTER)
    _hip.check(_hip.lib().pnmn_sample_tokens(logits.data_ptr(), tokens.data_ptr(), lp.data_ptr(), B, V, int(greedy),
                                             seed, row_offset, step, pad, unk, start, 0 if rec is None else rec.ctypes.data,
                                             _hip.stream_ptr(logits.device)), "sample_tokens")
    return tokens, lp


def add_sentence_boundary_token_ids(tokens: torch.Tensor, pad: int, bos: int, eos: int) -> torch.Tensor:
    """(B,T) right-padded -> (B,T+2): @start@ first, @end@ right after the last real token
    (allennlp.nn.util.add_sentence_boundary_token_ids, vectorised)."""
    B, T = tokens.shape
    lengths = (tokens != pad).sum(1)
    out = tokens.new_zeros(B, T + 2)
    out[:, 1:-1] = tokens
    out[:, 0] = bos
    out.scatter_(1, (lengths + 1).unsqueeze(1), eos)
    return out


def masked_softmax(vector: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """allennlp.nn.util.masked_softmax (memory_efficient=False), including its 1e-13."""
    result = F.softmax(vector * mask, dim=-1) * mask
    return result / (result.sum(dim=-1, keepdim=True) + 1e-13)


def sequence_cross_entropy(logits, targets, weights, eps: float = 1e-13):
    """Per-sequence masked-mean cross entropy (allennlp sequence_cross_entropy_with_logits,
    average=None) with explicit weights -- plain torch ops (the kernels take a token mask, see
    ``sequence_nll``)."""
    weights = weights.float()
    nll = -F.log_softmax(logits, dim=-1).gather(2, targets.unsqueeze(-1)).squeeze(-1) * weights
    return nll.sum(1) / (weights.sum(1) + eps)


class _SeqNLL(torch.autograd.Function):
    """``pnmn_seq_nll_{fwd,bwd}``: one launch instead of log_softmax / gather / mask / sum / divide."""

    @staticmethod
    def forward(ctx, logits, tokens, mask_tokens, pad, eps):
        B, T, V = logits.shape
        if logits.stride(2) != 1 or logits.stride(1) != V:
            logits = logits.contiguous()
        if tokens.stride(1) != 1:
            tokens = tokens.contiguous()
        if mask_tokens.stride(1) != 1:
            mask_tokens = mask_tokens.contiguous()
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
        lse = torch.empty(B, T, dtype=torch.float32, device=logits.device)
        _hip.check(_hip.lib().pnmn_seq_nll_fwd(logits.data_ptr(), logits.stride(0), tokens.data_ptr(), tokens.stride(0),
                                               mask_tokens.data_ptr(), mask_tokens.stride(0), pad, loss.data_ptr(),
                                               lse.data_ptr(), B, T, V, eps, _hip.stream_ptr(logits.device)), "seq_nll_fwd")
        ctx.save_for_backward(logits, tokens, mask_tokens, lse)
        ctx.pad, ctx.eps = pad, eps
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, tokens, mask_tokens, lse = ctx.saved_tensors
        B, T, V = logits.shape
        dlogits = torch.empty(B, T, V, dtype=torch.float32, device=logits.device)
        dloss = dloss.contiguous()
        _hip.check(_hip.lib().pnmn_seq_nll_bwd(logits.data_ptr(), logits.stride(0), tokens.data_ptr(), tokens.stride(0),
                                               mask_tokens.data_ptr(), mask_tokens.stride(0), ctx.pad, lse.data_ptr(),
                                               dloss.data_ptr(), dlogits.data_ptr(), T * V, B, T, V, ctx.eps,
                                               _hip.stream_ptr(logits.device)), "seq_nll_bwd")
        return dlogits, None, None, None, None


def sequence_nll(logits: torch.Tensor, tokens: torch.Tensor, mask_tokens: torch.Tensor, pad: int, eps: float) -> torch.Tensor:
    """loss[b] = sum_t w_t (-log_softmax(logits[b,t])[tokens[b,t]]) / (sum_t w_t + eps), w = mask_tokens != pad.
    Covers both sequence losses of the reference: teacher-forced cross entropy (tokens = mask_tokens =
    targets, eps 1e-13: allennlp's sequence_cross_entropy_with_logits) and the negative mean log-probability
    of a sampled sequence (tokens = the raw samples, mask_tokens = the trimmed predictions, eps 1e-12:
    seq2seq_base.py:235-244)."""
    if logits.device.type != "cuda":
        raise _hip.HipLibraryError("sequence loss input on %s: the HIP path needs a ROCm device" % logits.device)
    return _SeqNLL.apply(logits, tokens, mask_tokens, pad, eps)


def lstm_derived_specs(lstm: nn.LSTM, prefix: str = "l"):
    """DerivedParams specs of an ``nn.LSTM``: per layer the fragment-order W_hh, its transpose and b_ih + b_hh."""
    specs = []
    for layer in range(lstm.num_layers):
        w_hh = getattr(lstm, "weight_hh_l%d" % layer)
        specs.append(("%s%d.hh" % (prefix, layer), "pack", w_hh, None))
        specs.append(("%s%d.hhT" % (prefix, layer), "packT", w_hh, None))
        specs.append(("%s%d.b" % (prefix, layer), "sum", getattr(lstm, "bias_ih_l%d" % layer), getattr(lstm, "bias_hh_l%d" % layer)))
        if layer > 0 and lstm.input_size == lstm.hidden_size == 256:
            # the wavefront launches (pnmn_lstm_stack_*) keep a slice of the upper layers' input weights in registers too
            w_ih = getattr(lstm, "weight_ih_l%d" % layer)
            specs.append(("%s%d.ih" % (prefix, layer), "pack", w_ih, None))
            specs.append(("%s%d.ihT" % (prefix, layer), "packT", w_ih, None))
    return specs


def lstm_derived_params(lstm: nn.LSTM):
    """The parameters ``lstm_derived_specs`` reads (cache key of ``DerivedParams.get``)."""
    return [getattr(lstm, "%s_l%d" % (n, layer)) for layer in range(lstm.num_layers)
            for n in ("weight_hh", "bias_ih", "bias_hh") + (("weight_ih",) if layer > 0 else ())]


_SLOW_PATHS_NOTED = set()


def _note_slow_path(what: str, why: str) -> None:
    """The step-by-step paths (a GEMM and a cell kernel per time step) serve shapes no reference config has; they are
    correct and ~10x slower than the persistent kernels, so they say so once instead of engaging silently."""
    if what not in _SLOW_PATHS_NOTED:
        _SLOW_PATHS_NOTED.add(what)
        import warnings

        warnings.warn("probnmn seq2seq %s runs step by step (one GEMM + one cell launch per time step): %s" % (what, why),
                      RuntimeWarning, stacklevel=3)


def lstm_bias(lstm: nn.LSTM, layer: int, derived: Optional[Dict[str, torch.Tensor]], prefix: str = "l") -> torch.Tensor:
    b_ih, b_hh = getattr(lstm, "bias_ih_l%d" % layer), getattr(lstm, "bias_hh_l%d" % layer)
    if derived is None:
        return b_ih + b_hh
    return _Alias.apply(b_ih, b_hh, derived["%s%d.b" % (prefix, layer)])


def masked_lstm(lstm: nn.LSTM, x: torch.Tensor, mask: torch.Tensor, first_projection: Optional[torch.Tensor] = None,
                derived: Optional[Dict[str, torch.Tensor]] = None, last: Optional[torch.Tensor] = None,
                first_tokens: Optional[torch.Tensor] = None, dropout_seed: Optional[int] = None, row_offset: int = 0,
                dropout: bool = True):
    """``PytorchSeq2SeqWrapper(nn.LSTM)(x, mask)``: zero initial state, outputs zero past each row's
    length.  The input GEMM is batched over time and the recurrence is one persistent HIP kernel per layer.  Without
    ``last`` rows are run over all T steps (a unidirectional state never sees later steps); with it (and hidden size 256)
    the layers' row tiles are grouped by length and each runs to its longest row (``length_order``; one order for all
    layers and both directions; PNMN_LSTM_LENGTH_ORDER=0: all T steps as before).
    ``first_projection``: the first layer's input projection when the caller already has it
    ; ``x`` is then unused -- with ``first_tokens`` it is the [V,4H] per-token TABLE and the
    layer kernel looks the rows up itself.  ``derived``: the model's ``DerivedParams`` output (packed
    weights, bias sums).  ``last`` ([B] int32, ``mask`` then being the float mask): also return each row's
    state at that step -- (outputs, last states) from one launch.  In training mode with ``lstm.dropout`` > 0 the output of
    every layer but the last passes through ``_LSTMDropout`` under ``dropout_seed`` (drawn here when not given) with row keys
    from ``row_offset``.  ``dropout=False``: no mask and no seed drawn whatever the mode (inference inside a training run)."""
    B, T = mask.shape
    inp = x
    if not dropout:
        dropout_seed = None
    elif dropout_seed is None:
        dropout_seed = lstm_dropout_seed(lstm)
    order = tile_steps = None
    if last is not None and lstm.hidden_size == 256 and lstm_length_order_enabled():
        order, tile_steps = length_order(last, T)
    for layer in range(lstm.num_layers):
        w_ih = getattr(lstm, "weight_ih_l%d" % layer)
        w_hh = getattr(lstm, "weight_hh_l%d" % layer)
        tokens = None
        if layer == 0 and first_projection is not None:
            xp = first_projection
            if first_tokens is not None:
                if lstm.hidden_size == 256:
                    tokens = first_tokens
                else:
                    xp = _EmbeddingLookup.apply(xp, first_tokens, None)
        else:
            xp = linear_rows(inp, w_ih, lstm_bias(lstm, layer, derived))  # (B,T,4H): one GEMM for all time steps
        if lstm.hidden_size == 256:
            # one persistent launch for all T steps
            if derived is not None:
                inp = _LSTMLayerSeq.apply(xp, w_hh, derived["l%d.hh" % layer], derived["l%d.hhT" % layer], tokens, order, tile_steps)
            else:
                inp = _LSTMLayerSeq.apply(xp, w_hh, None, None, tokens, order, tile_steps)
        else:  # other widths: step by step (GEMM per step + the cell kernel)
            _note_slow_path("LSTM layer", "hidden size %d (the persistent layer kernel is built for 256)" % lstm.hidden_size)
            h = xp.new_zeros(B, lstm.hidden_size)
            c = xp.new_zeros(B, lstm.hidden_size)
            w_hh_t = w_hh.t()
            outs = []
            for t in range(T):
                gates = torch.addmm(xp[:, t], h, w_hh_t)
                h, c = lstm_cell_pointwise(gates, c)
                outs.append(h)
            inp = torch.stack(outs, 1)
        if dropout_seed is not None and layer + 1 < lstm.num_layers:
            inp = _LSTMDropout.apply(inp, float(lstm.dropout), dropout_seed, row_offset)
    if last is not None:
        return _MaskAndLast.apply(inp, mask, last)
    return inp * mask.unsqueeze(-1).to(inp.dtype)


class _TokenEmbedder(nn.Module):
    """``BasicTextFieldEmbedder({"tokens": Embedding})`` as far as parameter naming goes."""

    def __init__(self, key: str, num_embeddings: int, dim: int, padding_index: int):
        super().__init__()
        emb = nn.Embedding(num_embeddings, dim, padding_idx=padding_index)
        nn.init.xavier_uniform_(emb.weight)  # AllenNLP Embedding init, then zero padding row
        with torch.no_grad():
            emb.weight[padding_index].fill_(0)
        setattr(self, "token_embedder_" + key, emb)
        self._key = "token_embedder_" + key

    @property
    def embedding(self) -> nn.Embedding:
        return getattr(self, self._key)

    def forward(self, tokens):
        return embedding_lookup(self.embedding, tokens)


class _Encoder(nn.Module):
    def __init__(self, input_size, hidden_size, num_layers, dropout):
        super().__init__()
        self._module = nn.LSTM(input_size, hidden_size, num_layers, dropout=dropout, batch_first=True)

    def forward(self, x, mask):
        return masked_lstm(self._module, x, mask)

    def forward_tokens(self, embedding: nn.Embedding, tokens: torch.Tensor, mask: torch.Tensor,
                       derived: Optional[Dict[str, torch.Tensor]] = None, last: Optional[torch.Tensor] = None,
                       dropout_seed: Optional[int] = None, row_offset: int = 0, dropout: bool = True):
        """``forward(embedding(tokens), mask)`` with the first layer's input projection taken from a
        per-token table (``_TokenTable``: V < 100 projected rows instead of a GEMM over all B x T); with ``last`` also each row's state at that step."""
        lstm = self._module
        table = _TokenTable.apply(embedding.weight, lstm.weight_ih_l0, lstm_bias(lstm, 0, derived), embedding.padding_idx)
        return masked_lstm(lstm, None, mask, first_projection=table, derived=derived, last=last, first_tokens=tokens,
                           dropout_seed=dropout_seed, row_offset=row_offset, dropout=dropout)


class Seq2SeqBase(nn.Module):
    def __init__(
        self,
        vocabulary,
        source_namespace: str,
        target_namespace: str,
        input_size: int = 256,
        hidden_size: int = 256,
        num_layers: int = 2,
        dropout: float = 0.0,
        max_decoding_steps: int = 30,
    ):
        super().__init__()
        self.vocabulary = vocabulary
        # @@PADDING@@, @@UNKNOWN@@, @start@, @end@ have the same indices in all namespaces
        self._pad_index = vocabulary.get_token_index("@@PADDING@@", namespace=source_namespace)
        self._unk_index = vocabulary.get_token_index("@@UNKNOWN@@", namespace=source_namespace)
        self._end_index = vocabulary.get_token_index("@end@", namespace=target_namespace)
        self._start_index = vocabulary.get_token_index("@start@", namespace=target_namespace)
        self._max_decoding_steps = max_decoding_steps
        self._scheduled_sampling_ratio = 0.0

        v_src = vocabulary.get_vocab_size(namespace=source_namespace)
        v_tgt = vocabulary.get_vocab_size(namespace=target_namespace)
        self._source_embedder = _TokenEmbedder("tokens", v_src, input_size, self._pad_index)
        self._encoder = _Encoder(input_size, hidden_size, num_layers, dropout)
        # SimpleSeq2Seq: target embedding dim = source embedding dim; decoder dim = encoder dim
        self._target_embedder = nn.Embedding(v_tgt, input_size)
        nn.init.xavier_uniform_(self._target_embedder.weight)
        self._decoder_cell = nn.LSTMCell(hidden_size + input_size, hidden_size)
        self._output_projection_layer = nn.Linear(hidden_size, v_tgt)

        self._log2_perplexity = Average()
        self._sequence_accuracy = Average()
        self._unigram_recall = Average()
        # SimpleSeq2Seq(use_bleu=True): BLEU over evaluation predictions, special indices excluded
        self._bleu = BLEU(exclude_indices={self._pad_index, self._end_index, self._start_index})
        # row offset of this rank's shard in the global batch (keeps the sample stream shard-invariant)
        self.sample_row_offset = 0
        self.__dict__["_derived_cache"] = DerivedParams()  # (not a submodule, not part of the state_dict)

    def _derived(self) -> Optional[Dict[str, torch.Tensor]]:
        """Packed recurrent weights and bias sums of this model (``DerivedParams``), None for shapes the
        persistent kernels are not built for."""
        lstm, cell = self._encoder._module, self._decoder_cell
        Hd = cell.hidden_size
        if lstm.hidden_size != 256 or Hd != 256 or lstm.weight_hh_l0.device.type != "cuda":
            return None
        def specs():
            w_c = cell.weight_ih[:, :Hd]
            return lstm_derived_specs(lstm) + [
                ("d.c", "pack", w_c, None), ("d.hh", "pack", cell.weight_hh, None),
                ("d.cT", "packT", w_c, None), ("d.hhT", "packT", cell.weight_hh, None),
                ("d.b", "sum", cell.bias_ih, cell.bias_hh)]

        return self._derived_cache.get(lstm_derived_params(lstm) + [cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh],
                                       specs)

    # ---------------------------------------------------------------------------------------------
    def forward(
        self,
        source_tokens: torch.LongTensor,
        target_tokens: Optional[torch.LongTensor] = None,
        decoding_strategy: str = "sampling",
        need_predictions: bool = True,
        beam_size: int = 4,
        constraint=None,
        temperature: float = 1.0,
        top_k: int = 0,
        top_p: float = 1.0,
    ) -> Dict[str, torch.Tensor]:
        """``decoding_strategy``: "sampling" / "greedy" as the reference; "beam": beam search of width ``beam_size`` (free
        running only, no gradients -- see ``decode_beam``); "stochastic_beam": ``beam_size`` hypotheses sampled without
        replacement, accepted wherever "beam" is, with the same argument rules (see ``decode_stochastic_beam``; it draws one
        seed from the torch CPU generator); "constrained_sampling" / "constrained_greedy": a sampled / arg-max
        decode under the token automaton ``constraint`` (free running, inference only -- see ``decode_constrained``).
        ``beam_size`` is ignored by the other strategies; ``constraint`` (a token automaton) is required by the constrained
        strategies, optional for "beam" and refused by "sampling" / "greedy".  ``temperature``, ``top_k``, ``top_p``: the
        sampling filter, "sampling" and "constrained_sampling" only (see ``decode``).  "grammar_sampling": the TRAINING twin of
        "sampling" under ``constraint`` (required) -- sampled, or teacher forced on ``target_tokens``, with a graph and the
        encoder's dropout following the module's mode, scored under the grammar-normalised distribution (``decode_grammar``)."""
        self._check_filter(decoding_strategy, temperature, top_k, top_p)
        if decoding_strategy == "grammar_sampling":
            if constraint is None:
                raise ValueError("decoding_strategy='grammar_sampling' needs constraint= (a token automaton)")
            return self.decode_grammar(self.encode(source_tokens), constraint, target_tokens)
        if decoding_strategy in self.CONSTRAINED_STRATEGIES:
            self._check_constrained_arguments(target_tokens, constraint)
            with torch.no_grad():  # (the encoder without its dropout, as for "beam": the same in train() and eval() mode)
                return self.decode_constrained(self.encode(source_tokens, dropout=False), constraint,
                                               greedy=decoding_strategy == "constrained_greedy", temperature=temperature,
                                               top_k=top_k, top_p=top_p)
        if decoding_strategy in ("beam", "stochastic_beam"):
            self._check_beam_arguments(target_tokens, beam_size, decoding_strategy)
            with torch.no_grad():  # (the encoder without its dropout: the search is the same in train() and eval() mode)
                state = self.encode(source_tokens, dropout=False)
                if decoding_strategy == "stochastic_beam":
                    return self.decode_stochastic_beam(state, beam_size, constraint=constraint)
                return self.decode_beam(state, beam_size, constraint=constraint)
        if constraint is not None:
            raise ValueError("constraint: only decoding_strategy='beam' / 'stochastic_beam' decode under a token automaton")
        return self.decode(self.encode(source_tokens), target_tokens, decoding_strategy, need_predictions,
                           temperature=temperature, top_k=top_k, top_p=top_p)

    def encode(self, source_tokens: torch.LongTensor, dropout: bool = True) -> Dict[str, torch.Tensor]:
        """Encoder half of ``forward`` (reference seq2seq_base.py ``_encode`` + ``_init_decoder_state``).
        Rows are independent, so a trainer may encode one batch once and ``decode`` row subsets of
        the state in different modes (``select_rows``).  ``dropout=False``: the encoder's LSTM dropout is off whatever the
        mode and no seed is drawn for it -- what ``decoding_strategy="beam"`` encodes with, and what a caller of
        ``decode(state, decoding_strategy="beam")`` on a model in ``train()`` mode wants its state from."""
        if source_tokens.device.type != "cuda":
            raise _hip.HipLibraryError("seq2seq input on %s: the HIP path needs a ROCm device" % source_tokens.device)
        pad, bos, eos = self._pad_index, self._start_index, self._end_index
        # boundaries (@start@ is not encoded), mask and index of the last real token: one launch
        src, fmask, last = _TokenPrep.run(source_tokens, pad, bos, eos, drop_first=True, want_mask=True)
        # (the dropout seed of this pass, if it drops anything, is drawn before any seed of the decodes that follow)
        seed = lstm_dropout_seed(self._encoder._module) if dropout else None
        enc, h = self._encoder.forward_tokens(self._source_embedder.embedding, src, fmask, derived=self._derived(), last=last,
                                              dropout_seed=seed, row_offset=self.sample_row_offset, dropout=dropout)
        return {"enc": enc, "h": h, "fmask": fmask}

    @staticmethod
    def select_rows(state: Dict[str, torch.Tensor], rows: torch.LongTensor) -> Dict[str, torch.Tensor]:
        return {k: v.index_select(0, rows) for k, v in state.items()}

    @staticmethod
    def split_rows(state: Dict[str, torch.Tensor], n: int):
        """The state of rows ``[0, n)`` and of rows ``[n, B)`` -- views, no copies (a trainer that wants two row SETS
        decoded differently encodes the batch in that order: rows are independent)."""
        first, rest = {}, {}
        for k, v in state.items():
            if v.requires_grad:
                first[k], rest[k] = _SplitRows.apply(v, n)
            else:
                first[k], rest[k] = v[:n], v[n:]
        return first, rest

    def decode(
        self,
        state: Dict[str, torch.Tensor],
        target_tokens: Optional[torch.LongTensor] = None,
        decoding_strategy: str = "sampling",
        need_predictions: bool = True,
        seed: Optional[int] = None,
        beam_size: int = 4,
        constraint=None,
        temperature: float = 1.0,
        top_k: int = 0,
        top_p: float = 1.0,
    ) -> Dict[str, torch.Tensor]:
        """``need_predictions=False`` (teacher forcing only): skip drawing the per-step predictions from the
        teacher-forced distributions (reference :196-220) -- training iterations never read them.  ``seed``: the sampler
        seed a ``decode_prepare`` of this pass already drew (its pairing fell through): one draw per pass either way, so
        paired and unpaired schedules sample the same programs from the same torch seed.  ``decoding_strategy="beam"``:
        ``decode_beam`` with ``beam_size`` (which the other strategies ignore) and ``constraint``.
        ``decoding_strategy="constrained_sampling"`` / ``"constrained_greedy"``: ``decode_constrained`` under ``constraint``
        (required; "sampling" / "greedy" refuse one).  ``decoding_strategy="grammar_sampling"``: ``decode_grammar`` under
        ``constraint`` (required), free running or teacher forced, with a graph; it takes no filter.
        ``temperature``, ``top_k``, ``top_p`` (``decoding_strategy="sampling"`` / ``"constrained_sampling"`` only; anything but
        (1, 0, 1) with another strategy is a ``ValueError``): the tokens -- the free-running decode's, and the predictions drawn from teacher-forced
        distributions -- are drawn from the distribution sharpened by the temperature and cut to its ``top_k`` most likely
        tokens and its ``top_p`` nucleus (the rule: include/probnmn_hip.h).  They use the uniforms an unfiltered decode from
        the same seed uses, and ``loss`` still scores them under the unmodified distribution.  Shapes outside the persistent
        kernels have no filtered path: ``NotImplementedError``."""
        filt = self._check_filter(decoding_strategy, temperature, top_k, top_p)
        if decoding_strategy in self.CONSTRAINED_STRATEGIES:
            self._check_constrained_arguments(target_tokens, constraint)
            return self.decode_constrained(state, constraint, greedy=decoding_strategy == "constrained_greedy", seed=seed,
                                           temperature=temperature, top_k=top_k, top_p=top_p)
        if decoding_strategy == "grammar_sampling":
            if constraint is None:
                raise ValueError("decoding_strategy='grammar_sampling' needs constraint= (a token automaton)")
            return self.decode_grammar(state, constraint, target_tokens, seed=seed)
        if decoding_strategy == "beam":
            self._check_beam_arguments(target_tokens, beam_size)
            return self.decode_beam(state, beam_size, constraint=constraint)
        if decoding_strategy == "stochastic_beam":
            self._check_beam_arguments(target_tokens, beam_size, decoding_strategy)
            return self.decode_stochastic_beam(state, beam_size, seed=seed, constraint=constraint)
        if constraint is not None:
            raise ValueError("constraint: decoding_strategy='beam', 'stochastic_beam', 'constrained_sampling', "
                             "'constrained_greedy' and 'grammar_sampling' decode under a token automaton; %r does not"
                             % (decoding_strategy,))
        if decoding_strategy not in ("sampling", "greedy"):
            raise ValueError("decoding_strategy must be 'sampling', 'greedy', 'beam', 'stochastic_beam', 'constrained_sampling', "
                             "'constrained_greedy' or 'grammar_sampling'")
        pad, bos, eos = self._pad_index, self._start_index, self._end_index
        enc, h, fmask = state["enc"], state["h"], state["fmask"]
        tgt = None
        if target_tokens is not None:
            tgt = _TokenPrep.run(target_tokens, pad, bos, eos, drop_first=False, want_mask=False)[0]
        B = enc.size(0)

        steps = tgt.size(1) - 1 if tgt is not None else self._max_decoding_steps
        greedy = decoding_strategy == "greedy"
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        Hd = h.size(1)
        fused = Hd == 256 and enc.size(1) <= 64 and self._output_projection_layer.weight.size(0) <= 128
        if fused:
            prep = self._fused_prep(state, tgt, greedy, seed, self._derived())
            if filt is not None:
                prep["meta"]["filter"] = filt
            hs, raw = _AttnLSTMDecoderGroup.apply(*_prep_tensors(prep), [prep["meta"]], None)
            output_dict, logits_all = self._finish(prep, hs, raw)
            if tgt is not None and (need_predictions or not self.training):
                # predictions are drawn / arg-maxed from the teacher-forced distributions (reference :196-220)
                raw, _ = choose_tokens(logits_all.reshape(B * steps, -1), greedy, seed, self.sample_row_offset * steps,
                                       0, pad, self._unk_index, bos, *(filt or ()))
                output_dict["predictions"] = self._trim_predictions(raw.view(B, steps))
            ce = output_dict["loss"]
            predictions = output_dict.get("predictions")
        else:
            if filt is not None:
                raise NotImplementedError("temperature / top_k / top_p: hidden size %d, %d source positions, %d target tokens -- the "
                                          "filtered draw exists in the persistent decoder kernels only (256 / <= 64 / <= 128)"
                                          % (Hd, enc.size(1), self._output_projection_layer.weight.size(0)))
            _note_slow_path("decoder", "hidden size %d, %d source positions, %d target tokens (the persistent decoder kernel is "
                            "built for 256 / <= 64 / <= 128)" % (Hd, enc.size(1), self._output_projection_layer.weight.size(0)))
            raw, logits_all, logprobs = self._decode_stepwise(enc, fmask, h, torch.zeros_like(h), tgt, steps, greedy, seed)
            predictions = self._trim_predictions(raw)
            pmask = (predictions != pad).float()
            sequence_logprobs = (logprobs * pmask).sum(-1) / (pmask.sum(-1) + 1e-12)
            output_dict = {"predictions": predictions, "loss": -sequence_logprobs}
            if tgt is not None:
                tmask = tgt != pad
                ce = sequence_cross_entropy(logits_all, tgt[:, 1:], tmask[:, 1:])
                output_dict["loss"] = ce
        if tgt is not None:
            if not self.training:
                self._record_metrics(predictions, tgt[:, 1:], ce)
                self._bleu(predictions, tgt)  # (reference :260: against the targets WITH their @start@, as allennlp)
        return output_dict

    @staticmethod
    def _check_filter(decoding_strategy, temperature, top_k, top_p):
        """The sampling filter of a call (``sampling_filter``: None for the identity); ``ValueError`` for values out of range,
        and for a filter on a strategy that does not sample."""
        filt = sampling_filter(temperature, top_k, top_p)
        if filt is not None and decoding_strategy not in ("sampling", "constrained_sampling"):
            raise ValueError("temperature / top_k / top_p filter what decoding_strategy='sampling' draws; %r does not sample"
                             % (decoding_strategy,))
        return filt

    # ---- sampling and greedy decoding under a token automaton (inference) ----------------------------------------------
    CONSTRAINED_STRATEGIES = ("constrained_sampling", "constrained_greedy")

    @staticmethod
    def _check_constrained_arguments(target_tokens, constraint) -> None:
        if constraint is None:
            raise ValueError("decoding_strategy='constrained_sampling' / 'constrained_greedy' needs constraint= (a token automaton)")
        if target_tokens is not None:
            raise ValueError("a constrained decode is free running: it takes no target_tokens")

    @torch.no_grad()
    def decode_constrained(self, state: Dict[str, torch.Tensor], constraint, greedy: bool = False, seed: Optional[int] = None,
                           temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> Dict[str, torch.Tensor]:
        """A sampled (or, ``greedy``, arg-max) free-running decode over ``max_decoding_steps`` steps in which every row is a
        string the token automaton ``constraint`` accepts (``ProgramCompiler.decoding_automaton``: a valid program), on the
        persistent decoder kernels the unconstrained decode runs on (``pnmn_attn_lstm_fwd_group`` / ``pnmn_attn_lstm_fwd``
        with their tables; the rule is stated in include/probnmn_hip.h beside the latter).  At every step a row may take only
        the tokens from which an accepted string can still be completed in the steps that remain, and @end@ only where the
        string so far is accepted; the draw is the usual one restricted to that set (with ``temperature`` / ``top_k`` /
        ``top_p``: rank, top-k and nucleus within the set), the greedy choice the first largest logit within it.  The
        uniforms are those of an unconstrained sampling decode from the same seed.

        INFERENCE ONLY, no graph, the same in ``train()`` and ``eval()`` mode: a constrained draw is not a draw from the
        generator's distribution, so no trainer calls this (a trainer samples AND scores under the automaton through
        ``decode_grammar``, whose loss is under the distribution the draw comes from).  Returns ``predictions`` [B, T] (trimmed: padding after a row's
        first @end@) and ``loss`` [B], the length-normalised negative log-probability of the trimmed row as the sampling
        decode reports it -- ``log_softmax(z)[token]`` of the UNMODIFIED distribution, not of the restricted one.
        ``seed``: None draws ONE seed from the torch CPU generator, exactly as the sampling decode does; a greedy call
        draws none.  ``ValueError``: no constraint, tables of another vocabulary size, an automaton whose shortest accepted
        string is longer than ``max_decoding_steps``, a filter together with ``greedy``.  There is no step-by-step path:
        shapes outside the persistent kernels raise ``NotImplementedError``."""
        if constraint is None:
            raise ValueError("decode_constrained needs a token automaton")
        filt = sampling_filter(temperature, top_k, top_p)
        if greedy and filt is not None:
            raise ValueError("temperature / top_k / top_p filter a draw; a greedy constrained decode draws nothing")
        enc, h = state["enc"], state["h"]
        n_vocab, T = self._output_projection_layer.weight.size(0), self._max_decoding_steps
        tables = constraint_tables(constraint, n_vocab, self._end_index)
        if int(tables[2][0]) > T:
            raise ValueError("constraint: the shortest accepted string takes %d tokens, max_decoding_steps is %d" % (int(tables[2][0]), T))
        Hd = h.size(1)
        if not (Hd == 256 and enc.size(1) <= 64 and n_vocab <= 128):
            raise NotImplementedError("constrained decoding: hidden size %d, %d source positions, %d target tokens -- it exists in the "
                                      "persistent decoder kernels only (256 / <= 64 / <= 128)" % (Hd, enc.size(1), n_vocab))
        if greedy:
            seed = 0
        elif seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        state = {k: v.detach() for k, v in state.items()}
        prep = self._fused_prep(state, None, greedy, seed, self._derived())
        prep["meta"]["constraint"] = tables
        if filt is not None:
            prep["meta"]["filter"] = filt
        hs, raw = _AttnLSTMDecoderGroup.apply(*_prep_tensors(prep), [prep["meta"]], None)
        return self._finish(prep, hs, raw)[0]

    # ---- training under a token automaton: the grammar-normalised distribution ---------------------------------------------
    def decode_grammar(self, state: Dict[str, torch.Tensor], constraint, target_tokens: Optional[torch.LongTensor] = None,
                       seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``decoding_strategy="grammar_sampling"``: a decode WITH a graph on ``state`` as it is (the encoder's dropout as
        ``encode`` applied it), scored under q_c -- the generator's step distributions renormalised over the allowed sets
        of the token automaton ``constraint``, which is the distribution ``decode_constrained`` (unfiltered) draws from.
        ``loss`` is then a differentiable function of the model that the REINFORCE and likelihood estimators of the
        trainers may use with every sample a valid program (``probnmn.modules.grammar``).  The horizon of the rule is
        ``max_decoding_steps`` in both modes, never the batch's padded length.

        Without ``target_tokens``: the free-running sampled pass -- the launch ``decode_constrained`` makes, through the
        autograd node of the sampling decode.  ``predictions`` [B, T] (trimmed) and ``loss`` [B] =
        ``sequence_nll(grammar_logits(logits, raw)[0], raw, predictions, pad, 1e-12)``: the reference's length-normalised
        negative log-probability, under q_c.  With ``target_tokens``: teacher forced, ``loss`` [B] the cross entropy of
        ``decode`` over the masked logits (a target the grammar does not allow stays finite: it is added to its step's set,
        and counted); no predictions are drawn.  Both return ``grammar_log_mass`` [B] (the sum over the row's scored steps
        of the log share of the unconstrained step distribution inside the grammar: log q - log q_c of the row) and
        ``grammar_outside`` [B] (int32: scored tokens outside their allowed set; 0 for every sampled row).

        No metric is recorded.  One seed is drawn from the torch CPU generator when ``seed`` is None, exactly as "sampling"
        draws it, teacher forced or not.  ``ValueError``: no constraint, tables of another vocabulary size, an automaton
        whose shortest accepted string is longer than ``max_decoding_steps``.  Shapes outside the persistent kernels raise
        ``NotImplementedError``."""
        from probnmn.modules.grammar import check_horizon, grammar_logits, scored_log_mass

        if constraint is None:
            raise ValueError("decode_grammar needs a token automaton")
        enc, h = state["enc"], state["h"]
        proj = self._output_projection_layer
        n_vocab, T = proj.weight.size(0), self._max_decoding_steps
        tables = constraint_tables(constraint, n_vocab, self._end_index)
        check_horizon(tables, T)
        Hd = h.size(1)
        if not (Hd == 256 and enc.size(1) <= 64 and n_vocab <= 128):
            raise NotImplementedError("grammar_sampling: hidden size %d, %d source positions, %d target tokens -- it exists in the "
                                      "persistent decoder kernels only (256 / <= 64 / <= 128)" % (Hd, enc.size(1), n_vocab))
        pad, bos, eos = self._pad_index, self._start_index, self._end_index
        tgt = None
        if target_tokens is not None:
            tgt = _TokenPrep.run(target_tokens, pad, bos, eos, drop_first=False, want_mask=False)[0]
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        prep = self._fused_prep(state, tgt, False, seed, self._derived())
        if tgt is None:
            prep["meta"]["constraint"] = tables
        hs, raw = _AttnLSTMDecoderGroup.apply(*_prep_tensors(prep), [prep["meta"]], None)
        logits_all = linear_rows(hs, proj.weight, proj.bias)
        if tgt is None:
            predictions = self._trim_predictions(raw)
            scored, weighted, eps = raw, predictions, 1e-12
        else:
            scored = weighted = tgt[:, 1:]
            eps = 1e-13
        masked, log_mass, outside = grammar_logits(logits_all, scored, tables, T, pad, self._unk_index, bos, eos)
        out = {"loss": sequence_nll(masked, scored, weighted, pad, eps),
               "grammar_log_mass": scored_log_mass(log_mass, weighted, pad), "grammar_outside": outside}
        if tgt is None:
            out["predictions"] = predictions
        return out

    # ---- beam search (inference) ---------------------------------------------------------------------------------------
    BEAM_SIZES = (1, 2, 4, 8, 16)

    @staticmethod
    def _check_beam_arguments(target_tokens, beam_size, strategy="beam") -> None:
        if target_tokens is not None:
            raise ValueError("decoding_strategy=%r is free running: it takes no target_tokens" % (strategy,))
        if isinstance(beam_size, bool) or not isinstance(beam_size, int) or beam_size not in Seq2SeqBase.BEAM_SIZES:
            raise ValueError("beam_size must be one of %s, got %r" % (Seq2SeqBase.BEAM_SIZES, beam_size))

    @torch.no_grad()
    def decode_beam(self, state: Dict[str, torch.Tensor], beam_size: int = 4, trace: bool = False,
                    constraint=None) -> Dict[str, torch.Tensor]:
        """Beam search over ``max_decoding_steps`` steps in ONE launch of the persistent beam kernel
        (``pnmn_attn_lstm_beam``, csrc/decoder_beam.hip; the selection rule is stated in include/probnmn_hip.h).  Inference
        only: no graph, no seed drawn from the torch generator, the same in ``train()`` and ``eval()`` mode given a ``state``
        encoded without dropout (``encode(..., dropout=False)``, as ``forward`` does for this strategy).  Returns
        ``beam_predictions`` [B, K, T] (best first, each row trimmed at its first @end@), ``beam_log_probabilities`` [B, K]
        (sums of token log-probabilities), ``predictions`` = the best hypothesis and ``loss`` [B] = its negative
        log-probability over its number of non-padding tokens (the free-running sampled path's quantity).  ``trace=True``
        adds ``beam_trace``: (token, back-pointer, score) of every slot at every step, [B, T, K] each.  There is no
        step-by-step path for this mode: shapes outside the kernel's limits raise ``NotImplementedError``.

        ``constraint``: a token automaton (``token_class`` [V], ``next_state`` [n_states, n_classes], ``min_left``
        [n_states] as uint8 numpy arrays -- ``ProgramCompiler.decoding_automaton``).  The same call then gets its tables:
        a hypothesis offers a token only while an accepted completion stays reachable in the steps that remain, so every
        hypothesis with a finite score is accepted by the automaton.  The same keys come back.  ``None``: unconstrained."""
        return self._beam_launch(state, beam_size, trace, constraint, None)

    def _beam_launch(self, state, beam_size, trace, constraint, stochastic) -> Dict[str, torch.Tensor]:
        """``decode_beam`` (``stochastic`` None) or ``decode_stochastic_beam`` (``stochastic`` = the seed): one launch of the
        beam kernel and the trimming of what it returns."""
        self._check_beam_arguments(None, beam_size)
        tables = None
        if constraint is not None:
            tables = constraint_tables(constraint, self._output_projection_layer.weight.size(0), self._end_index)[:3]
        enc, h, fmask = state["enc"].detach(), state["h"].detach(), state["fmask"].detach()
        dev = enc.device
        if dev.type != "cuda":
            raise _hip.HipLibraryError("beam decoder on %s: the HIP path needs a ROCm device (no CPU fallback)" % dev)
        B, S, Hd = enc.shape
        K, T = beam_size, self._max_decoding_steps
        w_p, b_p = self._output_projection_layer.weight.detach(), self._output_projection_layer.bias.detach()
        V = w_p.size(0)
        for what, value, ok, limit in (("hidden size", Hd, Hd == 256, "256"), ("source positions", S, S <= 64, "<= 64"),
                                       ("target vocabulary", V, V <= 128, "<= 128"), ("decoding steps", T, T <= 64, "<= 64")):
            if not ok:
                raise NotImplementedError("beam search: %s = %d, the beam kernel is built for %s" % (what, value, limit))
        derived = self._derived()
        w_ih = self._decoder_cell.weight_ih.detach()
        if derived is not None:
            bias, w_c_p, w_hh_p = derived["d.b"], derived["d.c"], derived["d.hh"]
        else:
            bias = self._decoder_cell.bias_ih.detach() + self._decoder_cell.bias_hh.detach()
            w_c_p, w_hh_p = pack_fragments(w_ih[:, :Hd]), pack_fragments(self._decoder_cell.weight_hh)
        # (the token table is rebuilt per call, as the free-running path does: one small GEMM, ~0.01 ms, that a timing of this
        #  method includes; without DerivedParams -- never on a ROCm device at hidden 256 -- so are the two weight packs)
        etable = F.linear(self._target_embedder.weight.detach(), w_ih[:, Hd:], bias).contiguous()
        enc, h, fmask, w_p, b_p = enc.contiguous(), h.contiguous(), fmask.contiguous(), w_p.contiguous(), b_p.contiguous()
        raw = torch.empty(B, K, T, dtype=torch.long, device=dev)
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        perturbed = torch.empty(B, K, dtype=torch.float32, device=dev) if stochastic is not None else None
        tr = None
        if trace:
            tr = (torch.empty(B, T, K, dtype=torch.int32, device=dev), torch.empty(B, T, K, dtype=torch.int32, device=dev),
                  torch.empty(B, T, K, dtype=torch.float32, device=dev))
            if stochastic is not None:
                tr += (torch.empty(B, T, K, dtype=torch.float32, device=dev),)
        if B > 0 and T > 0:
            automaton = (0, 0, 0, 0, 0)  # (null tables: unconstrained)
            if tables is not None:  # (the tables are host arrays: the library checks every entry and passes them by value)
                automaton = (tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, *tables[1].shape)
            args = (etable.data_ptr(), enc.data_ptr(), fmask.data_ptr(), h.data_ptr(), w_c_p.data_ptr(), w_hh_p.data_ptr(),
                    w_p.data_ptr(), b_p.data_ptr(), raw.data_ptr(), scores.data_ptr(),
                    tr[0].data_ptr() if tr else None, tr[1].data_ptr() if tr else None, tr[2].data_ptr() if tr else None,
                    B, T, S, V, Hd, K, self._pad_index, self._unk_index, self._start_index, self._end_index, *automaton)
            if stochastic is None:
                _hip.check(_hip.lib().pnmn_attn_lstm_beam(*args, _hip.stream_ptr(dev)), "attn_lstm_beam")
            else:
                _hip.check(_hip.lib().pnmn_attn_lstm_beam_stochastic(
                    *args, perturbed.data_ptr(), tr[3].data_ptr() if tr else None, stochastic, self.sample_row_offset,
                    _hip.stream_ptr(dev)), "attn_lstm_beam_stochastic")
        beams = self._trim_predictions(raw.view(B * K, T)).view(B, K, T)
        best = beams[:, 0]
        n = (best != self._pad_index).sum(-1).to(scores.dtype)
        # (an empty best hypothesis, n = 0: the sampled path sums no log-probability and returns 0)
        loss = torch.where(n > 0, -scores[:, 0] / (n + 1e-12), torch.zeros_like(n))
        out = {"predictions": best, "loss": loss, "beam_predictions": beams, "beam_log_probabilities": scores}
        if stochastic is not None:
            out["beam_perturbed"] = perturbed
        if tr:
            out["beam_trace"] = {"tokens": tr[0], "backpointers": tr[1], "scores": tr[2]}
            if stochastic is not None:
                out["beam_trace"]["perturbed"] = tr[3]
        return out

    @torch.no_grad()
    def decode_stochastic_beam(self, state: Dict[str, torch.Tensor], beam_size: int = 4, seed: Optional[int] = None,
                               trace: bool = False, constraint=None) -> Dict[str, torch.Tensor]:
        """Stochastic beam search (Kool, van Hoof and Welling 2019) in ONE launch of the beam kernel's second candidate stage
        (``pnmn_attn_lstm_beam_stochastic``; the rule is stated in include/probnmn_hip.h): the K hypotheses of a question
        are an exact sample WITHOUT replacement from the decoder's sequence distribution -- K distinct sequences, in the
        order a sequential sample would draw them, so ``predictions`` (hypothesis 0) is an ordinary sample.  The
        distribution is the one the sampling decode draws from: every step's softmax restricted to the tokens that may be
        offered (never pad / unk / start; with ``constraint``, the automaton's rule, as ``decode_constrained``).

        Returns what ``decode_beam`` returns -- ``beam_predictions`` [B, K, T], ``beam_log_probabilities`` [B, K] (phi, the
        log-probability under that distribution), ``predictions``, ``loss`` -- and ``beam_perturbed`` [B, K], the perturbed
        log-probability G of every hypothesis (best first; ``evaluators.without_replacement_weights`` turns the two into
        importance weights).  A slot left without a sequence (the support is smaller than K) holds -inf in both.
        ``trace=True``: ``beam_trace`` gains ``"perturbed"``.

        ``seed``: None draws ONE seed from the torch CPU generator, exactly as the sampling decode does, so
        ``torch.manual_seed`` reproduces a run; the uniform of (question, slot, token, step) depends on the seed and on
        ``sample_row_offset`` + the question's row only, so a question draws the same hypotheses alone or in a batch.
        Inference only, no dropout, no graph; the refusals are ``decode_beam``'s and there is no CPU or step-by-step path."""
        self._check_beam_arguments(None, beam_size)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        return self._beam_launch(state, beam_size, trace, constraint, int(seed))

    # ---- two teacher-forced decodes of a training iteration side by side -------------------------------------------
    def decode_prepare(self, state: Dict[str, torch.Tensor], target_tokens: Optional[torch.LongTensor] = None,
                       decoding_strategy: str = "sampling"):
        """First half of a training ``decode`` whose persistent-kernel launch is to be shared with another pass
        (``decode_pair``): everything up to the launch.  ``target_tokens`` given: teacher forced; ``None``: free running
        (the kernel samples / arg-maxes each step's token).  Returns ``None`` when this pass cannot take part (shapes
        outside the fused kernels, evaluation: metrics want predictions from the teacher-forced distributions)."""
        enc, h, fmask = state["enc"], state["h"], state["fmask"]
        w_p, b_p = self._output_projection_layer.weight, self._output_projection_layer.bias
        Hd = h.size(1)
        if not (self.training and torch.is_grad_enabled() and enc.is_cuda and Hd == 256 and enc.size(1) <= 64 and w_p.size(0) <= 128):
            return None
        # the pair kernels are multi-CU only: PNMN_DECODER_CLUSTER=0, or a device that cannot host eight resident
        # workgroups per tile (the library then reports no workspace), leave both passes to decode()
        if _decoder_workspace_bytes([enc.size(0)], False) <= 0:
            return None
        derived = self._derived()
        if derived is None:
            return None
        tgt = None
        if target_tokens is not None:
            tgt = _TokenPrep.run(target_tokens, self._pad_index, self._start_index, self._end_index, drop_first=False,
                                 want_mask=False)[0]
        # (decode() draws one seed per pass, used or not: keep the generator in step)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        return self._fused_prep(state, tgt, decoding_strategy == "greedy", seed, derived)

    def _fused_prep(self, state: Dict[str, torch.Tensor], tgt: Optional[torch.Tensor], greedy: bool, seed: int,
                    derived: Optional[Dict[str, torch.Tensor]]):
        """The inputs of one pass through the persistent decoder kernels: the six tensors and the ``meta`` of
        ``_prepare_decoder_side`` (``_prep_tensors``), and what ``decode_finish`` reads.  ``tgt`` (targets with their
        boundary tokens): teacher forced; None: free running under ``seed``.  ``derived``: the model's ``DerivedParams``
        output, or None (the bias sum and the weight packs are then computed per call)."""
        Hd = state["h"].size(1)
        w_ih = self._decoder_cell.weight_ih
        # the cell's input is cat(attended, embedding)
        w_c, w_e = _SplitColumns.apply(w_ih, Hd) if w_ih.requires_grad and torch.is_grad_enabled() else (w_ih[:, :Hd], w_ih[:, Hd:])
        if derived is not None:
            bias = _Alias.apply(self._decoder_cell.bias_ih, self._decoder_cell.bias_hh, derived["d.b"])
            packs = (derived["d.c"], derived["d.hh"], derived["d.cT"], derived["d.hhT"])
        else:
            bias = self._decoder_cell.bias_ih + self._decoder_cell.bias_hh
            packs = None
        emb = self._target_embedder
        meta = {"packs": packs, "start": self._start_index}
        if tgt is not None:  # teacher forcing: every step's input embedding is known up front
            steps = tgt.size(1) - 1
            etable = _TokenTable.apply(emb.weight, w_e, bias, emb.padding_idx)
            meta.update(mode=0, in_tokens=tgt[:, :steps], T=steps)
        else:  # free running: the kernel also picks each step's token
            steps = self._max_decoding_steps
            etable = F.linear(emb.weight, w_e, bias)
            meta.update(mode=2 if greedy else 1, T=steps, pad=self._pad_index, unk=self._unk_index, seed=seed,
                        row_offset=self.sample_row_offset, w_p=self._output_projection_layer.weight,
                        b_p=self._output_projection_layer.bias)
        return {"model": self, "tgt": tgt, "steps": steps, "etable": etable, "enc": state["enc"], "fmask": state["fmask"],
                "h": state["h"], "w_c": w_c, "w_hh": self._decoder_cell.weight_hh, "meta": meta}

    def decode_finish(self, prep, hs: torch.Tensor, raw: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Second half: the output projection over all steps and the per-row loss -- the cross entropy of the targets
        (reference :235-254) or, free running, the length-normalised negative log-probability of the trimmed samples
        (reference :222-233)."""
        return self._finish(prep, hs, raw)[0]

    def _finish(self, prep, hs, raw):
        """``decode_finish`` and the logits [B,T,V] it took the loss from."""
        proj = self._output_projection_layer
        # one GEMM for all steps; its weight gradient [V, B*T] x [B*T, H] -- 44-100 output rows over a 13 000-47 000 long
        # reduction -- through the K-split of wgrad_gemm (as a plain mm: 80-144 us at 3-17 TFLOP/s, scripts/r05_gemm_sites.py)
        logits_all = linear_rows(hs, proj.weight, proj.bias)
        tgt = prep["tgt"]
        if tgt is not None:
            return {"loss": sequence_nll(logits_all, tgt[:, 1:], tgt[:, 1:], self._pad_index, 1e-13)}, logits_all
        predictions = self._trim_predictions(raw)
        return {"predictions": predictions, "loss": sequence_nll(logits_all, raw, predictions, self._pad_index, 1e-12)}, logits_all

    def _decode_stepwise(self, enc, fmask, h, c, tgt, steps, greedy, seed, choose: bool = True):
        """Step-by-step decoding for shapes the persistent kernel is not built for (hidden != 256,
        more than 64 source positions or 128 target tokens): a GEMM per step + the cell kernel.  ``choose=False`` (teacher
        forcing only): no token is chosen from the distributions; the tokens and their log-probabilities come back None."""
        B = enc.size(0)
        pad, bos = self._pad_index, self._start_index
        last = fmask.new_full((B,), bos, dtype=torch.long)
        w_ih_t = self._decoder_cell.weight_ih.t()
        w_hh_t = self._decoder_cell.weight_hh.t()
        bias = self._decoder_cell.bias_ih + self._decoder_cell.bias_hh
        step_logits, step_logprobs, step_predictions = [], [], []
        for t in range(steps):
            inputs = tgt[:, t] if tgt is not None else last
            e = self._target_embedder(inputs)
            scores = torch.bmm(enc, h.unsqueeze(-1)).squeeze(-1)
            weights = masked_softmax(scores, fmask)
            attended = torch.bmm(weights.unsqueeze(1), enc).squeeze(1)
            x = torch.cat((attended, e), -1)
            gates = torch.addmm(torch.addmm(bias, x, w_ih_t), h, w_hh_t)
            h, c = lstm_cell_pointwise(gates, c)
            logits = self._output_projection_layer(h)
            step_logits.append(logits.unsqueeze(1))
            if not choose:
                continue
            last, _ = choose_tokens(logits, greedy, seed, self.sample_row_offset, t, pad, self._unk_index, bos)
            step_predictions.append(last.unsqueeze(1))
            step_logprobs.append(F.log_softmax(logits, dim=-1).gather(1, last.unsqueeze(1)))
        if not choose:
            return None, torch.cat(step_logits, 1), None
        return torch.cat(step_predictions, 1), torch.cat(step_logits, 1), torch.cat(step_logprobs, 1)

    def teacher_forced_logits(self, source_tokens: torch.LongTensor, target_tokens: torch.LongTensor, *,
                              differentiable: bool = False, constraint=None):
        """The teacher-forced distributions of ``target_tokens`` given ``source_tokens``, for SCORING: (logits [R, T, V],
        targets [R, T]), ``targets`` being the ``tgt[:, 1:]`` that ``decode`` scores them against (the targets after their
        @start@, @end@ behind the last one, padding after) -- log p(target | source) is the sum over the non-padding targets
        of ``log_softmax(logits)[target]``.

        An inference pass that leaves the model as it was, unlike ``decode(state, targets)`` in ``eval()`` mode: no loss, no
        predictions drawn from the distributions, no metric (perplexity, accuracy, BLEU) touched, no seed drawn from the
        torch generator, no graph, the encoder without its dropout whatever the mode (``encode(dropout=False)``).  The
        persistent decoder kernels of ``decode`` on their shapes; step by step (``_decode_stepwise``) on the others.

        ``differentiable=True``: the same logits WITH a graph, to train the model on a loss of its sequence scores
        (``sequence_marginal_loss``): the persistent decoder runs through the autograd node ``decode`` uses for teacher
        forcing (``_AttnLSTMDecoderGroup``, then ``linear_rows``), step by step on the other shapes, and the encoder's
        dropout follows the module's mode as in ``forward`` (``train()`` mode with LSTM dropout draws one seed; in ``eval()``
        mode the logits are the plain call's).  Still no loss, no predictions, no metric and no BLEU.

        ``constraint`` (a token automaton): the logits come back masked to the allowed set of every step
        (``probnmn.modules.grammar.grammar_logits`` along the targets, horizon ``max_decoding_steps``), in both calls:
        ``log_softmax`` of them scores the targets under the grammar-normalised distribution q_c."""
        with torch.set_grad_enabled(torch.is_grad_enabled() and differentiable):
            if differentiable:
                logits, targets = self._teacher_forced_logits_with_graph(source_tokens, target_tokens)
            else:
                logits, targets = self._teacher_forced_logits(source_tokens, target_tokens)
            if constraint is not None:
                from probnmn.modules.grammar import grammar_logits

                logits = grammar_logits(logits, targets, constraint, self._max_decoding_steps, self._pad_index,
                                        self._unk_index, self._start_index, self._end_index)[0]
        return logits, targets

    def _teacher_forced_logits_with_graph(self, source_tokens, target_tokens):
        state = self.encode(source_tokens)
        tgt = _TokenPrep.run(target_tokens, self._pad_index, self._start_index, self._end_index, drop_first=False,
                             want_mask=False)[0]
        enc, h, fmask = state["enc"], state["h"], state["fmask"]
        proj = self._output_projection_layer
        if h.size(1) == 256 and enc.size(1) <= 64 and proj.weight.size(0) <= 128:
            prep = self._fused_prep(state, tgt, False, 0, self._derived())
            hs, _ = _AttnLSTMDecoderGroup.apply(*_prep_tensors(prep), [prep["meta"]], None)
            logits = linear_rows(hs, proj.weight, proj.bias)
        else:
            _note_slow_path("decoder", "hidden size %d, %d source positions, %d target tokens (the persistent decoder kernel is "
                            "built for 256 / <= 64 / <= 128)" % (h.size(1), enc.size(1), proj.weight.size(0)))
            logits = self._decode_stepwise(enc, fmask, h, torch.zeros_like(h), tgt, tgt.size(1) - 1, True, 0, choose=False)[1]
        return logits, tgt[:, 1:]

    def _teacher_forced_logits(self, source_tokens, target_tokens):
        state = self.encode(source_tokens, dropout=False)
        tgt = _TokenPrep.run(target_tokens, self._pad_index, self._start_index, self._end_index, drop_first=False,
                             want_mask=False)[0]
        enc, h, fmask = state["enc"], state["h"], state["fmask"]
        proj = self._output_projection_layer
        if h.size(1) == 256 and enc.size(1) <= 64 and proj.weight.size(0) <= 128:
            prep = self._fused_prep(state, tgt, False, 0, self._derived())
            hs = _decoder_forward([_prep_tensors(prep)], [prep["meta"]]).outs[0]
            logits = linear_rows(hs, proj.weight, proj.bias)
        else:
            _note_slow_path("decoder", "hidden size %d, %d source positions, %d target tokens (the persistent decoder kernel is "
                            "built for 256 / <= 64 / <= 128)" % (h.size(1), enc.size(1), proj.weight.size(0)))
            logits = self._decode_stepwise(enc, fmask, h, torch.zeros_like(h), tgt, tgt.size(1) - 1, True, 0, choose=False)[1]
        return logits, tgt[:, 1:]

    def _trim_predictions(self, predictions: torch.LongTensor) -> torch.LongTensor:
        """Keep each row up to and including its first @end@; a row starting with @end@ becomes all
        padding, a row without @end@ is kept whole (reference :278-293), without leaving the device."""
        if predictions.device.type == "cuda" and predictions.dtype == torch.long and predictions.dim() == 2:
            predictions = predictions.contiguous()
            out = torch.empty_like(predictions)
            _hip.check(_hip.lib().pnmn_trim_predictions(predictions.data_ptr(), predictions.size(0), predictions.size(1),
                                                        self._end_index, out.data_ptr(), _hip.stream_ptr(predictions.device)),
                       "trim_predictions")
            return out
        steps = predictions.size(1)
        is_end = predictions == self._end_index
        has_end = is_end.any(1, keepdim=True)
        first = is_end.float().argmax(1, keepdim=True)  # first occurrence
        pos = torch.arange(steps, device=predictions.device).unsqueeze(0)
        keep = torch.where(has_end, (pos <= first) & (first > 0), torch.ones_like(is_end))
        return predictions * keep

    @torch.no_grad()
    def _record_metrics(self, predictions, relevant_targets, ce) -> None:
        n = relevant_targets.size(1)
        pred = predictions[:, :n]
        mask = relevant_targets != self._pad_index
        correct = ((pred == relevant_targets) | ~mask).all(1).float().mean()
        # unigram recall: fraction of gold tokens that appear anywhere in the prediction
        hit = (relevant_targets.unsqueeze(2) == pred.unsqueeze(1)).any(2) & mask
        recall = (hit.sum(1).float() / mask.sum(1).clamp(min=1).float()).mean()
        self._log2_perplexity(ce.mean())
        self._sequence_accuracy(correct)
        self._unigram_recall(recall)

    def get_metrics(self, reset: bool = True) -> Dict[str, float]:
        if self.training:
            return {}
        return {
            **self._bleu.get_metric(reset=True),  # (the reference resets BLEU unconditionally, :367)
            "perplexity": 2 ** self._log2_perplexity.get_metric(reset=reset),
            "sequence_accuracy": self._sequence_accuracy.get_metric(reset=reset),
            "word_error_rate": 1 - self._unigram_recall.get_metric(reset=reset),
        }


def _prep_tensors(prep):
    """A prepared decode's tensor inputs, in ``_prepare_decoder_side``'s order."""
    return prep["etable"], prep["enc"], prep["fmask"], prep["h"], prep["w_c"], prep["w_hh"]


def decode_pair(prep_a, prep_b):
    """The launches of two prepared decodes (``Seq2SeqBase.decode_prepare``) as one, then each model's second half.
    Returns the two output dicts ({"loss": per-row loss[, "predictions"]})."""
    return tuple(decode_group([prep_a, prep_b], None, [None, None]))


def decode_pair_launch(prep_a, prep_b) -> _DecoderLaunch:
    """The forward launch of two prepared decodes NOW, without a graph node: returns what ``decode_group`` needs to create
    the node later (``.outs`` = (hidden states a, tokens a, hidden states b, tokens b))."""
    with torch.no_grad():
        return _decoder_forward([_prep_tensors(prep_a), _prep_tensors(prep_b)], [prep_a["meta"], prep_b["meta"]])


def decode_group(preps, pre, pre_index):
    """One graph node for the prepared decodes ``preps`` (``_AttnLSTMDecoderGroup``): ``pre_index[k]`` = position of pass k in
    the earlier ``decode_pair_launch`` ``pre``, or None (launched now); then each model's second half.  Returns the
    passes' output dicts."""
    flat, metas = [], []
    for p, j in zip(preps, pre_index):
        flat += _prep_tensors(p)
        metas.append(dict(p["meta"], pre=j))
    outs = _AttnLSTMDecoderGroup.apply(*flat, metas, pre)
    return [p["model"].decode_finish(p, outs[2 * k], outs[2 * k + 1]) for k, p in enumerate(preps)]
