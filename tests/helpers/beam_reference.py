"""Host reference of the beam-search decoder (test infrastructure): the selection rule of
``pnmn_attn_lstm_beam`` (include/probnmn_hip.h) in torch on the CPU over a ``state_dict``, built from the pieces
of oracle/seq2seq_oracle.py, in fp64 by default.

    score[b][0] = 0, score[b][k>0] = -inf, last[b][k] = @start@            (step 0 expands one state)
    each step:
      logp[k][v] = log_softmax(logits[k])[v];  logp[k][pad|unk|start] = -inf
      last[b][k] == @end@:  logp[k][:] = -inf, logp[k][@end@] = 0           (a finished hypothesis keeps its score)
      cand[k*V+v] = score[b][k] + logp[k][v]                                (a non-finite cand counts as -inf)
      new beams = the K largest cand, best first; equal cand: smaller k*V+v first
      a slot left without a finite candidate: token @end@, back-pointer 0, score -inf

Two modes: ``beam_search`` searches; ``replay`` follows a given trace (token and back-pointer of every slot at every
step -- the device's own prefixes) and returns the candidate table of every step, so a check against it does not
depend on how a near-tie was decided.  Also here: the synthetic task and the host training loop that give the GPU
tests a model whose hypotheses finish at different steps."""
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle.seq2seq_oracle import (END, PAD, START, UNK, add_sentence_boundary_token_ids, lstm_cell, masked_softmax,
                                   packed_lstm, seq2seq_forward)

NEG_INF = float("-inf")


def encode(sd: Dict[str, torch.Tensor], source_tokens: torch.Tensor):
    """Encoder half of ``seq2seq_forward``: (enc [B,S,H], float mask [B,S], h0 [B,H])."""
    src, _ = add_sentence_boundary_token_ids(source_tokens, source_tokens != PAD, START, END)
    src = src[:, 1:]
    emb = F.embedding(src, sd["_source_embedder.token_embedder_tokens.weight"], padding_idx=PAD)
    src_mask = (src != PAD).long()
    enc = packed_lstm(sd, "_encoder._module.", emb, src_mask)
    h = enc[torch.arange(src.size(0)), src_mask.sum(1) - 1]
    return enc, src_mask.to(enc.dtype), h


def candidates(sd, enc, fmask, h, c, last, score):
    """One decoder step of all B*K hypotheses: (h', c', cand [B, K*V]) from h, c [B,K,H], last [B,K], score [B,K]."""
    B, K, H = h.shape
    S = enc.size(1)
    enc_k = enc.unsqueeze(1).expand(B, K, S, H).reshape(B * K, S, H)
    mask_k = fmask.unsqueeze(1).expand(B, K, S).reshape(B * K, S)
    hf, cf = h.reshape(B * K, H), c.reshape(B * K, H)
    e = F.embedding(last.reshape(-1), sd["_target_embedder.weight"])
    weights = masked_softmax(torch.bmm(enc_k, hf.unsqueeze(-1)).squeeze(-1), mask_k)
    attended = torch.bmm(weights.unsqueeze(1), enc_k).squeeze(1)
    h2, c2 = lstm_cell(torch.cat((attended, e), -1), hf, cf, sd["_decoder_cell.weight_ih"], sd["_decoder_cell.weight_hh"],
                       sd["_decoder_cell.bias_ih"], sd["_decoder_cell.bias_hh"])
    logits = F.linear(h2, sd["_output_projection_layer.weight"], sd["_output_projection_layer.bias"])
    cand = candidate_table(F.log_softmax(logits, dim=-1).view(B, K, -1), last, score)
    return h2.view(B, K, H), c2.view(B, K, H), cand


def candidate_table(logp: torch.Tensor, last: torch.Tensor, score: torch.Tensor) -> torch.Tensor:
    """cand [B, K*V] from logp [B,K,V] (log-softmax over the full vocabulary), last [B,K], score [B,K]."""
    B, K, V = logp.shape
    logp = logp.clone()
    for idx in (PAD, UNK, START):
        if idx < V:
            logp[:, :, idx] = NEG_INF
    finished = last == END
    done = torch.full_like(logp, NEG_INF)
    done[:, :, END] = 0.0
    logp = torch.where(finished.unsqueeze(-1), done, logp)
    cand = score.unsqueeze(-1) + logp
    cand = torch.where(torch.isfinite(cand), cand, torch.full_like(cand, NEG_INF))
    return cand.view(B, K * V)


def select(cand: torch.Tensor, K: int):
    """The K largest of cand [B, K*V], best first, equal values by smaller flat index:
    (token [B,K], back-pointer [B,K], score [B,K], sorted values [B, min(K+1, K*V)])."""
    V = cand.size(1) // K
    neg, order = torch.sort(-cand, dim=1, stable=True)  # ascending -cand, ties in index order
    value, flat = -neg[:, :K], order[:, :K]
    ok = value > NEG_INF
    tok = torch.where(ok, flat % V, torch.full_like(flat, END))
    bp = torch.where(ok, flat // V, torch.zeros_like(flat))
    return tok, bp, value, -neg[:, :K + 1]


def _advance(h2, c2, tok, bp):
    idx = bp.unsqueeze(-1).expand(-1, -1, h2.size(-1))
    return h2.gather(1, idx), c2.gather(1, idx)


def _cast(sd, dtype):
    return {k: v.detach().to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


@torch.no_grad()
def beam_search(sd, source_tokens: torch.Tensor, beam: int, steps: int, dtype=torch.float64):
    """{"tokens" [B,K,T] back-tracked best first, "scores" [B,K], "trace_tokens" / "trace_backptr" / "trace_scores"
    [B,T,K], "margin" [B]: the smallest gap between adjacent ranks 1..K+1 of any step's candidates}."""
    sd = _cast(sd, dtype)
    enc, fmask, h0 = encode(sd, source_tokens)
    B, K = source_tokens.size(0), beam
    h = h0.unsqueeze(1).expand(B, K, -1).contiguous()
    c = torch.zeros_like(h)
    last = torch.full((B, K), START, dtype=torch.long)
    score = torch.full((B, K), NEG_INF, dtype=dtype)
    score[:, 0] = 0.0
    toks, bps, scs = [], [], []
    margin = torch.full((B,), float("inf"), dtype=dtype)
    for _ in range(steps):
        h2, c2, cand = candidates(sd, enc, fmask, h, c, last, score)
        tok, bp, score, ranked = select(cand, K)
        gap = ranked[:, :-1] - ranked[:, 1:]
        gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)  # (-inf) - (-inf): no candidate at all
        margin = torch.minimum(margin, gap.min(1)[0])
        h, c = _advance(h2, c2, tok, bp)
        last = tok
        toks.append(tok), bps.append(bp), scs.append(score)
    trace_tokens, trace_backptr, trace_scores = torch.stack(toks, 1), torch.stack(bps, 1), torch.stack(scs, 1)
    return {"tokens": backtrack(trace_tokens, trace_backptr), "scores": score, "trace_tokens": trace_tokens,
            "trace_backptr": trace_backptr, "trace_scores": trace_scores, "margin": margin}


def backtrack(trace_tokens: torch.Tensor, trace_backptr: torch.Tensor) -> torch.Tensor:
    """[B,T,K] token / back-pointer of every slot at every step -> tokens [B,K,T] of the last step's slots."""
    B, T, K = trace_tokens.shape
    out = torch.zeros(B, K, T, dtype=torch.long)
    cur = torch.arange(K).unsqueeze(0).expand(B, K)
    for t in range(T - 1, -1, -1):
        out[:, :, t] = trace_tokens[:, t].long().gather(1, cur)
        cur = trace_backptr[:, t].long().gather(1, cur)
    return out


@torch.no_grad()
def replay(sd, source_tokens: torch.Tensor, trace_tokens: torch.Tensor, trace_backptr: torch.Tensor,
           dtype=torch.float64) -> List[torch.Tensor]:
    """Follow the given prefixes: per step the candidate table [B, K*V] (in ``dtype``) of the hypotheses the trace
    kept up to that step; a slot's score along the way is the table's own entry for the trace's choice."""
    sd = _cast(sd, dtype)
    enc, fmask, h0 = encode(sd, source_tokens)
    B, T, K = trace_tokens.shape
    h = h0.unsqueeze(1).expand(B, K, -1).contiguous()
    c = torch.zeros_like(h)
    last = torch.full((B, K), START, dtype=torch.long)
    score = torch.full((B, K), NEG_INF, dtype=dtype)
    score[:, 0] = 0.0
    tables = []
    for t in range(T):
        h2, c2, cand = candidates(sd, enc, fmask, h, c, last, score)
        tables.append(cand)
        V = cand.size(1) // K
        tok, bp = trace_tokens[:, t].long(), trace_backptr[:, t].long()
        score = cand.gather(1, bp * V + tok)
        h, c = _advance(h2, c2, tok, bp)
        last = tok
    return tables


# ---- a model whose hypotheses finish ------------------------------------------------------------------------------
def synthetic_task(v_src: int, v_tgt: int, rows: int, generator: torch.Generator):
    """Sources of 3-7 copies of one of ten tokens, which decides the target: 2-6 tokens, token i = a fixed function of
    that token and i.  (source [rows, 7], target [rows, 6]), right-padded with 0."""
    src = torch.zeros(rows, 7, dtype=torch.long)
    tgt = torch.zeros(rows, 6, dtype=torch.long)
    for r in range(rows):
        n = int(torch.randint(3, 8, (1,), generator=generator))
        key = int(torch.randint(0, 10, (1,), generator=generator))
        src[r, :n] = 4 + key % (v_src - 4)
        m = 2 + key % 5
        for i in range(m):
            tgt[r, i] = 4 + (3 * key + 5 * i) % (v_tgt - 4)
    return src, tgt


def train_on_host(sd: Dict[str, torch.Tensor], v_src: int, v_tgt: int, steps: int = 100, rows: int = 64, seed: int = 0,
                  lr: float = 1e-3) -> Dict[str, torch.Tensor]:
    """``steps`` Adam steps of the teacher-forced oracle loss on the synthetic task; returns the trained state_dict."""
    gen = torch.Generator().manual_seed(seed)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    for _ in range(steps):
        src, tgt = synthetic_task(v_src, v_tgt, rows, gen)
        loss = seq2seq_forward(params, src, tgt, "greedy")["loss"].mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return {k: v.detach().clone() for k, v in params.items()}


def first_end_steps(tokens: torch.Tensor) -> torch.Tensor:
    """[..., T] -> index of the first @end@ of every row, T where there is none."""
    T = tokens.size(-1)
    is_end = tokens == END
    return torch.where(is_end.any(-1), is_end.float().argmax(-1), torch.full(tokens.shape[:-1], T, dtype=torch.long))
