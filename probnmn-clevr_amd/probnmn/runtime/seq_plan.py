"""The seq2seq half of a question-coding / joint-training iteration as a static launch plan.

The reference runs ProgramGenerator, QuestionReconstructor and ProgramPrior through AllenNLP's ``SimpleSeq2Seq`` loop under
autograd (probnmn/trainers/question_coding_trainer.py:128-160, joint_training_trainer.py:150-190,
probnmn/modules/seq2seq_base.py:101-276, probnmn/models/program_prior.py:80-155).  ``Seq2SeqBase`` of this package keeps
that call structure with one autograd node per kernel -- right for evaluation, the drop-in graft and the kernel tests, but
at 128 questions per GPU the iteration is then bound by the HOST: ~40 autograd-function applications, ~60 small torch ops
and 20 library GEMM calls per iteration cost 5 of its 6.5 ms (profiles/r06a_b128_host.txt).

For given row counts and token widths the passes are a FIXED sequence of launches over FIXED shapes.  ``Seq2SeqPlan``
therefore builds, once per shape signature,

* a workspace of persistent device buffers (every activation, saved tensor, gradient and scratch block of the passes);
* three forward call lists -- generator (encoder over [unsupervised ; supervised] questions, sampling + teacher-forced
  decoder pair, losses), reconstructor (encoder over [sampled ; ground-truth] programs, teacher-forced decoder, loss),
  prior (LSTM language model over the samples, no gradient) -- and one backward list; an entry is a bound C-ABI entry
  point of libprobnmn_hip.so with its final argument tuple;
* ONE autograd node (``_PlanNode``) whose outputs are the per-row losses and whose backward replays the backward list:
  seq_nll backward -> output-projection data gradient -> the three decoders' backward in one launch -> encoder-output
  gradients -> the two encoders' layers, with every product over all time steps on ``pnmn_gemm`` and EVERY weight
  gradient of a model deferred into one grouped GEMM launch at the end.  Parameter gradients are written straight into
  one flat buffer per model whose slices become the parameters' ``.grad``.

Per iteration the host then replays ~100 prepared calls (a few microseconds each) and touches no torch op in the passes.
Arithmetic is the eager path's kernel for kernel (same recurrent kernels, same losses); the GEMMs are this library's
instead of hipBLASLt's, so results agree with ``Seq2SeqBase.forward`` to fp32 round-off (tests/test_seq_plan_gpu.py)."""
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from probnmn import _hip


#: workgroup slots of the chip for a launch of split-K products (256 CUs, the 64 KB workgroups of pnmn_gemm sit two to a CU)
#: and the shortest chunk (k tiles) a product is cut into
SPLIT_SLOTS = int(os.environ.get("PNMN_PLAN_SPLIT_SLOTS", "512"))
SPLIT_MIN_KTILES = int(os.environ.get("PNMN_PLAN_SPLIT_MIN", "8"))
#: an encoder's two LSTM layers as a wavefront, independent encoder passes in one launch (pnmn_lstm_stack_*); False: a launch
#: per layer with the input projection as a GEMM in between (A/B aid, and what batches too large for the chip fall back to)
USE_STACK = True
#: encoder passes per wavefront launch, forward / generator alone / backward (0: a launch per layer) -- A/B aids; the
#: defaults are what measured best beside the NMN trunk at 128 questions (DESIGN 5 "Round 6")
STACK_FWD_ENCODERS = int(os.environ.get("PNMN_PLAN_FWD_ENC", "2"))
STACK_PG_ENCODER = int(os.environ.get("PNMN_PLAN_PG_ENC", "1"))
STACK_BWD_ENCODERS = int(os.environ.get("PNMN_PLAN_BWD_ENC", "0"))
#: rows of an encoder pass above which its per-layer launches group their row tiles by length (pnmn_length_order,
#: pnmn_lstm_seq_*_ordered): the passes too large for the wavefront launches.  Up to 256 rows a pass runs as a wavefront,
#: whose job record has no room for an order, and its per-layer form (USE_STACK = False) stays the A/B partner of that, call
#: for call.  PNMN_LSTM_LENGTH_ORDER=0 (read when a plan is built) keeps every pass on the unordered calls.
LENGTH_ORDER_ABOVE_ROWS = 256
#: rows of a pass (a decoder's passes: of their model's batch) above which its weight gradients sum over the valid (row, step)
#: pairs only (pnmn_valid_rows,
#: pnmn_gemm_rows): dy is zero at the padded pairs -- the recurrent kernels write zeros there, and past a row's last weighted
#: step the decoders' gradients are 0 x finite -- so about half of the k rows of a 1024-question pass add nothing.  Below it
#: the plan is call for call what it was.  PNMN_GEMM_VALID_PAIRS=0 (read when a plan is built) keeps every product whole.
VALID_PAIRS_ABOVE_ROWS = LENGTH_ORDER_ABOVE_ROWS
#: teacher-forced decoder passes above LENGTH_ORDER_ABOVE_ROWS rows run with their rows grouped by length, one order per pass for
#: forward and backward (pnmn_decoder_last, pnmn_length_order, pnmn_attn_lstm_*_group_ordered): a row tile stops at its longest
#: row's last weighted step.  The sampling pass's forward never is (its lengths are known only as it runs: see
#: SAMPLED_PASS_STOP_ENV); below the threshold the plan is call for call what it was.  PNMN_DECODER_LENGTH_ORDER (read when a
#: plan is built): "0" keeps the unordered calls, "1" selects the ordered ones; unset, this default.
DECODER_LENGTH_ORDER_DEFAULT = "1"
#: the sampling pass above LENGTH_ORDER_ABOVE_ROWS rows: its forward tiles stop once all their rows have emitted @end@
#: (pnmn_attn_lstm_fwd_group_stop, which also counts every row's steps), and its backward runs with the rows grouped by those
#: steps (pnmn_length_order_steps, pnmn_attn_lstm_bwd_group_ordered); the forward itself stays in batch order.  Who builds the
#: plan asks for it (``Seq2SeqPlan(..., sampled_stop=True)``: the trainers do); a plan built without the argument, a pass at or
#: below the threshold, and PNMN_SAMPLED_PASS_STOP=0 keep the calls as they were, call for call.  PNMN_SAMPLED_PASS_STOP (read
#: when a plan is built) overrides the argument either way: "0" off, anything else on.
SAMPLED_PASS_STOP_ENV = "PNMN_SAMPLED_PASS_STOP"
#: the per-model decoder buffers, [flat sequence rows of all the model's passes][width]
DECODER_BUFFERS = (("hs", 256), ("cs", 256), ("cx", 256), ("act", 1024), ("dhs", 256), ("dg", 1024), ("dctx", 256))


class PlanUnsupported(Exception):
    """The models / shapes are outside what the plan is built for: the trainer keeps the eager passes."""


class _Calls(list):
    def add(self, name: str, *args) -> None:
        self.append((getattr(_hip.lib(), name), args, name))

    def add_fn(self, name: str, fn) -> None:
        """A call whose arguments are read when it runs (a dropout mask's seed changes every iteration)."""
        self.append((fn, (), name))

    def run(self) -> None:
        for fn, args, name in self:
            rc = fn(*args)
            if rc:
                _hip.check(rc, name)


def _supported(model) -> bool:
    lstm, cell = model._encoder._module, model._decoder_cell
    return (lstm.hidden_size == 256 and lstm.num_layers == 2 and lstm.input_size == 256 and cell.hidden_size == 256
            and cell.input_size == 512 and model._output_projection_layer.weight.size(0) <= 128
            and model._source_embedder.embedding.weight.size(0) <= 128)


def _dropout_p(lstm) -> float:
    """p of the mask between an encoder's layers in a training-mode pass (0: none)."""
    return float(lstm.dropout) if lstm.num_layers > 1 else 0.0


class _Model:
    """Parameter handles of one Seq2SeqBase in the plan's terms, and its flat gradient buffer."""

    def __init__(self, model, dev):
        self.model = model
        lstm, cell, proj = model._encoder._module, model._decoder_cell, model._output_projection_layer
        self.emb_src, self.emb_tgt = model._source_embedder.embedding.weight, model._target_embedder.weight
        self.lstm, self.cell, self.proj = lstm, cell, proj
        self.params = [self.emb_src] + [getattr(lstm, "%s_l%d" % (n, layer)) for layer in (0, 1)
                                        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] \
            + [self.emb_tgt, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, proj.weight, proj.bias]
        for p in self.params:
            if not p.is_contiguous() or p.device != dev or p.dtype != torch.float32:
                raise PlanUnsupported("parameter layout")
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64
        self.gflat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grads = [self.gflat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, self.params)]
        self.g = {id(p): g for p, g in zip(self.params, self.grads)}
        self.signature = tuple(p.data_ptr() for p in self.params)
        self.derived = model._derived()  # (the same dict as long as the plan is valid: ``Seq2SeqPlan.still_valid``)

    def grad(self, p) -> torch.Tensor:
        return self.g[id(p)]

    def attach(self) -> None:
        for p, g in zip(self.params, self.grads):
            p.grad = g


class _TokenTable(NamedTuple):
    """A per-token projection table, table[v] = bias + emb[v] @ w_ih[:, col0:col0 + 256].T (a first encoder layer's input
    projection, or the embedding half of a decoder cell's): its forward launch and its gradient's come from here."""
    tag: str
    emb: torch.Tensor
    w_ih: torch.Tensor
    col0: int
    b_ih: torch.Tensor
    b_hh: torch.Tensor
    bias: torch.Tensor  # their sum (a derived parameter)
    pad_idx: int        # the embedding row that receives no gradient (-1: none)
    table: torch.Tensor


class _Loss(NamedTuple):
    """A sequence loss over [rows][T] steps of a logits view.  ``pnmn_seq_nll_fwd`` and ``pnmn_seq_nll_bwd`` are both
    generated from this record, so they cannot disagree."""
    logits: torch.Tensor  # from the pass's first row on
    ld: int               # logits elements from one sequence to the next
    target: int           # pointer to the first target token / elements from row to row
    target_stride: int
    mask: int             # same for the tokens whose padding masks the steps
    mask_stride: int
    pad: int
    loss: torch.Tensor
    lse: torch.Tensor
    rows: int
    T: int
    V: int
    eps: float

    def _head(self):
        return (self.logits.data_ptr(), self.ld, self.target, self.target_stride, self.mask, self.mask_stride, self.pad)

    def forward(self, calls: _Calls, stream: int) -> None:
        calls.add("pnmn_seq_nll_fwd", *self._head(), self.loss.data_ptr(), self.lse.data_ptr(), self.rows, self.T, self.V,
                  self.eps, stream)

    def backward(self, calls: _Calls, dloss: torch.Tensor, dlogits: torch.Tensor, stream: int) -> None:
        calls.add("pnmn_seq_nll_bwd", *self._head(), self.lse.data_ptr(), dloss.data_ptr(), dlogits.data_ptr(), self.ld,
                  self.rows, self.T, self.V, self.eps, stream)


@dataclass
class _DecoderPass:
    """One pass of a model's decoder: ``rows`` sequences of ``T`` steps attending to ``S`` source positions."""
    tag: str
    rows: int
    T: int
    S: int
    row0: int             # first flat row in the model's decoder buffers
    enc_row0: int         # first row in the model's encoder batch
    tokens: torch.Tensor  # step tokens: a teacher-forced [@start@, ..., @end@] matrix, or the tokens the pass samples
    shift: int            # step t reads tokens[t - shift] (1: its own sample of the step before, @start@ at t = 0)
    trimmed: Optional[torch.Tensor]  # the sampling pass only: its samples cut at @end@ (what masks its loss)
    v: Dict[str, torch.Tensor]       # [rows][T][.] views of DECODER_BUFFERS, and the pass's own probs / dscore / weights
    loss: _Loss
    order: Optional[torch.Tensor] = None       # rows grouped by length (``_decoder_order``): pnmn_length_order's lists, or None
    tile_steps: Optional[torch.Tensor] = None


@dataclass
class _DecoderSet:
    """A model's decoder: its passes share the parameters, the token table and flat buffers over all their rows."""
    tag: str
    mm: _Model
    enc: Dict
    table: _TokenTable
    flat: Dict[str, torch.Tensor]
    logits: torch.Tensor
    dlogits: torch.Tensor
    passes: List[_DecoderPass]


class _EncoderPass(NamedTuple):
    """What ``_encoder_prepare`` builds an encoder pass from."""
    tag: str
    mm: Optional[_Model]         # None: the prior (no gradients)
    embedding: torch.nn.Embedding
    tokens: torch.Tensor
    width: int
    rows: int
    drop_first: bool = True      # drop the first of [@start@, tokens, @end@]
    want_last: bool = True       # masked outputs and last states (what a decoder attends to / starts from)
    p: float = 0.0               # dropout between the layers


class Seq2SeqPlan:
    """See the module docstring.  ``n`` unsupervised (sampled) rows, ``m`` supervised rows, both > 0; ``tq`` / ``tp``: the
    widths of the batch's question / program matrices.  ``sampled_stop``: see SAMPLED_PASS_STOP_ENV."""

    def __init__(self, pg, qr, prior, dev: torch.device, n: int, m: int, tq: int, tp: int, sampled_stop: bool = False):
        if not (_supported(pg) and _supported(qr)) or n <= 0 or m <= 0:
            raise PlanUnsupported("model shapes")
        pl = prior._encoder._module
        if pl.hidden_size != 256 or pl.num_layers != 2 or pl.input_size != 256:
            raise PlanUnsupported("prior shapes")
        if pl.training and _dropout_p(pl) > 0:  # (the trainers keep the prior in eval mode: its pass drops nothing)
            raise PlanUnsupported("prior in training mode with dropout")
        self.dev, self.n, self.m, self.tq, self.tp = dev, n, m, tq, tp
        self.stream = _hip.stream_ptr(dev)
        self.pg, self.qr, self.prior = _Model(pg, dev), _Model(qr, dev), prior
        # the masks between the encoders' layers (the plan serves training-mode passes only)
        self.drop_p = (_dropout_p(pg._encoder._module), _dropout_p(qr._encoder._module))
        self.B, self.D = n + m, pg._max_decoding_steps
        if _hip.decoder_workspace_bytes([n, m], False) <= 0 or _hip.decoder_workspace_bytes([self.B], False) <= 0 \
                or int(_hip.lib().pnmn_lstm_seq_workspace_bytes(self.B, 0)) <= 0:
            raise PlanUnsupported("batch does not fit the multi-CU recurrent kernels in one launch")
        self._bufs: Dict[str, torch.Tensor] = {}
        self._keep: List = []  # numpy records the call tuples point into
        self._keep_args: List[np.ndarray] = []  # plain host arrays the call tuples point into (per-problem / per-segment arguments)
        self._valid_lists: List = []  # segments of the (row, step) lists the weight gradients sum over (``_valid_list``)
        self.valid_pairs = os.environ.get("PNMN_GEMM_VALID_PAIRS", "1") != "0"
        self.decoder_order = os.environ.get("PNMN_DECODER_LENGTH_ORDER", DECODER_LENGTH_ORDER_DEFAULT) != "0"
        self.sampled_stop = os.environ[SAMPLED_PASS_STOP_ENV] != "0" if SAMPLED_PASS_STOP_ENV in os.environ else bool(sampled_stop)
        self.anchor = torch.zeros((), device=dev, requires_grad=True)
        self.fwd_pg_enc, self.fwd_pg, self.fwd_pg_finish, self.fwd_qr, self.fwd_prior = (_Calls() for _ in range(5))
        self.bwd_a, self.bwd_b = _Calls(), _Calls()  # the decoders' backward / the encoders' and every parameter gradient
        self._build()

    # ---- workspace ---------------------------------------------------------------------------------------------------------
    def buf(self, name: str, *shape, dtype=torch.float32, zero: bool = False) -> torch.Tensor:
        if name in self._bufs:
            raise KeyError(name)
        t = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.dev)
        self._bufs[name] = t
        return t

    def bytes_buf(self, name: str, nbytes: int, zero: bool = False) -> torch.Tensor:
        return self.buf(name, max(int(nbytes), 16), dtype=torch.uint8, zero=zero)

    def __getitem__(self, name: str) -> torch.Tensor:
        return self._bufs[name]

    # ---- pieces ------------------------------------------------------------------------------------------------------------
    def _gemm(self, calls: _Calls, name: str, descs) -> None:
        """descs: list of dicts(a, b, c, M, N, K, lda, ldb, ldc, ta, tb, acc, bias, split, shift_t, h0, ld_h0, colsum, colsum2,
        valid); valid = (list, count) of ``_valid_list``: the k rows the product sums over (ta = 1 products only)."""
        lib = _hip.lib()
        for lo in range(0, len(descs), _hip.GEMM_MAX):
            part = descs[lo:lo + _hip.GEMM_MAX]
            rec = np.zeros(len(part), _hip.GEMM_DESC)
            # split-K of the problems that ask for it ("auto"), chosen for the LAUNCH: chunks of one common length (in 32-wide
            # k tiles) for every problem of the launch, so that the launch is a few ROUNDS of equal workgroups over the chip's
            # 512 slots (two 64 KB workgroups per CU) -- a chunk count per problem that merely filled the chip once left the CUs
            # holding two long chunks running after the others had finished (eight weight gradients of 512-question passes:
            # 78 TFLOP/s).  The length is the one with the least modelled time among 8 .. 128 k tiles: rounds x chunk length,
            # a started last round counting 0.6 (its workgroups have their CU to themselves), plus the partial tiles' trip
            # through memory (64 KB written and read back per chunk: ~4 k tiles' worth of a workgroup's time).  2114 equal
            # chunks are 4.13 rounds -- five in practice; 2040 are four.
            tiles = [((d["M"] + 127) // 128) * ((d["N"] + 127) // 128) for d in part]
            ktiles = [(d["K"] + 31) // 32 for d in part]
            auto = [i for i, d in enumerate(part) if d.get("split") == "auto"]
            fixed_units = sum(t for i, t in enumerate(tiles) if i not in auto)
            chunk_len, best = SPLIT_MIN_KTILES, None
            for cand in range(SPLIT_MIN_KTILES, 129):
                splits = [max(1, min(-(-ktiles[i] // cand), 64)) for i in auto]
                units = fixed_units + sum(tiles[i] * sp for i, sp in zip(auto, splits))
                longest = max([-(-ktiles[i] // sp) for i, sp in zip(auto, splits)] + [ktiles[i] for i in range(len(part)) if i not in auto] + [1])
                rounds = units // SPLIT_SLOTS + (0.6 if units % SPLIT_SLOTS else 0.0)
                cost = rounds * longest + 4.0 * sum(tiles[i] * sp for i, sp in zip(auto, splits) if sp > 1) / SPLIT_SLOTS
                if best is None or cost < best:
                    chunk_len, best = cand, cost
            for i, d in enumerate(part):
                r = rec[i]
                r["a"], r["b"], r["c"] = d["a"], d["b"], d["c"]
                r["lda"], r["ldb"], r["ldc"] = d["lda"], d["ldb"], d["ldc"]
                r["M"], r["N"], r["K"] = d["M"], d["N"], d["K"]
                r["flags"] = (_hip.GEMM_A_T if d.get("ta") else 0) | (_hip.GEMM_B_T if d.get("tb") else 0) | (_hip.GEMM_ACC if d.get("acc") else 0)
                r["bias"] = d.get("bias", 0)
                split = d.get("split", 1)
                if split == "auto":
                    split = max(1, min(-(-ktiles[i] // chunk_len), 64))
                r["split_k"] = split
                if split > 1:
                    ws = self.bytes_buf("%s.ws%d" % (name, lo + i), lib.pnmn_gemm_workspace_bytes(d["M"], d["N"], split), zero=True)
                    r["workspace"] = ws.data_ptr()
                r["shift_t"], r["shift_h0"], r["ld_h0"] = d.get("shift_t", 0), d.get("h0", 0), d.get("ld_h0", 0)
                r["colsum"], r["colsum2"] = d.get("colsum", 0), d.get("colsum2", 0)
            self._keep.append(rec)
            if any(d.get("valid") for d in part):
                # (the chunk counts above are those of the full K: the list's length is known to the device alone)
                lists = np.array([d.get("valid", (0, 0)) for d in part], np.uint64).T.copy()
                self._keep_args.append(lists)
                calls.add("pnmn_gemm_rows", rec.ctypes.data, len(rec), lists[0].ctypes.data, lists[1].ctypes.data, 0, self.stream)
            else:
                calls.add("pnmn_gemm_cus", rec.ctypes.data, len(rec), 0, self.stream)

    def _valid_list(self, name: str, segments) -> tuple:
        """The list of valid (row, step) pairs of passes stored one behind the other, for the weight gradients that contract
        them.  segments: (last, mask tokens, mask row stride, pad, rows, T) per pass -- `last` (an encoder's) or the tokens that
        mask the pass's loss (a decoder's), the other 0.  Returns (list, count) for a ``_gemm`` description; the lists of a
        backward are built by ``_valid_list_calls``."""
        rows = self.buf(name + ".rows", sum(r * T for _, _, _, _, r, T in segments), 2, dtype=torch.int32)
        count = self.buf(name + ".count", 1, dtype=torch.int32, zero=True)
        self._valid_lists.append((rows.data_ptr(), count.data_ptr(), segments))
        return rows.data_ptr(), count.data_ptr()

    def _valid_list_calls(self, calls: _Calls) -> None:
        """One launch for up to eight segments of the lists asked for so far (a workgroup per list)."""
        group: List = []

        def flush():
            if group:
                arg = np.array(group, np.int64).T.copy()  # rows: last, mask, stride, pad, rows, T, list, count
                pad, rows, T = (arg[k].astype(np.int32) for k in (3, 4, 5))
                self._keep_args += [arg, pad, rows, T]
                calls.add("pnmn_valid_rows", arg[0].ctypes.data, arg[1].ctypes.data, arg[2].ctypes.data, pad.ctypes.data, rows.ctypes.data,
                          T.ctypes.data, arg[6].ctypes.data, arg[7].ctypes.data, len(group), self.stream)
                del group[:]
        for lst, count, segments in self._valid_lists:
            if len(group) + len(segments) > 8:
                flush()
            group += [seg + (lst, count) for seg in segments]
        flush()
        self._valid_lists = []

    def _table_forward(self, calls: _Calls, t: _TokenTable) -> None:
        calls.add("pnmn_token_table_fwd", t.emb.data_ptr(), t.w_ih.data_ptr() + 4 * t.col0, t.w_ih.stride(0), t.bias.data_ptr(),
                  t.emb.size(0), 256, 1024, t.table.data_ptr(), self.stream)

    def _table_backward(self, calls: _Calls, t: _TokenTable, mm: _Model, start: int, uses) -> None:
        """The gradients a token table passes on.  uses: (workspace name, dgates [rows][T][1024], tokens, shift) per pass that
        read it -- step t of a row read table[tokens[t - shift]], table[start] before its first token."""
        V, g = t.emb.size(0), mm.grad
        dtable = self.buf(t.tag + ".dtable", V, 1024)
        for k, (ws_name, dg, tokens, shift) in enumerate(uses):
            rows, T = dg.shape[:2]
            ews = self.bytes_buf(ws_name, _hip.lib().pnmn_embedding_grad_workspace_bytes(rows, T, V))
            calls.add("pnmn_embedding_grad", dg.data_ptr(), tokens.data_ptr(), tokens.stride(0), rows, T, 1024, V, shift, start, -1,
                      1 if k else 0, dtable.data_ptr(), ews.data_ptr(), self.stream)
        ld = t.w_ih.stride(0)  # (the gradient's: 0 where its rows are just the table's 256 columns)
        calls.add("pnmn_token_table_bwd", dtable.data_ptr(), t.emb.data_ptr(), t.w_ih.data_ptr() + 4 * t.col0, ld, V, 256, 1024, t.pad_idx,
                  g(t.emb).data_ptr(), g(t.w_ih).data_ptr() + 4 * t.col0, ld if ld != 256 else 0, g(t.b_ih).data_ptr(),
                  g(t.b_hh).data_ptr(), self.stream)

    def _encoder_prepare(self, calls: _Calls, ep: _EncoderPass) -> Dict:
        """Buffers of one encoder pass + what precedes its recurrence: token_prep and the per-token table of layer 1.  ``p`` > 0:
        dropout between the layers -- "hsd" holds layer 1's output after the mask (layer 2's input), and every call that
        applies the mask finds this iteration's seed in "seed" / the records listed in "drop_recs" (``_set_dropout``)."""
        model, derived = (ep.mm.model, ep.mm.derived) if ep.mm is not None else (self.prior, self.prior._derived())
        tag, rows, lstm, emb, f = ep.tag, ep.rows, model._encoder._module, ep.embedding.weight, self.buf
        T, V = ep.width + 2 - int(ep.drop_first), emb.size(0)
        e = dict(tag=tag, mm=ep.mm, derived=derived, lstm=lstm, T=T, rows=rows, want_last=ep.want_last,
                 src=f(tag + ".src", rows, T, dtype=torch.long), fmask=f(tag + ".fmask", rows, T), last=f(tag + ".last", rows, dtype=torch.int32),
                 table=f(tag + ".table", V, 1024), hs1=f(tag + ".hs1", rows, T, 256), cs1=f(tag + ".cs1", rows, T, 256),
                 act1=f(tag + ".act1", rows, T, 1024), hs2=f(tag + ".hs2", rows, T, 256), cs2=f(tag + ".cs2", rows, T, 256),
                 act2=f(tag + ".act2", rows, T, 1024), p=ep.p, seed=0, row_offset=0, drop_recs=[])
        e["tab"] = _TokenTable(tag, emb, lstm.weight_ih_l0, 0, lstm.bias_ih_l0, lstm.bias_hh_l0, derived["l0.b"],
                               -1 if ep.embedding.padding_idx is None else ep.embedding.padding_idx, e["table"])
        if ep.p > 0:
            e["hsd"] = f(tag + ".hsd", rows, T, 256)
        calls.add("pnmn_token_prep", ep.tokens.data_ptr(), ep.tokens.stride(0), rows, ep.width, model._pad_index, model._start_index,
                  model._end_index, int(ep.drop_first), e["src"].data_ptr(), e["fmask"].data_ptr(), e["last"].data_ptr(), self.stream)
        if rows > LENGTH_ORDER_ABOVE_ROWS and os.environ.get("PNMN_LSTM_LENGTH_ORDER", "1") != "0":
            # the pass's rows grouped by length: one order for both layers, forward and backward
            e["order"], e["tile_steps"] = f(tag + ".order", rows, dtype=torch.int32), f(tag + ".tile_steps", (rows + 15) // 16, dtype=torch.int32)
            calls.add("pnmn_length_order", e["last"].data_ptr(), rows, T, e["order"].data_ptr(), e["tile_steps"].data_ptr(), self.stream)
        self._table_forward(calls, e["tab"])
        if ep.want_last:
            e["enc"], e["h"] = f(tag + ".enc", rows, T, 256), f(tag + ".h", rows, 256)
        return e

    def _stack_jobs(self, encs: List[Dict], backward: bool) -> np.ndarray:
        jobs = np.zeros(2 * len(encs), _hip.LSTM_STACK_JOB)
        for k, e in enumerate(encs):
            d = e["derived"]
            a, b = jobs[2 * k], jobs[2 * k + 1]
            if not backward:
                a["xp"], a["tokens"], a["token_stride"], a["w_hh"] = e["table"].data_ptr(), e["src"].data_ptr(), e["src"].stride(0), d["l0.hh"].data_ptr()
                a["hs"], a["cs"], a["act"], a["dep"] = e["hs1"].data_ptr(), e["cs1"].data_ptr(), e["act1"].data_ptr(), -1
                b["w_hh"], b["w_ih"], b["bias"] = d["l1.hh"].data_ptr(), d["l1.ih"].data_ptr(), d["l1.b"].data_ptr()
                b["hs"], b["cs"], b["act"], b["dep"] = e["hs2"].data_ptr(), e["cs2"].data_ptr(), e["act2"].data_ptr(), 2 * k
            else:  # layer 2 first (top), layer 1 below it
                a["dhs"], a["act"], a["cs"], a["w_hh"], a["dgates"], a["dep"] = (e["dhs2"].data_ptr(), e["act2"].data_ptr(), e["cs2"].data_ptr(),
                                                                                 d["l1.hhT"].data_ptr(), e["dg2"].data_ptr(), -1)
                b["act"], b["cs"], b["w_hh"], b["w_ih"], b["dgates"], b["dep"] = (e["act1"].data_ptr(), e["cs1"].data_ptr(), d["l0.hhT"].data_ptr(),
                                                                                 d["l1.ihT"].data_ptr(), e["dg1"].data_ptr(), 2 * k)
            for j in (a, b):
                j["B"], j["T"] = e["rows"], e["T"]
        return jobs

    def _stack_launches(self, calls: _Calls, name: str, encs: List[Dict], backward: bool, most: Optional[int] = None) -> List[Dict]:
        """The recurrences of several encoder passes as wavefront launches: all of them in one launch when their workgroups
        fit the chip together, else greedily as many as fit per launch; returns the encoders no stack launch takes (their
        layers go out one by one)."""
        lib, left, group = _hip.lib(), [], []
        if most is None:
            most = STACK_BWD_ENCODERS if backward else STACK_FWD_ENCODERS
        use = USE_STACK and most > 0 and all("l1.ih" in e["derived"] for e in encs)

        def flush():
            if not group:
                return
            jobs = self._stack_jobs(group, backward)
            ws = self.bytes_buf("%s.stack_ws%d" % (name, len(self._keep)), lib.pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, len(jobs), int(backward)))
            self._keep.append(jobs)
            if any(e["p"] > 0 for e in group):
                # dropout descriptors: on layer 1's job (forward: the FIRST job writes hsd; backward: the BELOW job masks the
                # gradient from above); seeds are written into them per iteration
                drops = np.zeros(len(jobs), _hip.LSTM_DROPOUT_DESC)
                for k, e in enumerate(group):
                    if e["p"] > 0:
                        i = 2 * k + int(backward)
                        drops[i]["p"] = e["p"]
                        if not backward:
                            drops[i]["hsd"] = e["hsd"].data_ptr()
                        e["drop_recs"].append((drops, i))
                self._keep.append(drops)
                calls.add("pnmn_lstm_stack_bwd_dropout" if backward else "pnmn_lstm_stack_fwd_dropout", jobs.ctypes.data, drops.ctypes.data,
                          len(jobs), ws.data_ptr(), self.stream)
            else:
                calls.add("pnmn_lstm_stack_bwd" if backward else "pnmn_lstm_stack_fwd", jobs.ctypes.data, len(jobs), ws.data_ptr(), self.stream)
            del group[:]

        for e in encs:
            if not use:
                left.append(e)
                continue
            trial = self._stack_jobs(group + [e], backward)
            if len(group) < most and 2 * (len(group) + 1) <= _hip.LSTM_STACK_JOBS and int(lib.pnmn_lstm_stack_workspace_bytes(trial.ctypes.data, len(trial), int(backward))) > 0:
                group.append(e)
                continue
            flush()
            alone = self._stack_jobs([e], backward)
            if int(lib.pnmn_lstm_stack_workspace_bytes(alone.ctypes.data, 2, int(backward))) > 0:
                group.append(e)
            else:
                left.append(e)
        flush()
        return left

    def _dropout_call(self, calls: _Calls, e: Dict, src: torch.Tensor, dst: torch.Tensor) -> None:
        """pnmn_lstm_dropout over one of the encoder's [rows][T][256] tensors with the iteration's seed (y == x allowed)."""
        fn, st = _hip.lib().pnmn_lstm_dropout, self.stream
        x, y, rows, T, p = src.data_ptr(), dst.data_ptr(), e["rows"], e["T"], e["p"]
        calls.add_fn("pnmn_lstm_dropout", lambda: fn(x, y, rows, T, 256, p, e["seed"], e["row_offset"], st))

    def _set_dropout(self, e: Dict, seed: int, row_offset: int) -> None:
        e["seed"], e["row_offset"] = seed, row_offset
        for rec, i in e["drop_recs"]:
            rec[i]["seed"], rec[i]["row_offset"] = seed, row_offset

    def _encoders_fwd(self, calls: _Calls, name: str, encs: List[Dict], most: Optional[int] = None) -> None:
        lib, st = _hip.lib(), self.stream
        for e in self._stack_launches(calls, name, encs, False, most):
            d, lstm, rows, T = e["derived"], e["lstm"], e["rows"], e["T"]
            xp2 = self.buf(e["tag"] + ".xp2", rows, T, 1024)
            ws = self.bytes_buf(e["tag"] + ".lstm_ws", lib.pnmn_lstm_seq_workspace_bytes(rows, 0))
            fwd, ordered = ("pnmn_lstm_seq_fwd_ordered", (e["order"].data_ptr(), e["tile_steps"].data_ptr())) if "order" in e else ("pnmn_lstm_seq_fwd", ())
            calls.add(fwd, e["table"].data_ptr(), e["src"].data_ptr(), e["src"].stride(0), d["l0.hh"].data_ptr(),
                      e["hs1"].data_ptr(), e["cs1"].data_ptr(), e["act1"].data_ptr(), rows, T, 256, *ordered, ws.data_ptr(), st)
            x2 = e["hs1"]
            if e["p"] > 0:
                self._dropout_call(calls, e, e["hs1"], e["hsd"])
                x2 = e["hsd"]
            self._gemm(calls, e["tag"] + ".xp2g", [dict(a=x2.data_ptr(), b=lstm.weight_ih_l1.data_ptr(), c=xp2.data_ptr(), M=rows * T,
                                                        N=1024, K=256, lda=256, ldb=256, ldc=1024, tb=1, bias=d["l1.b"].data_ptr())])
            calls.add(fwd, xp2.data_ptr(), None, 0, d["l1.hh"].data_ptr(), e["hs2"].data_ptr(), e["cs2"].data_ptr(),
                      e["act2"].data_ptr(), rows, T, 256, *ordered, ws.data_ptr(), st)
        for e in encs:
            if e["want_last"]:
                calls.add("pnmn_mask_last_fwd", e["hs2"].data_ptr(), e["fmask"].data_ptr(), e["last"].data_ptr(), e["rows"], e["T"], 256,
                          e["enc"].data_ptr(), e["h"].data_ptr(), st)

    def _encoders_bwd(self, calls: _Calls, name: str, encs: List[Dict]) -> None:
        """The encoders' backward CHAIN.  encs: encoder dicts with "denc" / "dh" set (gradients of the masked outputs and of
        the last states)."""
        lib, st = _hip.lib(), self.stream
        f = self.buf
        for e in encs:
            tag, rows, T = e["tag"], e["rows"], e["T"]
            e["dhs2"], e["dg2"], e["dg1"] = f(tag + ".dhs2", rows, T, 256), f(tag + ".dg2", rows, T, 1024), f(tag + ".dg1", rows, T, 1024)
            calls.add("pnmn_mask_last_bwd", e["denc"].data_ptr(), e["dh"].data_ptr(), e["fmask"].data_ptr(), e["last"].data_ptr(), rows, T, 256,
                      e["dhs2"].data_ptr(), st)
        for e in self._stack_launches(calls, name, encs, True):
            d, lstm, tag, rows, T = e["derived"], e["lstm"], e["tag"], e["rows"], e["T"]
            dhs1 = f(tag + ".dhs1", rows, T, 256)
            ws = self.bytes_buf(tag + ".lstm_bws", lib.pnmn_lstm_seq_workspace_bytes(rows, 1))
            bwd, ordered = ("pnmn_lstm_seq_bwd_ordered", (e["order"].data_ptr(), e["tile_steps"].data_ptr())) if "order" in e else ("pnmn_lstm_seq_bwd", ())
            calls.add(bwd, e["dhs2"].data_ptr(), e["act2"].data_ptr(), e["cs2"].data_ptr(), d["l1.hhT"].data_ptr(),
                      e["dg2"].data_ptr(), rows, T, 256, *ordered, ws.data_ptr(), st)
            self._gemm(calls, tag + ".dx", [dict(a=e["dg2"].data_ptr(), b=lstm.weight_ih_l1.data_ptr(), c=dhs1.data_ptr(), M=rows * T, N=256,
                                                 K=1024, lda=1024, ldb=256, ldc=256, split="auto")])
            if e["p"] > 0:
                self._dropout_call(calls, e, dhs1, dhs1)
            calls.add(bwd, dhs1.data_ptr(), e["act1"].data_ptr(), e["cs1"].data_ptr(), d["l0.hhT"].data_ptr(),
                      e["dg1"].data_ptr(), rows, T, 256, *ordered, ws.data_ptr(), st)

    def _encoders_param_grads(self, calls: _Calls, deferred: List, encs: List[Dict]) -> None:
        """The encoders' parameter gradients from what the chain left behind (dgates of both layers): the table's rows and the
        bias sums as launches, everything GEMM-shaped appended to ``deferred``."""
        for e in encs:
            mm, lstm, rows, T = e["mm"], e["lstm"], e["rows"], e["T"]
            dg1, dg2, g = e["dg1"], e["dg2"], mm.grad
            self._table_backward(calls, e["tab"], mm, 0, [(e["tag"] + ".emb_ws", dg1, e["src"], 0)])
            K = rows * T
            # (one list for the pass's three products: both layers' dgates are zero from the row's length on)
            valid = dict(valid=self._valid_list(e["tag"] + ".valid", [(e["last"].data_ptr(), 0, 0, 0, rows, T)])) \
                if self.valid_pairs and rows > VALID_PAIRS_ABOVE_ROWS else {}
            # (layer 2's bias gradients = the column sums of dgates2: the weight-gradient product that reads dgates2 as its
            # transposed operand adds them up on the way -- pnmn_gemm_desc.colsum)
            deferred += [
                dict(a=dg2.data_ptr(), b=e["hs2"].data_ptr(), c=g(lstm.weight_hh_l1).data_ptr(), M=1024, N=256, K=K, lda=1024, ldb=256,
                     ldc=256, ta=1, split="auto", shift_t=T, colsum=g(lstm.bias_ih_l1).data_ptr(), colsum2=g(lstm.bias_hh_l1).data_ptr(), **valid),
                dict(a=dg2.data_ptr(), b=(e["hsd"] if e["p"] > 0 else e["hs1"]).data_ptr(), c=g(lstm.weight_ih_l1).data_ptr(), M=1024,
                     N=256, K=K, lda=1024, ldb=256, ldc=256, ta=1, split="auto", **valid),  # (layer 2's input: after the mask)
                dict(a=dg1.data_ptr(), b=e["hs1"].data_ptr(), c=g(lstm.weight_hh_l0).data_ptr(), M=1024, N=256, K=K, lda=1024, ldb=256,
                     ldc=256, ta=1, split="auto", shift_t=T, **valid),
            ]

    def _decoder_set(self, tag: str, mm: _Model, enc: Dict, passes) -> _DecoderSet:
        """A model's decoder buffers and its passes.  passes: (tag, loss-name suffix, rows, T, tokens, trimmed) in the
        order of their rows in the encoder's batch, which is their order in the flat buffers."""
        f, S, V = self.buf, enc["T"], mm.proj.weight.size(0)
        R = sum(rows * T for _, _, rows, T, _, _ in passes)
        # (the table's weight: columns [256, 512) of W_ih, the embedding half of cat(attended, embedded))
        table = _TokenTable(tag + ".d", mm.emb_tgt, mm.cell.weight_ih, 256, mm.cell.bias_ih, mm.cell.bias_hh, mm.derived["d.b"], -1,
                            f(tag + ".d.table", V, 1024))
        dec = _DecoderSet(tag, mm, enc, table, {k: f("%s.d.%s" % (tag, k), R, w) for k, w in DECODER_BUFFERS},
                          f(tag + ".logits", R, V), f(tag + ".dlogits", R, V), [])
        row0 = enc_row0 = 0
        for ptag, suffix, rows, T, tokens, trimmed in passes:
            v = {k: dec.flat[k][row0:row0 + rows * T].view(rows, T, w) for k, w in DECODER_BUFFERS}
            for k in ("probs", "dscore", "weights"):
                v[k] = f("%s.%s" % (ptag, k), rows, T, S)
            # a sampling pass is scored on its own tokens, masked by their trimmed copy, a teacher-forced pass on its
            # matrix from the token after @start@ on
            target = tokens.data_ptr() + (0 if trimmed is not None else 8)
            loss = _Loss(dec.logits[row0:], T * V, target, tokens.stride(0), target if trimmed is None else trimmed.data_ptr(),
                         tokens.stride(0), mm.model._pad_index, f("%s.loss%s" % (tag, suffix), rows), f("%s.lse%s" % (tag, suffix), rows, T),
                         rows, T, V, 1e-13 if trimmed is None else 1e-12)
            dec.passes.append(_DecoderPass(ptag, rows, T, S, row0, enc_row0, tokens, int(trimmed is not None), trimmed, v, loss))
            row0, enc_row0 = row0 + rows * T, enc_row0 + rows
        return dec

    def _decoder_fwd_job(self, j, dec: _DecoderSet, p: _DecoderPass) -> None:
        """A pass's ``DECODER_FWD_JOB``; its step tokens are read from the teacher-forced matrix, or drawn by the sampler and written."""
        e, r0, mm = dec.enc, p.enc_row0, dec.mm
        j["etable"], j["enc"], j["mask"], j["h0"] = dec.table.table.data_ptr(), e["enc"][r0:].data_ptr(), e["fmask"][r0:].data_ptr(), e["h"][r0:].data_ptr()
        j["w_c"], j["w_hh"] = mm.derived["d.c"].data_ptr(), mm.derived["d.hh"].data_ptr()
        j["hs"], j["cs"], j["act"], j["ctx"], j["probs"] = (p.v[k].data_ptr() for k in ("hs", "cs", "act", "cx", "probs"))
        j["B"], j["T"], j["S"], j["start_index"] = p.rows, p.T, p.S, mm.model._start_index
        if p.trimmed is None:
            j["in_tokens"], j["in_token_stride"] = p.tokens.data_ptr(), p.tokens.stride(0)
        else:
            j["w_p"], j["b_p"], j["tokens"], j["V"], j["sample"] = mm.proj.weight.data_ptr(), mm.proj.bias.data_ptr(), p.tokens.data_ptr(), mm.proj.weight.size(0), 1
            j["pad_index"], j["unk_index"] = mm.model._pad_index, mm.model._unk_index

    def _decoder_order(self, calls: _Calls, p: _DecoderPass) -> None:
        """A large teacher-forced pass's rows grouped by length: its steps are the ones its loss weights (the mask tokens of
        ``p.loss``, in place when this runs), one order for forward and backward."""
        if not self.decoder_order or p.trimmed is not None or p.rows <= LENGTH_ORDER_ABOVE_ROWS:
            return
        f, i32 = self.buf, torch.int32
        last = f(p.tag + ".last", p.rows, dtype=i32)
        p.order, p.tile_steps = f(p.tag + ".order", p.rows, dtype=i32), f(p.tag + ".tile_steps", (p.rows + 15) // 16, dtype=i32)
        calls.add("pnmn_decoder_last", p.loss.mask, p.loss.mask_stride, p.loss.pad, p.rows, p.T, last.data_ptr(), self.stream)
        calls.add("pnmn_length_order", last.data_ptr(), p.rows, p.T, p.order.data_ptr(), p.tile_steps.data_ptr(), self.stream)

    def _order_lists(self, passes: List[_DecoderPass]):
        """() when no pass has an order, else the two host arrays of device pointers the ``_ordered`` calls take."""
        if all(p.order is None for p in passes):
            return ()
        lists = np.array([[0 if t is None else t.data_ptr() for t in col] for col in
                          ([p.order for p in passes], [p.tile_steps for p in passes])], np.uint64)
        self._keep_args.append(lists)
        return lists[0].ctypes.data, lists[1].ctypes.data

    def _decoder_forward(self, calls: _Calls, dec: _DecoderSet, source: torch.Tensor, tgt: torch.Tensor, ws_name: str) -> np.ndarray:
        """[@start@, source row, @end@] as the teacher-forced matrix ``tgt``, the token table, and the set's passes in one launch;
        returns the launch's job records, for the caller to keep."""
        model, rows = dec.mm.model, [p.rows for p in dec.passes]
        calls.add("pnmn_token_prep", source.data_ptr(), source.stride(0), source.size(0), source.size(1), model._pad_index, model._start_index,
                  model._end_index, 0, tgt.data_ptr(), None, None, self.stream)
        for p in dec.passes:
            self._decoder_order(calls, p)
        self._table_forward(calls, dec.table)
        jobs = np.zeros(len(dec.passes), _hip.DECODER_FWD_JOB)
        for j, p in zip(jobs, dec.passes):
            self._decoder_fwd_job(j, dec, p)
        ws = self.bytes_buf(ws_name, _hip.decoder_workspace_bytes(rows, False))
        ordered = self._order_lists(dec.passes)
        stopping = [p for p in dec.passes if self.sampled_stop and p.trimmed is not None and p.rows > LENGTH_ORDER_ABOVE_ROWS]
        if not stopping:
            calls.add("pnmn_attn_lstm_fwd_group_ordered" if ordered else "pnmn_attn_lstm_fwd_group", jobs.ctypes.data,
                      None, 0, None, None, None, 0, 0,  # (no filters, no automaton)
                      len(jobs), 256, *ordered, ws.data_ptr(), self.stream)
            return jobs
        # a large sampling pass: its tiles stop at their rows' @end@ and count the rows' steps; its BACKWARD then runs with the
        # rows grouped by those steps (the order is built behind the forward, which stays in batch order)
        i32 = torch.int32
        steps = {p.tag: self.buf(p.tag + ".steps", p.rows, dtype=i32) for p in stopping}
        outs = np.array([steps[p.tag].data_ptr() if p.tag in steps else 0 for p in dec.passes], np.uint64)
        self._keep_args.append(outs)
        calls.add("pnmn_attn_lstm_fwd_group_stop", jobs.ctypes.data, None, model._end_index, None, None, None, 0, 0,
                  len(jobs), 256, *(ordered or (None, None)), outs.ctypes.data, ws.data_ptr(), self.stream)
        for p in stopping:
            p.order, p.tile_steps = self.buf(p.tag + ".order", p.rows, dtype=i32), self.buf(p.tag + ".tile_steps", (p.rows + 15) // 16, dtype=i32)
            calls.add("pnmn_length_order_steps", steps[p.tag].data_ptr(), p.rows, p.T, p.order.data_ptr(), p.tile_steps.data_ptr(), self.stream)
        return jobs

    def _decoder_losses(self, calls: _Calls, dec: _DecoderSet) -> None:
        """The output projection over all rows of the set's passes, and each pass's loss."""
        proj, (R, V) = dec.mm.proj, dec.logits.shape
        self._gemm(calls, dec.tag + ".logits_g", [dict(a=dec.flat["hs"].data_ptr(), b=proj.weight.data_ptr(), c=dec.logits.data_ptr(), M=R, N=V,
                                                       K=256, lda=256, ldb=256, ldc=V, tb=1, bias=proj.bias.data_ptr())])
        for p in dec.passes:
            p.loss.forward(calls, self.stream)

    # ---- the plan ----------------------------------------------------------------------------------------------------------
    def _build(self) -> None:
        if self.pg.derived is None or self.qr.derived is None or self.prior._derived() is None:
            raise PlanUnsupported("derived parameters")
        self._generator_encoder()
        dec_pg = self._generator_decoders()
        self._decoder_losses(self.fwd_pg_finish, dec_pg)  # (apart from the decoders: the samples are what the host waits for)
        e_pr = self._reconstructor_encoder()
        dec_qr = self._reconstructor_decoder()
        self._prior_loss(e_pr)
        self._backward_chain([dec_pg, dec_qr])
        self._parameter_gradients([dec_pg, dec_qr])
        self.out.update(loss_s=dec_pg.passes[0].loss.loss, loss_t=dec_pg.passes[1].loss.loss, loss_q=dec_qr.passes[0].loss.loss)
        self._derived_sig = self._sig()

    def _generator_encoder(self) -> None:
        """The encoder over the [unsupervised ; supervised] questions."""
        pg, f = self.pg, self.buf
        self.out = dict(ques=f("ques", self.B, self.tq, dtype=torch.long), prog_sup=f("prog_sup", self.m, self.tp, dtype=torch.long))
        self.e_pg = self._encoder_prepare(self.fwd_pg_enc, _EncoderPass(
            "pg.e", pg, pg.model._source_embedder.embedding, self.out["ques"], self.tq, self.B, p=self.drop_p[0]))
        self._encoders_fwd(self.fwd_pg_enc, "pg.e", [self.e_pg], most=STACK_PG_ENCODER)
        #: workgroups of the generator's encoder launch (0: a launch per layer): a trainer that runs the NMN's stem beside it
        #: cuts the stem's launches for the CUs this leaves (JointTrainingStep)
        stacked = any(name.startswith("pnmn_lstm_stack_fwd") for _, _, name in self.fwd_pg_enc)
        self.pg_encoder_workgroups = 16 * (-(-self.B // 16)) if stacked else 0
        if self.e_pg["T"] > 64 or self.D > 64:
            raise PlanUnsupported("more than 64 source positions / decoding steps")

    def _generator_decoders(self) -> _DecoderSet:
        """The sampling decode of rows [0, n) and the teacher-forced decode of rows [n, B) over [@start@, program, @end@] in one
        launch, and the samples' trimmed copy."""
        n, m, D, tp, f = self.n, self.m, self.D, self.tp, self.buf
        tgt, raw, z = f("pg.tgt", m, tp + 2, dtype=torch.long), f("pg.raw", n, D, dtype=torch.long), f("pg.z", n, D, dtype=torch.long)
        dec = self._decoder_set("pg", self.pg, self.e_pg, [("pg.s", "_s", n, D, raw, z), ("pg.t", "_t", m, tp + 1, tgt, None)])
        self.pair_jobs = self._decoder_forward(self.fwd_pg, dec, self.out["prog_sup"], tgt, "pg.pair_ws")
        self.fwd_pg.add("pnmn_trim_predictions", raw.data_ptr(), n, D, self.pg.model._end_index, z.data_ptr(), self.stream)
        self.out.update(z=z, raw=raw)
        return dec

    def _reconstructor_encoder(self) -> Dict:
        """The encoder over the [sampled ; ground-truth] programs.  The prior reads the same samples: its two LSTM layers ride
        in this launch (its projections and loss follow in `fwd_prior`, behind the trunk's launch); returns its pass."""
        n, m, D, tp, qr, pr, c = self.n, self.m, self.D, self.tp, self.qr, self.prior, self.fwd_qr
        z, Wq = self.out["z"], max(D, tp)
        source = self.buf("qr.source", self.B, Wq, dtype=torch.long)
        segs = np.zeros(2, _hip.TOKEN_SEG)
        segs[0]["src"], segs[0]["row_stride"], segs[0]["rows"], segs[0]["width"] = z.data_ptr(), D, n, D
        segs[1]["src"], segs[1]["row_stride"], segs[1]["rows"], segs[1]["width"] = self.out["prog_sup"].data_ptr(), tp, m, tp
        self._keep.append(segs)
        c.add("pnmn_token_rows", segs.ctypes.data, 2, source.data_ptr(), Wq, 0, self.stream)
        self.e_qr = self._encoder_prepare(c, _EncoderPass(
            "qr.e", qr, qr.model._source_embedder.embedding, source, Wq, self.B, p=self.drop_p[1]))
        e_pr = self._encoder_prepare(c, _EncoderPass("pr.e", None, pr._embedder.embedding, z, D, n, drop_first=False, want_last=False))
        self._encoders_fwd(c, "qr.e", [self.e_qr, e_pr])
        if self.e_qr["T"] > 64 or self.tq + 1 > 64:
            raise PlanUnsupported("more than 64 positions in the reconstructor")
        return e_pr

    def _reconstructor_decoder(self) -> _DecoderSet:
        """The teacher-forced decode of all rows over [@start@, question, @end@], and its loss."""
        tgt = self.buf("qr.tgt", self.B, self.tq + 2, dtype=torch.long)
        dec = self._decoder_set("qr", self.qr, self.e_qr, [("qr.q", "", self.B, self.tq + 1, tgt, None)])
        self._keep.append(self._decoder_forward(self.fwd_qr, dec, self.out["ques"], tgt, "qr.dec_ws"))
        self._decoder_losses(self.fwd_qr, dec)
        return dec

    def _prior_loss(self, e_pr: Dict) -> None:
        """The prior's projections and loss over the samples (no gradient: its loss only enters the detached reward)."""
        n, pr, c, f = self.n, self.prior, self.fwd_prior, self.buf
        emb, src, Tz, Vz = pr._embedder.embedding.weight, e_pr["src"], e_pr["T"], pr._embedder.embedding.weight.size(0)
        proj, plog = f("pr.proj", n * Tz, 256), f("pr.logits", n * Tz, Vz)
        # (the padded steps are not zeroed as PytorchSeq2SeqWrapper does: they only meet padded targets, whose weight is zero)
        self._gemm(c, "pr.proj_g", [dict(a=e_pr["hs2"].data_ptr(), b=pr._projection_layer.weight.data_ptr(), c=proj.data_ptr(), M=n * Tz,
                                         N=256, K=256, lda=256, ldb=256, ldc=256, tb=1)])
        self._gemm(c, "pr.out_g", [dict(a=proj.data_ptr(), b=emb.data_ptr(), c=plog.data_ptr(), M=n * Tz, N=Vz, K=256, lda=256, ldb=256,
                                        ldc=Vz, tb=1)])
        loss = _Loss(plog, Tz * Vz, src.data_ptr() + 8, src.stride(0), src.data_ptr() + 8, src.stride(0), pr._pad_index,
                     f("pr.loss", n), f("pr.lse", n, Tz - 1), n, Tz - 1, Vz, 1e-13)
        loss.forward(c, self.stream)
        self.out["loss_p"] = loss.loss
        self.prior_sig = tuple(p.data_ptr() for p in pr.parameters())

    def _backward_chain(self, decs: List[_DecoderSet]) -> None:
        """`bwd_a`: the losses' backward, the output projections' data gradient, every decoder pass's backward in one launch and
        the encoder-output gradients; `bwd_b` begins with the encoders' layers."""
        c, f, st = self.bwd_a, self.buf, self.stream
        passes = [(dec, p) for dec in decs for p in dec.passes]
        self.d_rows = {key: f("d.loss_" + key, p.rows) for key, (_, p) in zip("stq", passes)}
        for dloss, (dec, p) in zip(self.d_rows.values(), passes):
            p.loss.backward(c, dloss, dec.dlogits[p.row0:], st)
        self._gemm(c, "dhs_g", [dict(a=dec.dlogits.data_ptr(), b=dec.mm.proj.weight.data_ptr(), c=dec.flat["dhs"].data_ptr(), M=dec.logits.size(0),
                                     N=256, K=dec.logits.size(1), lda=dec.logits.size(1), ldb=256, ldc=256) for dec in decs])
        for dec in decs:  # (gradients of what the decoders read of their encoder: its masked outputs and last states)
            dec.enc["denc"], dec.enc["dh"] = f(dec.tag + ".denc", *dec.enc["enc"].shape), f(dec.tag + ".dh", *dec.enc["h"].shape)
        bj = np.zeros(len(passes), _hip.DECODER_BWD_JOB)
        for j, (dec, p) in zip(bj, passes):
            e, r0 = dec.enc, p.enc_row0
            j["dhs"], j["act"], j["cs"], j["hs"], j["probs"] = (p.v[k].data_ptr() for k in ("dhs", "act", "cs", "hs", "probs"))
            j["enc"], j["mask"], j["h0"] = e["enc"][r0:].data_ptr(), e["fmask"][r0:].data_ptr(), e["h"][r0:].data_ptr()
            j["w_c_t"], j["w_hh_t"] = dec.mm.derived["d.cT"].data_ptr(), dec.mm.derived["d.hhT"].data_ptr()
            j["dgates"], j["dctx"], j["dscore"], j["weights"] = (p.v[k].data_ptr() for k in ("dg", "dctx", "dscore", "weights"))
            j["dh0"] = e["dh"][r0:].data_ptr()
            j["B"], j["T"], j["S"] = p.rows, p.T, p.S
        self._keep.append(bj)
        gws = self.bytes_buf("group_ws", _hip.decoder_workspace_bytes([p.rows for _, p in passes], True))
        ordered = self._order_lists([p for _, p in passes])
        c.add("pnmn_attn_lstm_bwd_group_ordered" if ordered else "pnmn_attn_lstm_bwd_group", bj.ctypes.data, len(bj), 256, *ordered,
              gws.data_ptr(), st)
        for dec, p in passes:
            c.add("pnmn_attn_denc", p.v["weights"].data_ptr(), p.v["dscore"].data_ptr(), p.v["dctx"].data_ptr(), p.v["hs"].data_ptr(),
                  dec.enc["h"][p.enc_row0:].data_ptr(), dec.enc["denc"][p.enc_row0:].data_ptr(), p.rows, p.T, p.S, 256, st)
        self._encoders_bwd(self.bwd_b, "enc", [dec.enc for dec in decs])

    def _parameter_gradients(self, decs: List[_DecoderSet]) -> None:
        """Nothing in backward waits for a parameter gradient, so they all follow the chain at the end of `bwd_b`: the token
        tables' as launches, every product over all steps in one grouped GEMM launch."""
        c, deferred = self.bwd_b, []
        for dec in decs:
            mm, flat, (R, V), g, cell = dec.mm, dec.flat, dec.logits.shape, dec.mm.grad, dec.mm.cell
            self._table_backward(c, dec.table, mm, mm.model._start_index,
                                 [("%s.d.emb_ws%d" % (dec.tag, k), p.v["dg"], p.tokens, p.shift) for k, p in enumerate(dec.passes)])
            # (a pass's valid steps end at the last one its loss weights: dlogits and dgates are zero behind it.  The products over
            # the flat buffers take the passes' list, the recurrent weights' each pass's own: a list's first steps point at
            # ITS h0 rows.  A model with one pass has one list.)
            segs = [(0, p.loss.mask, p.loss.mask_stride, p.loss.pad, p.rows, p.T) for p in dec.passes]
            listed = self.valid_pairs and sum(p.rows for p in dec.passes) > VALID_PAIRS_ABOVE_ROWS
            whole = dict(valid=self._valid_list(dec.tag + ".d.valid", segs)) if listed else {}
            own = [whole if len(segs) == 1 else dict(valid=self._valid_list(p.tag + ".valid", [seg])) if listed else {}
                   for p, seg in zip(dec.passes, segs)]
            deferred.append(dict(a=dec.dlogits.data_ptr(), b=flat["hs"].data_ptr(), c=g(mm.proj.weight).data_ptr(), M=V, N=256, K=R, lda=V,
                                 ldb=256, ldc=256, ta=1, split="auto", colsum=g(mm.proj.bias).data_ptr(), **whole))
            deferred.append(dict(a=flat["dg"].data_ptr(), b=flat["cx"].data_ptr(), c=g(cell.weight_ih).data_ptr(), M=1024, N=256, K=R, lda=1024,
                                 ldb=256, ldc=512, ta=1, split="auto", **whole))
            for k, p in enumerate(dec.passes):
                deferred.append(dict(a=p.v["dg"].data_ptr(), b=p.v["hs"].data_ptr(), c=g(cell.weight_hh).data_ptr(), M=1024, N=256,
                                     K=p.rows * p.T, lda=1024, ldb=256, ldc=256, ta=1, split="auto", shift_t=p.T,
                                     h0=dec.enc["h"][p.enc_row0:].data_ptr(), ld_h0=256, acc=1 if k else 0, **own[k]))
        self._encoders_param_grads(c, deferred, [dec.enc for dec in decs])
        self._valid_list_calls(c)
        # (an accumulating product must follow the product it adds to: keep them in different launches)
        self._gemm(c, "wgrad", [d for d in deferred if not d.get("acc")])
        self._gemm(c, "wgrad2", [d for d in deferred if d.get("acc")])

    def _sig(self):
        return tuple(t.data_ptr() for model in (self.pg.model, self.qr.model, self.prior) for t in model._derived().values())

    def still_valid(self) -> bool:
        """Parameters, derived copies and the stream are where the plan's calls point (a ``.to()``, a re-pointed parameter
        or another current stream: rebuild).  Also refreshes the derived copies (one launch per model and optimiser step)."""
        if _hip.stream_ptr(self.dev) != self.stream:
            return False
        for mm in (self.pg, self.qr):
            if tuple(p.data_ptr() for p in mm.params) != mm.signature:
                return False
        if tuple(p.data_ptr() for p in self.prior.parameters()) != self.prior_sig:
            return False
        if (_dropout_p(self.pg.lstm), _dropout_p(self.qr.lstm)) != self.drop_p:
            return False
        if self.prior.training and _dropout_p(self.prior._encoder._module) > 0:
            return False
        return self._sig() == self._derived_sig

    # ---- one iteration -------------------------------------------------------------------------------------------------------
    def run_encoder(self, question: torch.Tensor, program: torch.Tensor, nosup_d: torch.Tensor, sup_d: torch.Tensor) -> None:
        """The row subsets [unsupervised ; supervised] of the batch's questions, the supervised rows' programs, and the
        generator's encoder over the questions."""
        lib, st = _hip.lib(), self.stream
        if question.dtype != torch.long or program.dtype != torch.long or question.stride(1) != 1 or program.stride(1) != 1:
            raise _hip.HipLibraryError("token matrices must be int64 with contiguous rows")
        segs = np.zeros(2, _hip.TOKEN_SEG)
        segs[0]["src"], segs[0]["index"], segs[0]["row_stride"], segs[0]["rows"], segs[0]["width"] = \
            question.data_ptr(), nosup_d.data_ptr(), question.stride(0), self.n, self.tq
        segs[1]["src"], segs[1]["index"], segs[1]["row_stride"], segs[1]["rows"], segs[1]["width"] = \
            question.data_ptr(), sup_d.data_ptr(), question.stride(0), self.m, self.tq
        _hip.check(lib.pnmn_token_rows(segs.ctypes.data, 2, self.out["ques"].data_ptr(), self.tq, 0, st), "token_rows")
        segs[0]["src"], segs[0]["index"], segs[0]["row_stride"], segs[0]["rows"], segs[0]["width"] = \
            program.data_ptr(), sup_d.data_ptr(), program.stride(0), self.m, self.tp
        _hip.check(lib.pnmn_token_rows(segs.ctypes.data, 1, self.out["prog_sup"].data_ptr(), self.tp, 0, st), "token_rows")
        # one seed per pass, drawn as Seq2SeqBase.decode_prepare draws them (sampling, teacher-forced, reconstructor): the
        # eager and the planned iteration sample the same programs from the same torch seed -- with an encoder's dropout seed
        # (Seq2SeqBase.encode) where the eager iteration draws it: before its model's decode seeds
        if self.drop_p[0] > 0:
            self._set_dropout(self.e_pg, int(torch.randint(0, 2 ** 62, (1,)).item()), self.pg.model.sample_row_offset)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        torch.randint(0, 2 ** 62, (1,))
        if self.drop_p[1] > 0:
            self._set_dropout(self.e_qr, int(torch.randint(0, 2 ** 62, (1,)).item()), self.qr.model.sample_row_offset)
        torch.randint(0, 2 ** 62, (1,))
        self.pair_jobs[0]["seed"] = seed
        self.pair_jobs[0]["row_offset"] = self.pg.model.sample_row_offset
        self.fwd_pg_enc.run()

    def run_decoders(self) -> torch.Tensor:
        """The generator's sampling + teacher-forced decoder pair and the trim; returns the trimmed samples z [n, D] (a
        persistent buffer: overwritten by the next iteration)."""
        self.fwd_pg.run()
        return self.out["z"]

    def run_generator_finish(self) -> None:
        self.fwd_pg_finish.run()

    def run_reconstructor(self) -> None:
        self.fwd_qr.run()

    def run_prior(self) -> torch.Tensor:
        self.fwd_prior.run()
        return self.out["loss_p"]

    def losses(self):
        """(generator loss of the sampled rows [n], generator cross entropy of the supervised rows [m], reconstruction
        losses [n + m]) as outputs of the plan's single autograd node."""
        return _PlanNode.apply(self.anchor, self)

    def backward(self, d_s, d_t, d_q) -> None:
        for key, d in (("s", d_s), ("t", d_t), ("q", d_q)):
            if d is None:
                self.d_rows[key].zero_()
            else:
                self.d_rows[key].copy_(d)
        self.bwd_a.run()
        self.bwd_b.run()
        self.pg.attach()
        self.qr.attach()


class _PlanNode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, plan: Seq2SeqPlan):
        ctx.plan = plan
        o = plan.out
        return o["loss_s"].view_as(o["loss_s"]), o["loss_t"].view_as(o["loss_t"]), o["loss_q"].view_as(o["loss_q"])

    @staticmethod
    def backward(ctx, d_s, d_t, d_q):
        ctx.plan.backward(d_s, d_t, d_q)
        return None, None
