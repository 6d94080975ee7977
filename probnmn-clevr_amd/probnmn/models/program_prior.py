"""``ProgramPrior``: LSTM language model over programs, p(z) (reference:
probnmn/models/program_prior.py:15-155).  Input and output embeddings are tied.  ``forward`` gives
the per-sequence cross entropy used as -log p(z) in the REINFORCE reward, plus per-position
samples (unused by the trainers).  ``sample`` (reference :174-301) is outside the training hot path; on the shapes
of the reference configuration it is one persistent HIP launch (``pnmn_prior_sample``)."""
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from probnmn import _hip
from probnmn.modules.seq2seq_base import (DerivedParams, _Encoder, _TokenEmbedder, _TokenPrep, _TokenTable, constraint_tables,
                                          lstm_bias, lstm_derived_params, lstm_derived_specs, lstm_dropout_seed,
                                          sampling_filter, sequence_nll)
from probnmn.running_metrics import Average


class PriorSampleWeights(NamedTuple):
    """What ``pnmn_prior_sample`` reads (include/probnmn_hip.h), on the device, contiguous fp32."""
    table0: torch.Tensor   # [V, 1024]  Emb W_ih0^T + b_ih0 + b_hh0
    w_hh0: torch.Tensor    # [1024, 256] in fragment order (``pack_fragments``), as the next two
    w_ih1: torch.Tensor
    w_hh1: torch.Tensor
    b1: torch.Tensor       # [1024]  b_ih1 + b_hh1
    w_proj: torch.Tensor   # [256, 256] in fragment order
    w_out: torch.Tensor    # [V, 256] row major
    pad: int
    unk: int
    start: int


def prior_sample_call(w: PriorSampleWeights, num_samples: int, steps: int, mode: int, seed: int, row_offset: int = 0,
                      forced: Optional[torch.Tensor] = None, filt=None, constraint=None, want_proj: bool = False):
    """``pnmn_prior_sample`` on explicit weights: (tokens int64 [B, T], logprob_vocab [B, T], logprob_proj [B, T], proj
    [B, T, 256] or None).  ``mode`` 0 (``forced`` [B, >= T] int64 replaces the choice), 1 (sample) or 2 (greedy); ``filt``:
    ``sampling_filter``'s tuple or None; ``constraint``: ``constraint_tables``' tuple or None."""
    dev = w.table0.device
    B, T, V = int(num_samples), int(steps), w.table0.size(0)
    tokens = torch.empty(B, T, dtype=torch.long, device=dev)
    lp_vocab = torch.empty(B, T, dtype=torch.float32, device=dev)
    lp_proj = torch.empty(B, T, dtype=torch.float32, device=dev)
    proj = torch.empty(B, T, 256, dtype=torch.float32, device=dev) if want_proj else None
    if forced is not None:
        forced = forced.to(device=dev, dtype=torch.long)
        if forced.dim() != 2 or forced.size(0) != B or forced.size(1) < T or forced.stride(1) != 1:
            raise ValueError("forced tokens of shape %s / strides %s for %d rows of %d steps" % (tuple(forced.shape), forced.stride(), B, T))
    rec = None if filt is None else np.array([(*filt, 0)], _hip.SAMPLING_FILTER)
    tables = (None, None, None, 0) if constraint is None else constraint
    _hip.check(_hip.lib().pnmn_prior_sample(
        w.table0.data_ptr(), w.w_hh0.data_ptr(), w.w_ih1.data_ptr(), w.w_hh1.data_ptr(), w.b1.data_ptr(), w.w_proj.data_ptr(),
        w.w_out.data_ptr(), tokens.data_ptr(), lp_vocab.data_ptr(), lp_proj.data_ptr(), None if proj is None else proj.data_ptr(),
        B, T, V, w.w_proj.numel() // 256, mode, w.pad, w.unk, w.start, seed, row_offset,
        None if forced is None else forced.data_ptr(), 0 if forced is None else forced.stride(0),
        None if rec is None else rec.ctypes.data, tables[3],
        *(None if t is None else t.ctypes.data for t in tables[:3]),
        0 if constraint is None else tables[1].shape[0], 0 if constraint is None else tables[1].shape[1],
        _hip.stream_ptr(dev)), "prior_sample")
    return tokens, lp_vocab, lp_proj, proj


@torch.no_grad()
def prior_sample_launch(prior, num_samples: int, steps: int, mode: int, seed: int, row_offset: int = 0, forced=None, filt=None,
                        constraint=None, want_proj: bool = False):
    """``prior_sample_call`` on a ``ProgramPrior``'s own weights: the per-token table of its first layer (one launch) and
    the fragment-order packs of ``DerivedParams``; the tied embedding is read in place as W_out."""
    derived = prior._derived()
    if derived is None or "proj" not in derived:
        raise _hip.HipLibraryError("prior_sample_launch: the kernel is built for a two-layer LSTM of input = hidden size 256 on a ROCm device")
    lstm, emb = prior._encoder._module, prior._embedder.embedding
    table0 = _TokenTable.apply(emb.weight, lstm.weight_ih_l0, lstm_bias(lstm, 0, derived), emb.padding_idx)
    w = PriorSampleWeights(table0, derived["l0.hh"], derived["l1.ih"], derived["l1.hh"], derived["l1.b"], derived["proj"],
                           emb.weight.detach().contiguous(), prior._pad_index, prior._unk_index, prior._start_index)
    return prior_sample_call(w, num_samples, steps, mode, seed, row_offset, forced, filt, constraint, want_proj)


class ProgramPrior(nn.Module):
    def __init__(self, vocabulary, input_size: int = 256, hidden_size: int = 128, num_layers: int = 2,
                 dropout: float = 0.0):
        super().__init__()
        self.vocabulary = vocabulary
        self._start_index = vocabulary.get_token_index("@start@", namespace="programs")
        self._end_index = vocabulary.get_token_index("@end@", namespace="programs")
        self._pad_index = vocabulary.get_token_index("@@PADDING@@", namespace="programs")
        self._unk_index = vocabulary.get_token_index("@@UNKNOWN@@", namespace="programs")
        vocab_size = vocabulary.get_vocab_size(namespace="programs")
        self._embedder = _TokenEmbedder("programs", vocab_size, input_size, self._pad_index)
        self._encoder = _Encoder(input_size, hidden_size, num_layers, dropout)
        self._projection_layer = nn.Linear(hidden_size, input_size, bias=False)
        self._output_layer = nn.Linear(input_size, vocab_size, bias=False)
        self._output_layer.weight = self._embedder.embedding.weight  # tied
        self._log2_perplexity = Average()
        # row offset of this rank's shard in the global batch: the row key of the dropout masks (as Seq2SeqBase's)
        self.sample_row_offset = 0
        self.__dict__["_derived_cache"] = DerivedParams()  # (packed recurrent weights; not part of the state_dict)

    def _derived(self):
        lstm = self._encoder._module
        if lstm.hidden_size != 256 or lstm.weight_hh_l0.device.type != "cuda":
            return None
        proj = self._projection_layer.weight
        if tuple(proj.shape) != (256, 256):
            return self._derived_cache.get(lstm_derived_params(lstm), lambda: lstm_derived_specs(lstm))
        # (the projection's fragment-order pack rides in the same launch: what pnmn_prior_sample streams per step)
        return self._derived_cache.get(lstm_derived_params(lstm) + [proj],
                                       lambda: lstm_derived_specs(lstm) + [("proj", "pack", proj, None)])

    def _sample_kernel_path(self) -> bool:
        """``sample`` runs as one ``pnmn_prior_sample`` launch: ROCm device, input = hidden size 256, two layers, at most 128
        tokens, and no dropout between the layers (evaluation mode, or ``dropout == 0``)."""
        lstm, w = self._encoder._module, self._output_layer.weight
        return (w.device.type == "cuda" and lstm.input_size == lstm.hidden_size == 256 and lstm.num_layers == 2
                and w.size(0) <= 128 and tuple(self._projection_layer.weight.shape) == (256, 256)
                and (not self.training or lstm.dropout == 0))

    @classmethod
    def from_config(cls, config):
        from probnmn.vocabulary import Vocabulary

        _C = config
        return cls(vocabulary=Vocabulary.from_files(_C.DATA.VOCABULARY), input_size=_C.PROGRAM_PRIOR.INPUT_SIZE,
                   hidden_size=_C.PROGRAM_PRIOR.HIDDEN_SIZE, num_layers=_C.PROGRAM_PRIOR.NUM_LAYERS,
                   dropout=_C.PROGRAM_PRIOR.DROPOUT)

    def forward(self, program_tokens: torch.Tensor, need_predictions: bool = True) -> Dict[str, torch.Tensor]:
        # ``need_predictions=False``: skip the per-position samples (reference :119-143), which no trainer reads
        if program_tokens.device.type != "cuda":
            raise _hip.HipLibraryError("program prior input on %s: the HIP path needs a ROCm device" % program_tokens.device)
        toks, fmask, _ = _TokenPrep.run(program_tokens, self._pad_index, self._start_index, self._end_index,
                                        drop_first=False, want_mask=True)
        seed = lstm_dropout_seed(self._encoder._module)
        encoded = self._encoder.forward_tokens(self._embedder.embedding, toks, fmask, derived=self._derived(), dropout_seed=seed,
                                               row_offset=self.sample_row_offset)
        logits = self._output_layer(self._projection_layer(encoded))
        loss = sequence_nll(logits[:, :-1], toks[:, 1:], toks[:, 1:], self._pad_index, 1e-13)
        if not need_predictions:  # (the trainers' reward path: no samples, no validation metric)
            return {"loss": loss}
        if not self.training:
            self._log2_perplexity(loss.mean())
        with torch.no_grad():
            probs = F.softmax(logits, dim=-1).clone()
            forbidden = self.__dict__.get("_forbidden")
            if forbidden is None or forbidden.device != probs.device:
                forbidden = torch.tensor([self._start_index, self._pad_index, self._unk_index]).to(probs.device)
                self.__dict__["_forbidden"] = forbidden  # cached: building it costs a host -> device copy
            probs.index_fill_(2, forbidden, 0.0)
            B, T, V = probs.shape
            predictions = torch.multinomial(probs.view(B * T, V), 1).view(B, T)
            predictions = predictions[:, :-1] * (toks[:, 1:] != self._pad_index)
        return {"predictions": predictions, "loss": loss}

    @torch.no_grad()
    def teacher_forced_logits(self, program_tokens: torch.Tensor):
        """The first half of ``forward``, for SCORING: (logits [R, T + 1, V], targets [R, T + 1]) -- step t's distribution over
        the token that follows the first t ones and that token (the program's own, @end@ behind the last, padding after);
        log p(z) is the sum over the non-padding targets of ``log_softmax(logits)[target]``.  No loss, no perplexity update,
        no multinomial draw, no dropout whatever the mode and no seed drawn for it, no graph."""
        if program_tokens.device.type != "cuda":
            raise _hip.HipLibraryError("program prior input on %s: the HIP path needs a ROCm device" % program_tokens.device)
        toks, fmask, _ = _TokenPrep.run(program_tokens, self._pad_index, self._start_index, self._end_index,
                                        drop_first=False, want_mask=True)
        encoded = self._encoder.forward_tokens(self._embedder.embedding, toks, fmask, derived=self._derived(),
                                               row_offset=self.sample_row_offset, dropout=False)
        logits = self._output_layer(self._projection_layer(encoded))
        return logits[:, :-1], toks[:, 1:]

    @torch.no_grad()
    def sample(self, num_samples: int = 1, max_sequence_length: int = 28, _forced=None, *, seed: Optional[int] = None,
               temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, constraint=None,
               greedy: bool = False) -> Dict[str, torch.Tensor]:
        """Free-running categorical samples from the prior, most likely first (reference :174-301; inspection and synthetic
        programs, no trainer calls it).  Reproduced as the reference has it, including that the per-step log-probability
        behind ``"loss"`` is gathered from ``log_softmax`` of the 256-wide PROJECTION, not of the vocabulary logits
        (:243-244,257-259).  Returns ``"predictions"`` [B, T] (T = max_sequence_length - 1; kept up to and including the first
        @end@, a row starting with @end@ all padding), ``"loss"`` [B] ascending, and -- on the kernel path -- ``"log_probability"``
        [B] in the same order: the sum of ``log_softmax(z)[token]`` over the kept tokens, log p(z) as ``forward`` scores it.

        On a ROCm device with input = hidden size 256, two layers, at most 128 tokens and no active dropout, all T steps are ONE
        ``pnmn_prior_sample`` launch (the rule: include/probnmn_hip.h).  ``seed``: None draws one from the torch CPU generator as
        ``Seq2SeqBase.decode`` does (``torch.manual_seed`` makes the call reproducible); ``self.sample_row_offset`` is the row
        key.  ``temperature`` / ``top_k`` / ``top_p``: the decoders' sampling filter; ``constraint``: a token automaton
        (``ProgramCompiler.decoding_automaton``) under which every kept row is a valid program; ``greedy``: the arg-max in the
        place of the draw.  The log-probabilities stay those of the unmodified distribution.
        ``_forced`` (steps = max_sequence_length - 1 columns; replaces the draws in tests), and every other shape, run the
        step-by-step torch loop, which has none of these options: ``NotImplementedError``."""
        filt = sampling_filter(temperature, top_k, top_p)
        if greedy and filt is not None:
            raise ValueError("temperature / top_k / top_p filter a draw; a greedy sample draws nothing")
        steps = max_sequence_length - 1
        tables = None
        if constraint is not None:
            tables = constraint_tables(constraint, self._output_layer.weight.size(0), self._end_index)
            if int(tables[2][0]) > steps:
                raise ValueError("constraint: the shortest accepted string takes %d tokens, max_sequence_length - 1 is %d"
                                 % (int(tables[2][0]), steps))
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64):
            raise ValueError("seed must be an integer in [0, 2**64), got %r" % (seed,))
        if _forced is None and steps >= 1 and self._sample_kernel_path():
            if greedy:
                seed = 0
            elif seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
            raw, lp_vocab, lp_proj, _ = prior_sample_launch(self, num_samples, steps, 2 if greedy else 1, int(seed),
                                                            self.sample_row_offset, None, filt, tables)
            return self._trim_and_sort(raw, lp_proj, lp_vocab)
        if seed is not None or filt is not None or constraint is not None or greedy:
            lstm = self._encoder._module
            raise NotImplementedError(
                "seed / temperature / top_k / top_p / constraint / greedy exist in the persistent prior kernel only (ROCm device, input "
                "= hidden size 256, two layers, <= 128 tokens, no active dropout, no _forced); this is %s, %d -> %d x %d layers, %d "
                "tokens%s" % (self._output_layer.weight.device, lstm.input_size, lstm.hidden_size, lstm.num_layers,
                              self._output_layer.weight.size(0), ", _forced" if _forced is not None else ""))
        return self._sample_loop(num_samples, max_sequence_length, _forced)

    @torch.no_grad()
    def _sample_loop(self, num_samples: int, max_sequence_length: int, _forced=None) -> Dict[str, torch.Tensor]:
        """``sample`` with torch ops, one step at a time, on the model's device: every shape the kernel is not built for, and
        ``_forced``."""
        device = self._output_layer.weight.device
        lstm = self._encoder._module
        last = torch.full((num_samples, 1), self._start_index, dtype=torch.long, device=device)
        h = torch.zeros(lstm.num_layers, num_samples, lstm.hidden_size, device=device)
        c = torch.zeros_like(h)
        step_logprobs, step_predictions = [], []
        for t in range(max_sequence_length - 1):
            encoded, (h, c) = lstm(self._embedder.embedding(last), (h, c))
            projection = self._projection_layer(encoded)
            probabilities = F.softmax(self._output_layer(projection), dim=-1)
            logprobs = F.log_softmax(projection, dim=-1)
            probabilities[:, :, [self._start_index, self._pad_index, self._unk_index]] = 0
            last = torch.multinomial(probabilities.squeeze(1), 1) if _forced is None else _forced[:, t:t + 1].to(device)
            step_predictions.append(last)
            step_logprobs.append(torch.gather(logprobs, 2, last.unsqueeze(1)).squeeze(-1))
        return self._trim_and_sort(torch.cat(step_predictions, 1), torch.cat(step_logprobs, 1))

    def _trim_and_sort(self, raw, step_logprobs, vocab_logprobs=None) -> Dict[str, torch.Tensor]:
        # keep up to and including the first @end@; a row starting with @end@ becomes padding (:270-280)
        steps = raw.size(1)
        is_end = raw == self._end_index
        first = is_end.float().argmax(1, keepdim=True)
        pos = torch.arange(steps, device=raw.device).unsqueeze(0)
        keep = torch.where(is_end.any(1, keepdim=True), (pos <= first) & (first > 0), torch.ones_like(is_end))
        predictions = raw * keep
        mask = (predictions != self._pad_index).float()
        sequence_logprobs = (step_logprobs * mask).sum(-1) / (mask.sum(-1) + 1e-12)
        order = (-sequence_logprobs).sort()[1]
        out = {"predictions": predictions[order], "loss": -sequence_logprobs[order]}
        if vocab_logprobs is not None:
            out["log_probability"] = (vocab_logprobs * mask).sum(-1)[order]
        return out

    def get_metrics(self, reset: bool = True) -> Dict[str, float]:
        return {"perplexity": 2 ** self._log2_perplexity.get_metric(reset=reset)}
