"""``NeuralModuleNetwork`` -- class surface of the reference's ``probnmn.models.nmn`` (reference:
probnmn/models/nmn.py:23-296) executed by the gfx950 engine.

Same constructor / ``from_config`` arguments, same submodule and ``state_dict`` names (``stem.0``,
``stem.2``, ``classifier.{0,4,6}``, one child per program token), same ``forward`` signature and
return dict.  What differs is how ``forward`` gets there: programs are compiled statically
(validity included -- the reference's bare ``except`` is not reproduced, kernel errors surface),
all module calls of the batch run as grouped kernels, and stem / classifier conv / max-pool are
part of the same explicit forward+backward schedule (``probnmn.runtime.engine``).
"""
from typing import Dict, Optional, Tuple

import torch
from torch import nn
from torch.nn import functional as F

from probnmn.modules.nmn_modules import (
    AndModule,
    AttentionModule,
    ComparisonModule,
    Flatten,
    OrModule,
    QueryModule,
    RelateModule,
    SameModule,
)
from probnmn.runtime import program_compiler as pc
from probnmn.running_metrics import Average, BooleanAccuracy

INVALID_PROGRAM_LOSS = 3.33  # ~ ln(28), the reference's constant (nmn.py:260,269)


class _Tokens:
    """A batch of programs as the host token matrix, on its way through the library's trunk planner
    (``NMNEngine.run_forward_tokens``); ``valid`` is filled in by the forward pass."""

    __slots__ = ("tokens", "valid", "attention")

    def __init__(self, tokens):
        self.tokens, self.valid = tokens, None
        self.attention = None  # (maps, mask) when the caller asked for them (``return_attention``)


class _Trunk(torch.autograd.Function):
    """stem -> module programs -> classifier conv + max-pool, as one autograd node."""

    @staticmethod
    def forward(ctx, features, engine, compiled, started, *params):
        need_backward = any(ctx.needs_input_grad)  # (requires_grad of the inputs, whatever the grad mode)
        # the library compiles, plans and launches from the token matrix
        pooled, state, compiled.valid = engine.run_forward_tokens(features, compiled.tokens, need_backward, started)
        ctx.engine, ctx.state, ctx.n_params = engine, state, len(params)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        if ctx.state is None:
            raise RuntimeError("backward through a forward that was run without gradient tracking")
        grads = ctx.engine.run_backward(ctx.state, dpooled)
        return (None, None, None, None, *grads[: ctx.n_params])


class _SplitKLinear(torch.autograd.Function):
    """``F.linear`` for the classifier's first fully connected layer (K = class_projection_channels * H * W / 4 = 50 176
    inputs -> 1024 units; reference nmn.py:76-83) with the FORWARD product split along K: x [B, K] @ W^T [K, N] has only
    B/32 x N/96 output tiles for the library GEMM (22 workgroups at 64 rows, 170 at 512) over a 50 176-long reduction;
    sixteen K-slabs as ONE strided-batched GEMM (no copies: both operands are views) fill the chip and the partial
    products add up after.  Measured (scripts/fc_gemm_probe.py): 179 -> 65 us at 64 rows, 579 -> 398 us at 512.
    The two gradient products already have large outputs and stay plain GEMMs."""

    SLABS = 16

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        B, K = x.shape
        N, S = weight.size(0), _SplitKLinear.SLABS
        xs = x.view(B, S, K // S).transpose(0, 1)             # [S, B, K/S]
        ws = weight.view(N, S, K // S).permute(1, 2, 0)       # [S, K/S, N]
        return torch.bmm(xs, ws).sum(0).add_(bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dy @ weight if ctx.needs_input_grad[0] else None
        dw = dy.t() @ x if ctx.needs_input_grad[1] else None
        db = dy.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db


class _WeightGradOnly(torch.autograd.Function):
    """The weight / bias gradient of a linear layer as a node of its OWN: forward contributes zeros, backward computes
    dy^T x and sum(dy).  With ``_first_fc`` below the layer's backward is two nodes -- d(input) first, then this one -- so
    that what waits for d(input) (the trunk's backward, on its own stream) is released by the event behind the first GEMM
    instead of behind both: the 50 176 x 1024 weight-gradient GEMM (0.45 ms at 512 rows) then runs beside the trunk's first
    backward launches instead of in front of them.  (Deferring it to the end of backward instead would also delay the
    early all-reduce of this 205 MB gradient under data parallelism.)"""

    @staticmethod
    def forward(ctx, weight, bias, x):
        ctx.save_for_backward(x)
        return x.new_zeros(x.size(0), weight.size(0))

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return (dy.t() @ x if ctx.needs_input_grad[0] else None, dy.sum(0) if ctx.needs_input_grad[1] else None, None)


# ---- the same layer on this build's GEMM (csrc/gemm.hip) ----------------------------------------------------------------
# OPT-IN (PNMN_FC_OWN_ROWS=<rows>: from that many rows on; default 0 = never): the three products of the layer on pnmn_gemm --
# whole 128-row tiles straight into LDS, the forward product split along K so that its 8 x rows/128 output tiles fill the
# chip (partials added in chunk order: deterministic), the bias added in the epilogue, the bias gradient summed beside the
# weight gradient (colsum).  Measured at 512 rows (the 1024-question step): forward 503 us, d(input) 499, weight gradient
# 460 against the library path's 398 / 437 / 418 -- the step 27.60 against 27.13 ms (28.99 / 28.59 on one stream); at 64 rows
# a 128-row tile is half empty (41 against 88 TFLOP/s).  So the library path above stays the default (DESIGN 4.2 "Round 6").
OWN_FC_ROWS = int(__import__("os").environ.get("PNMN_FC_OWN_ROWS", "0"))
_FC_WORKSPACES: dict = {}


def _own_gemm(a, b, c, M, N, K, lda, ldb, ldc, ta=False, tb=False, bias=None, colsum=None, split=1):
    import numpy as np
    from probnmn import _hip

    lib, dev = _hip.lib(), c.device
    d = np.zeros(1, _hip.GEMM_DESC)
    d["a"], d["b"], d["c"] = a.data_ptr(), b.data_ptr(), c.data_ptr()
    d["lda"], d["ldb"], d["ldc"], d["M"], d["N"], d["K"] = lda, ldb, ldc, M, N, K
    d["flags"] = (_hip.GEMM_A_T if ta else 0) | (_hip.GEMM_B_T if tb else 0)
    d["split_k"] = split
    if bias is not None:
        d["bias"] = bias.data_ptr()
    if colsum is not None:
        d["colsum"] = colsum.data_ptr()
    if split > 1:
        need = int(lib.pnmn_gemm_workspace_bytes(M, N, split))
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        ws = _FC_WORKSPACES.get(key)
        if ws is None or ws.numel() < need:  # (one grow-only buffer per device: the products of a step run one after another)
            ws = _FC_WORKSPACES[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        d["workspace"] = ws.data_ptr()
    _hip.check(lib.pnmn_gemm(d.ctypes.data, 1, _hip.stream_ptr(dev)), "pnmn_gemm (fully connected layer)")


class _OwnLinear(torch.autograd.Function):
    """``F.linear`` of the first fully connected layer on pnmn_gemm: y = x W^T + b; backward: d(input) only (the weight
    gradient is ``_OwnWeightGrad``'s, see ``_WeightGradOnly`` for why the two are separate nodes)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from probnmn import _hip

        ctx.save_for_backward(weight)
        M, K = x.shape
        N = weight.size(0)
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        split = int(_hip.lib().pnmn_gemm_split_k(M, N, K, 0))
        _own_gemm(x, weight, y, M, N, K, K, K, N, tb=True, bias=bias, split=split)
        return y

    @staticmethod
    def backward(ctx, dy):
        (weight,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dy = dy.contiguous()
        M, N = dy.shape
        K = weight.size(1)
        dx = torch.empty(M, K, dtype=dy.dtype, device=dy.device)
        _own_gemm(dy, weight, dx, M, K, N, N, K, K)  # dy [M][N] . W [N][K]
        return dx, None, None


class _OwnWeightGrad(torch.autograd.Function):
    """``_WeightGradOnly`` on pnmn_gemm: dW = dy^T x with db = the column sums of dy from the same pass."""

    @staticmethod
    def forward(ctx, weight, bias, x):
        ctx.save_for_backward(x)
        return x.new_zeros(x.size(0), weight.size(0))

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        R, N = dy.shape
        K = x.size(1)
        dw = torch.empty(N, K, dtype=dy.dtype, device=dy.device)
        db = torch.empty(N, dtype=dy.dtype, device=dy.device)
        _own_gemm(dy, x, dw, N, K, R, N, K, K, ta=True, colsum=db)  # dy^T [N][R] . x [R][K]
        return dw, db, None


def _first_fc(layer: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    K = layer.in_features
    if (x.is_cuda and x.dim() == 2 and x.is_contiguous() and layer.weight.is_contiguous() and layer.bias is not None
            and x.dtype == torch.float32 and 0 < OWN_FC_ROWS <= x.size(0) and K % 4 == 0):
        if torch.is_grad_enabled() and x.requires_grad and layer.weight.requires_grad:
            from_weights = _OwnWeightGrad.apply(layer.weight, layer.bias, x.detach())
            return _OwnLinear.apply(x, layer.weight.detach(), layer.bias.detach()) + from_weights
        if not torch.is_grad_enabled() or not (x.requires_grad or layer.weight.requires_grad or layer.bias.requires_grad):
            return _OwnLinear.apply(x, layer.weight, layer.bias)
        # (gradients for some of the three only: the library path below knows every combination)
    if (x.is_cuda and x.dim() == 2 and x.is_contiguous() and layer.weight.is_contiguous() and layer.bias is not None
            and K % _SplitKLinear.SLABS == 0 and K >= 8192):
        if torch.is_grad_enabled() and x.requires_grad and layer.weight.requires_grad:
            # (autograd runs the node created LAST first: the weight-gradient node is made before the product)
            from_weights = _WeightGradOnly.apply(layer.weight, layer.bias, x.detach())
            return _SplitKLinear.apply(x, layer.weight.detach(), layer.bias.detach()) + from_weights
        return _SplitKLinear.apply(x, layer.weight, layer.bias)
    return layer(x)


class _AnswerLoss(torch.autograd.Function):
    """``pnmn_answer_loss``: log-softmax over the answers, arg-max prediction, cross entropy, the
    invalid-program overrides (prediction @@UNKNOWN@@, constant loss 3.33, no gradient) and d loss / d logits
    in one launch (reference nmn.py:245-269)."""

    @staticmethod
    def forward(ctx, logits, answers, valid, unknown_index):
        from probnmn import _hip

        logits = logits.contiguous()
        B, A = logits.shape
        dev = logits.device
        predictions = torch.empty(B, dtype=torch.long, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        dlogits = torch.empty(B, A, dtype=torch.float32, device=dev) if answers is not None else None
        _hip.check(_hip.lib().pnmn_answer_loss(
            logits.data_ptr(), 0 if answers is None else answers.data_ptr(), valid.data_ptr(), predictions.data_ptr(),
            loss.data_ptr(), 0 if dlogits is None else dlogits.data_ptr(), B, A, unknown_index, 1.0,
            _hip.stream_ptr(dev)), "answer_loss")
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(predictions)
        return loss, predictions

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        if dlogits is None:
            raise RuntimeError("the answer loss without answers (-max log-probability) is an evaluation quantity")
        return dlogits * dloss.unsqueeze(1), None, None, None


class _MarginalAnswerLoss(torch.autograd.Function):
    """The marginal likelihood of each question's answer over its program hypotheses,
        loss[g] = -log sum_r w_r p(a_g | z_r, image)^answer_weight       over the rows r of question g,
    and d loss / d logits in ONE launch: ``pnmn_answer_posterior`` in gradient mode (include/probnmn_hip.h) -- a row's
    cross-entropy gradient scaled by the row's posterior share.  ``logits`` fp32 [R, A], ``answers`` int64 [G], ``valid`` int32
    [R], ``log_weights`` fp32 [R] or None (uniform), ``group_start`` int32 [G + 1] (``hypothesis_rows.group_start``: from 0 to
    R, non-decreasing), all on the device.  Returns ``loss`` [G] -- ``INVALID_PROGRAM_LOSS``, without a gradient, where no
    row of the question counts -- and, not differentiable, ``log_posterior`` fp32 [R], the rows' own answers int64 [R],
    ``support`` and ``consistent_count`` int32 [G].  The weights get no gradient (the kernel has no slot for it): a
    ``log_weights`` that requires one is an error."""

    @staticmethod
    def forward(ctx, logits, answers, valid, log_weights, group_start, answer_weight, unknown_index):
        from probnmn import _hip

        if log_weights is not None and ctx.needs_input_grad[3]:
            raise ValueError("the marginal answer loss gives no gradient to log_weights (module training holds the program "
                             "generator frozen): detach them")
        logits = logits.contiguous()
        R, A = logits.shape
        G = answers.numel()
        dev = logits.device
        f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        d_logits = torch.zeros(R, A, **f)  # (a row that no group covers is not written)
        log_posterior, log_evidence = torch.full((R,), -float("inf"), **f), torch.empty(G, **f)
        predictions = torch.full((R,), unknown_index, dtype=torch.long, device=dev)
        support, consistent = torch.empty(G, **i), torch.empty(G, **i)
        if R == 0 or G == 0:  # (no row anywhere: what the kernel writes for a group without rows)
            log_evidence.fill_(-float("inf")), support.zero_(), consistent.zero_()
        else:
            _hip.check(_hip.lib().pnmn_answer_posterior(
                logits.data_ptr(), valid.data_ptr(), 0 if log_weights is None else log_weights.data_ptr(), answers.data_ptr(),
                group_start.data_ptr(), float(answer_weight), d_logits.data_ptr(), predictions.data_ptr(),
                log_posterior.data_ptr(), log_evidence.data_ptr(), 0, support.data_ptr(), consistent.data_ptr(), 0, G, R, A,
                unknown_index, _hip.stream_ptr(dev)), "answer_posterior (gradient mode)")
        loss = torch.where(support > 0, -log_evidence, torch.full_like(log_evidence, INVALID_PROGRAM_LOSS))
        # the question of every row: how many groups end at or before it
        question_of_row = torch.searchsorted(group_start[1:].long(), torch.arange(R, device=dev), right=True).clamp_(max=max(G - 1, 0))
        ctx.save_for_backward(d_logits, question_of_row)
        ctx.mark_non_differentiable(log_posterior, predictions, support, consistent)
        return loss, log_posterior, predictions, support, consistent

    @staticmethod
    def backward(ctx, dloss, *_):
        d_logits, question_of_row = ctx.saved_tensors
        return d_logits * dloss[question_of_row].unsqueeze(1), None, None, None, None, None, None


class NeuralModuleNetwork(nn.Module):
    def __init__(
        self,
        vocabulary,
        image_feature_size: Tuple[int, int, int] = (1024, 14, 14),
        module_channels: int = 128,
        class_projection_channels: int = 1024,
        classifier_linear_size: int = 1024,
    ):
        super().__init__()
        self.vocabulary = vocabulary
        channels, height, width = image_feature_size
        # "@@UNKNOWN@@" is never produced by the classifier (reference nmn.py:60-63)
        num_answers = len(vocabulary.get_index_to_token_vocabulary(namespace="answers")) - 1

        self.stem = nn.Sequential(
            nn.Conv2d(channels, module_channels, kernel_size=3, padding=1),
            nn.ReLU(),
            nn.Conv2d(module_channels, module_channels, kernel_size=3, padding=1),
            nn.ReLU(),
        )
        self.classifier = nn.Sequential(
            nn.Conv2d(module_channels, class_projection_channels, kernel_size=1),
            nn.ReLU(),
            nn.MaxPool2d(kernel_size=2, stride=2),
            Flatten(),
            nn.Linear(class_projection_channels * height * width // 4, classifier_linear_size),
            nn.ReLU(),
            nn.Linear(classifier_linear_size, num_answers),
        )

        # one child module per program token, named by the token (reference nmn.py:86-115)
        self._function_modules: Dict[str, Optional[nn.Module]] = {}
        factories = {pc.AND: AndModule, pc.OR: OrModule}
        sized = {pc.CMP: ComparisonModule, pc.QUERY: QueryModule, pc.REL: RelateModule,
                 pc.SAME: SameModule, pc.ATT: AttentionModule}
        for token in vocabulary.get_token_to_index_vocabulary("programs"):
            kind = pc.classify_token(token)
            if kind == pc.SKIP:
                continue
            if kind == pc.SCENE:
                module = None
            elif kind in factories:
                module = factories[kind]()
            else:
                module = sized[kind](module_channels)
            self._function_modules[token] = module
            self.add_module(token, module)

        self._unknown_answer = vocabulary.get_token_index("@@UNKNOWN@@", namespace="answers")
        self._answer_accuracy = BooleanAccuracy()
        self._average_invalid_programs = Average()
        # reference behaviour: every training forward returns batch metrics as Python floats, which
        # costs a device->host sync per step; trainers that log less often switch this off
        self.report_batch_metrics = True

        from probnmn.runtime.engine import NMNEngine

        self._engine = NMNEngine(self, tuple(image_feature_size), module_channels, class_projection_channels)

    @classmethod
    def from_config(cls, config):
        from probnmn.vocabulary import Vocabulary

        _C = config
        return cls(
            vocabulary=Vocabulary.from_files(_C.DATA.VOCABULARY),
            image_feature_size=tuple(_C.NMN.IMAGE_FEATURE_SIZE),
            module_channels=_C.NMN.MODULE_CHANNELS,
            class_projection_channels=_C.NMN.CLASS_PROJECTION_CHANNELS,
            classifier_linear_size=_C.NMN.CLASSIFIER_LINEAR_SIZE,
        )

    @property
    def engine(self):
        return self._engine

    def forward(self, features: torch.Tensor, programs: torch.Tensor, answers: Optional[torch.Tensor] = None,
                started=None, trunk_stream=None, rows: Optional[torch.Tensor] = None, return_attention: bool = False,
                return_logits: bool = False):
        # ``started``: token of ``begin(features)`` when the caller already launched the stem (optional)
        # ``rows``: run on ``features[rows]`` (programs / answers belong to those examples) without the gathered copy
        # ``trunk_stream``: run the trunk (stem, module programs, classifier conv + pool -- this build's own
        # kernels, none of which waits for another workgroup) on that stream, forward and backward, beside
        # whatever the caller queues on the current stream; the fully connected layers and the loss stay on
        # the current stream (see DESIGN 6 for why the library GEMMs must not leave it)
        # ``return_attention``: the output dict gains "attention" [B, T, H, W] -- the one-channel map each program token's
        # module wrote, zeros where there is none -- and "attention_mask" [B, T] (``NMNEngine.attention_maps``); detached
        # ``return_logits``: the output dict gains "answer_logits" [B, A], what the classifier's last layer gave for every
        # program, invalid ones included ("predictions" and "loss" apply the invalid-program overrides, these do not)
        return self.forward_head(self.forward_trunk(features, programs, started, trunk_stream, rows, return_attention), answers,
                                 return_logits)

    def forward_trunk(self, features: torch.Tensor, programs: torch.Tensor, started=None, trunk_stream=None,
                      rows: Optional[torch.Tensor] = None, return_attention: bool = False):
        """First half of ``forward``: compile and schedule the programs, launch the trunk (on ``trunk_stream`` when
        given).  Nothing is queued on the current stream, so a caller that runs the trunk on its own stream can
        keep feeding the current one before ``forward_head`` makes it wait for the trunk."""
        engine = self._engine
        arena = engine.ensure_arena()
        if rows is not None and started is None:
            started = self.begin(features, rows)
        # the programs decide the launch schedule, so they are needed on the host (the reference
        # also reads them back, once per example: nmn.py:203)
        # (a CPU ``programs`` tensor costs nothing; a device tensor costs one device->host sync)
        tokens = programs.detach().cpu().numpy()
        compiled = _Tokens(tokens)

        # the trunk's parameters as inputs of its autograd node -- all of them when autograd is to receive
        # their gradients; ONE anchor when a trainer reads the gradients straight from the arena
        # (engine.direct_grads): 218 inputs cost ~0.5 ms of host time per step in apply() and in 218
        # AccumulateGrad visits that carry nothing
        params = [arena.param(n) for n in arena.names]
        if engine.direct_grads:
            params = params[:1]
        if trunk_stream is not None:
            with torch.cuda.stream(trunk_stream):
                pooled = _Trunk.apply(features, engine, compiled, started, *params)
                if return_attention:  # (queued right behind the trunk, on its stream)
                    compiled.attention = engine.attention_maps(tokens.shape[1])
        else:
            pooled = _Trunk.apply(features, engine, compiled, started, *params)
            if return_attention:
                compiled.attention = engine.attention_maps(tokens.shape[1])
        return pooled, compiled, trunk_stream

    def _answer_logits(self, trunk):
        """The fully connected layers on a trunk pass, on the current stream: (answer logits [B, A], the validity of every
        program as a host list and as an int32 device tensor)."""
        from probnmn import _hip

        pooled, compiled, trunk_stream = trunk
        # (staged here, not in forward_trunk: the host's time between the sampled programs' arrival and the trunk's
        # launch is on the critical path of a small-batch step)
        valid_host = compiled.valid.tolist()
        valid = _hip.small_to_device(valid_host, torch.int32, pooled.device)
        self._engine.wait_params(pooled.device)  # (an optimiser step of the FC layers still running on the trunk's stream)
        if trunk_stream is not None:
            current = torch.cuda.current_stream(pooled.device)
            current.wait_stream(trunk_stream)
            pooled.record_stream(current)
            for t in compiled.attention or ():
                t.record_stream(current)
        hidden = F.relu(_first_fc(self.classifier[4], pooled))
        answer_logits = self.classifier[6](hidden)
        _hip.mark("classifier FC forward done")
        if answer_logits.requires_grad:
            answer_logits.register_hook(lambda g: _hip.mark("d(answer logits) arrives"))
            pooled.register_hook(lambda g: _hip.mark("d(pooled) computed (FC backward done)"))
        return answer_logits, valid_host, valid

    def forward_head(self, trunk, answers: Optional[torch.Tensor] = None, return_logits: bool = False):
        """Second half of ``forward``: the fully connected layers and the loss, on the current stream."""
        compiled = trunk[1]
        answer_logits, valid_host, valid = self._answer_logits(trunk)

        # log-softmax, arg-max, cross entropy (or -max log-probability without answers) and the
        # invalid-program overrides -- prediction @@UNKNOWN@@, constant loss 3.33, no gradient -- in one kernel
        if answers is not None:
            answers = answers.contiguous()
        loss, answer_predictions = _AnswerLoss.apply(answer_logits, answers, valid, self._unknown_answer)
        if answers is not None and (self.report_batch_metrics or not self.training):
            self._answer_accuracy(answer_predictions, answers)
            self._average_invalid_programs(sum(1 for v in valid_host if not v))

        output_dict = {"predictions": answer_predictions, "loss": loss}
        if compiled.attention is not None:
            output_dict["attention"], output_dict["attention_mask"] = compiled.attention
        if return_logits:
            output_dict["answer_logits"] = answer_logits.detach()
        if self.training and self.report_batch_metrics:
            output_dict["metrics"] = self.get_metrics(reset=True)
        return output_dict

    def _hypothesis_arguments(self, features, programs: torch.Tensor, question_rows):
        """The argument checks ``marginal_answers``, ``answer_posterior`` and ``marginal_answer_loss`` share.  Returns (device,
        G, R, A, programs [R, T] on the host, question_rows as host int64 [R])."""
        from probnmn import hypothesis_rows

        dev = features.device
        G = int(features.size(0))
        programs = programs.detach().cpu()
        qrows = hypothesis_rows.on_host(question_rows)
        R = int(qrows.size)
        if programs.dim() != 2 or programs.size(0) != R or qrows.ndim != 1:
            raise ValueError("programs [R, T] and question_rows [R]; got %s and %s" % (tuple(programs.shape), qrows.shape))
        hypothesis_rows.check(qrows, G)
        return dev, G, R, self.classifier[6].out_features, programs, qrows

    @staticmethod
    def _given_answers(features, answers, answer_weight):
        """The ``answers`` / ``answer_weight`` checks of ``answer_posterior`` and ``marginal_answer_loss``: (the weight as a
        finite float, the given answers as a detached integer tensor [G])."""
        import math

        try:
            w_a = float(answer_weight)
        except (TypeError, ValueError):
            raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
        if not math.isfinite(w_a):
            raise ValueError("answer_weight must be a finite number, got %r" % (answer_weight,))
        given = torch.as_tensor(answers).detach()
        if given.dim() != 1 or given.size(0) != int(features.size(0)) or given.dtype.is_floating_point or given.dtype == torch.bool:
            raise ValueError("answers int64 [%d]; got %s %s" % (int(features.size(0)), given.dtype, tuple(given.shape)))
        return w_a, given

    def _hypothesis_logits(self, features, programs: torch.Tensor, question_rows, max_rows: int):
        """The row loop of ``marginal_answers`` and ``answer_posterior``: their argument checks, then the NMN over the R
        hypothesis rows in passes of at most ``max_rows``, each row reading its question's feature map where it lies
        (``rows=`` / ``ResidentRows.subset``).  Returns (device, G, R, A, question_rows as host int64 [R], answer logits
        fp32 [R, A], validity int32 [R] -- both on the device)."""
        from probnmn import _hip
        from probnmn.data.feature_store import ResidentRows

        if max_rows < 1:
            raise ValueError("max_rows must be at least 1, got %r" % (max_rows,))
        dev, G, R, A, programs, qrows = self._hypothesis_arguments(features, programs, question_rows)
        logits = torch.empty(R, A, dtype=torch.float32, device=dev)
        valid = torch.empty(R, dtype=torch.int32, device=dev)
        resident = isinstance(features, ResidentRows)
        rows_dev = None if resident or R == 0 else _hip.to_device(qrows, dev).view(torch.long)
        for lo in range(0, R, max_rows):
            hi = min(lo + max_rows, R)
            if resident:
                trunk = self.forward_trunk(features.subset(qrows[lo:hi]), programs[lo:hi])
            else:
                trunk = self.forward_trunk(features, programs[lo:hi], rows=rows_dev[lo:hi])
            logits[lo:hi], _, valid[lo:hi] = self._answer_logits(trunk)
        return dev, G, R, A, qrows, logits, valid

    @torch.no_grad()
    def marginal_answers(self, features, programs: torch.Tensor, question_rows, log_weights=None, max_rows: int = 1024):
        """The answer of every question from SEVERAL programs: p(a | x, image) = sum_z q(z | x) p(a | z, image) over the
        hypotheses given for it (not in the reference, which answers from one program: nmn.py:245-269).  Evaluation only,
        no gradient.

        ``features``: the G questions' feature maps -- an NCHW or ``channels_last`` tensor, or a ``ResidentRows`` batch.
        ``programs`` [R, T] (host or device): the hypotheses.  ``question_rows`` [R], non-decreasing, in 0 .. G - 1:
        hypothesis r belongs to question ``question_rows[r]``; a question may have none.  ``log_weights`` [R]:
        unnormalised log q(z | x) of each hypothesis (None: uniform); the weights are renormalised over the hypotheses of
        a question that are valid programs and have a finite weight.

        The NMN runs over the R hypothesis rows in passes of at most ``max_rows`` (the engine has ONE activation arena),
        reading each row's feature map where it lies (``rows=`` / ``ResidentRows.subset``: nothing is gathered, but the
        stem runs once per hypothesis row, not once per question); then ONE ``pnmn_answer_marginal`` launch.

        Returns ``"predictions"`` int64 [G] (@@UNKNOWN@@ where no hypothesis counts), ``"log_probabilities"`` fp32 [G, A]
        (-inf there), ``"hypothesis_predictions"`` int64 [R] (each hypothesis's own answer), ``"hypothesis_weights"``
        fp32 [R] (0 for one that does not count) and ``"support"`` int32 [G] (how many count)."""
        from probnmn import _hip, hypothesis_rows

        dev, G, R, A, qrows, logits, valid = self._hypothesis_logits(features, programs, question_rows, max_rows)
        weights = None if log_weights is None else hypothesis_rows.row_vector(log_weights, "log_weights", R, dev)
        group_start = hypothesis_rows.group_start_on_device(qrows, G, dev)
        out = {"predictions": torch.empty(G, dtype=torch.long, device=dev),
               "log_probabilities": torch.empty(G, A, dtype=torch.float32, device=dev),
               "hypothesis_predictions": torch.empty(R, dtype=torch.long, device=dev),
               "hypothesis_weights": torch.empty(R, dtype=torch.float32, device=dev),
               "support": torch.empty(G, dtype=torch.int32, device=dev)}
        _hip.check(_hip.lib().pnmn_answer_marginal(
            logits.data_ptr(), valid.data_ptr(), 0 if weights is None else weights.data_ptr(), group_start.data_ptr(),
            out["log_probabilities"].data_ptr(), out["predictions"].data_ptr(), out["hypothesis_predictions"].data_ptr(),
            out["hypothesis_weights"].data_ptr(), out["support"].data_ptr(), G, R, A, self._unknown_answer,
            _hip.stream_ptr(dev)), "answer_marginal")
        return out

    @torch.no_grad()
    def answer_posterior(self, features, programs: torch.Tensor, question_rows, answers, log_weights=None,
                         answer_weight: float = 1.0, max_rows: int = 1024):
        """The posterior over every question's program hypotheses GIVEN ITS ANSWER (not in the reference, which uses
        p(a | z, image) to answer from one program and never to judge the program):
            log p(z_r | x, a, image) = log w_r + answer_weight * log p(a | z_r, image) - log of the sum over the question's rows
        with w_r the renormalised weight a hypothesis has before the answer is seen.  Inference only, no gradient.

        ``features``, ``programs`` [R, T], ``question_rows`` [R], ``max_rows``: as for ``marginal_answers``.  ``answers`` [G]
        (host or device, int64): the given answer of each question; one that is no index into the answers rules every
        hypothesis out (unless ``answer_weight`` is 0).  ``log_weights`` [R]: unnormalised log q(z | x) of each hypothesis, or
        ``hypothesis_posterior``'s ``"log_posterior"`` -- with which, and ``answer_weight`` 1, the result is the posterior
        under the whole generative model p(z) p(x | z) p(a | z, image) on the candidate set -- (None: uniform), renormalised
        over the hypotheses of a question that are valid programs and have a finite weight.  ``answer_weight``: a finite
        number; exactly 0 leaves the answer term out.

        The NMN runs over the R hypothesis rows exactly as in ``marginal_answers`` (the stem runs once per hypothesis row);
        then ONE ``pnmn_answer_posterior`` launch (the rule: include/probnmn_hip.h).  No metric moves, and the ``train()`` /
        ``eval()`` state is not touched.

        Returns device tensors: ``"log_answer_likelihood"`` fp32 [R] (log p(a | z_r, image), of every row), ``"log_posterior"``
        fp32 [R] (-inf for a hypothesis that does not count: an invalid program, a weight or a score that is not finite),
        ``"hypothesis_predictions"`` int64 [R] (each hypothesis's own answer; @@UNKNOWN@@ for an invalid program);
        ``"log_evidence"`` fp32 [G] (with ``answer_weight`` 1: log p(a | x, image) on the candidate set; -inf where no
        hypothesis counts), ``"best_row"`` int32 [G] (the MAP hypothesis's row, first of equals; -1 there),
        ``"first_consistent_row"`` int32 [G] (the first counting hypothesis whose own answer is the given one; -1 when there
        is none), ``"consistent_count"`` int32 [G] (how many there are) and ``"support"`` int32 [G] (how many count)."""
        from probnmn import _hip, hypothesis_rows

        w_a, given = self._given_answers(features, answers, answer_weight)
        dev, G, R, A, qrows, logits, valid = self._hypothesis_logits(features, programs, question_rows, max_rows)
        weights = None if log_weights is None else hypothesis_rows.row_vector(log_weights, "log_weights", R, dev)
        given = given.to(device=dev, dtype=torch.long).contiguous()
        group_start = hypothesis_rows.group_start_on_device(qrows, G, dev)
        f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        out = {"log_answer_likelihood": torch.empty(R, **f), "log_posterior": torch.empty(R, **f),
               "hypothesis_predictions": torch.empty(R, dtype=torch.long, device=dev), "log_evidence": torch.empty(G, **f),
               "best_row": torch.empty(G, **i), "first_consistent_row": torch.empty(G, **i),
               "consistent_count": torch.empty(G, **i), "support": torch.empty(G, **i)}
        if R == 0 or G == 0:  # (no row anywhere: what the kernel writes for a group without rows)
            out["log_evidence"].fill_(-float("inf"))
            out["best_row"].fill_(-1), out["first_consistent_row"].fill_(-1)
            out["consistent_count"].zero_(), out["support"].zero_()
            return out
        _hip.check(_hip.lib().pnmn_answer_posterior(
            logits.data_ptr(), valid.data_ptr(), 0 if weights is None else weights.data_ptr(), given.data_ptr(),
            group_start.data_ptr(), w_a, out["log_answer_likelihood"].data_ptr(), out["hypothesis_predictions"].data_ptr(),
            out["log_posterior"].data_ptr(), out["log_evidence"].data_ptr(), out["best_row"].data_ptr(), out["support"].data_ptr(),
            out["consistent_count"].data_ptr(), out["first_consistent_row"].data_ptr(), G, R, A, self._unknown_answer,
            _hip.stream_ptr(dev)), "answer_posterior")
        return out

    def marginal_answer_loss(self, features, programs: torch.Tensor, question_rows, answers, log_weights=None,
                             answer_weight: float = 1.0):
        """The marginal likelihood of every question's answer over its program hypotheses, as a loss to TRAIN the modules on
        (the maximum marginal likelihood objective of weakly supervised semantic parsing; not in the reference, which pays
        the cross entropy of one sampled program: nmn.py:245-269):
            loss[g] = -log sum_r w_r p(a_g | z_r, image)^answer_weight        over the hypothesis rows r of question g
        with w_r the renormalised weight of a hypothesis.  Its gradient reaches a row's answer logits as that row's
        cross-entropy gradient scaled by its posterior share p(z_r | x, a, image): a hypothesis that explains the answer is
        trained on, one that does not is left alone.

        ``features``, ``programs`` [R, T], ``question_rows`` [R], ``answers`` [G], ``log_weights`` [R], ``answer_weight``: the
        arguments of ``answer_posterior``, under its rules.  The weights receive NO gradient (a ``log_weights`` tensor that
        requires one is a ``ValueError``): the candidate set and its weights are given.

        The NMN runs over the R hypothesis rows in ONE pass with gradient tracking -- there is no ``max_rows``: the engine
        has one activation arena and backward needs it intact -- each row reading its question's feature map where it lies
        (``rows=`` / ``ResidentRows.subset``; the stem runs once per hypothesis row); then ONE ``pnmn_answer_posterior``
        launch in gradient mode gives the loss and d loss / d logits.  No metric moves, and the ``train()`` / ``eval()``
        state is not touched.

        Returns ``"loss"`` fp32 [G] (differentiable; ``INVALID_PROGRAM_LOSS`` = 3.33, without a gradient, for a question
        none of whose hypotheses counts) and, detached, ``"log_posterior"`` fp32 [R] (-inf for a hypothesis that does not
        count), ``"hypothesis_predictions"`` int64 [R], ``"support"`` and ``"consistent_count"`` int32 [G]."""
        from probnmn import _hip, hypothesis_rows
        from probnmn.data.feature_store import ResidentRows

        w_a, given = self._given_answers(features, answers, answer_weight)
        if torch.is_tensor(log_weights) and log_weights.requires_grad:
            raise ValueError("marginal_answer_loss gives no gradient to log_weights (the candidate set and its weights are "
                             "given): detach them")
        dev, G, R, A, programs, qrows = self._hypothesis_arguments(features, programs, question_rows)
        weights = None if log_weights is None else hypothesis_rows.row_vector(log_weights, "log_weights", R, dev)
        if R == 0 or G == 0:  # (no row anywhere: nothing to run the network on, every question pays the constant)
            i = dict(dtype=torch.int32, device=dev)
            return {"loss": torch.full((G,), INVALID_PROGRAM_LOSS, dtype=torch.float32, device=dev),
                    "log_posterior": torch.empty(0, dtype=torch.float32, device=dev),
                    "hypothesis_predictions": torch.empty(0, dtype=torch.long, device=dev),
                    "support": torch.zeros(G, **i), "consistent_count": torch.zeros(G, **i)}
        given = given.to(device=dev, dtype=torch.long).contiguous()
        group_start = hypothesis_rows.group_start_on_device(qrows, G, dev)
        if isinstance(features, ResidentRows):
            trunk = self.forward_trunk(features.subset(qrows), programs)
        else:
            trunk = self.forward_trunk(features, programs, rows=_hip.to_device(qrows, dev).view(torch.long))
        logits, _, valid = self._answer_logits(trunk)
        loss, log_posterior, predictions, support, consistent = _MarginalAnswerLoss.apply(
            logits, given, valid, weights, group_start, w_a, self._unknown_answer)
        return {"loss": loss, "log_posterior": log_posterior, "hypothesis_predictions": predictions, "support": support,
                "consistent_count": consistent}

    def answer_log_likelihood(self, features, programs: torch.Tensor, question_rows, answers):
        """log p(a_g | z_r, image_g) of every hypothesis row r of question g, WITH a graph: what a loss over a question's
        candidate programs that also trains the program generator (``sequence_marginal_loss``, ``MarginalJointStep``) takes
        as a row's answer term (not in the reference, which scores one sampled program per question: nmn.py:245-269).

        ``features``, ``programs`` [R, T], ``question_rows`` [R], ``answers`` [G]: the arguments of ``marginal_answer_loss``,
        under its rules.  The NMN runs over the R hypothesis rows in ONE pass with gradient tracking, as there: each row
        reads its question's feature map where it lies, the stem runs once per hypothesis row.  The row's value is the
        negative of the loss ``forward`` computes for that program and its question's answer (``pnmn_answer_loss``: the
        same launch, the same gradient); a row whose program is invalid gets -inf and no gradient -- it is no candidate.
        No metric moves, and the ``train()`` / ``eval()`` state is not touched.

        Returns ``"log_answer"`` fp32 [R] (differentiable) and, detached, ``"hypothesis_predictions"`` int64 [R] (each
        hypothesis's own answer; @@UNKNOWN@@ for an invalid program)."""
        from probnmn import _hip
        from probnmn.data.feature_store import ResidentRows

        _, given = self._given_answers(features, answers, 1.0)
        dev, G, R, A, programs, qrows = self._hypothesis_arguments(features, programs, question_rows)
        if R == 0 or G == 0:  # (no row anywhere: nothing to run the network on)
            return {"log_answer": torch.empty(0, dtype=torch.float32, device=dev),
                    "hypothesis_predictions": torch.empty(0, dtype=torch.long, device=dev)}
        rows_dev = _hip.to_device(qrows, dev).view(torch.long)
        row_answers = given.to(device=dev, dtype=torch.long).index_select(0, rows_dev).contiguous()
        if isinstance(features, ResidentRows):
            trunk = self.forward_trunk(features.subset(qrows), programs)
        else:
            trunk = self.forward_trunk(features, programs, rows=rows_dev)
        logits, _, valid = self._answer_logits(trunk)
        loss, predictions = _AnswerLoss.apply(logits, row_answers, valid, self._unknown_answer)
        log_answer = torch.where(valid != 0, -loss, torch.full_like(loss, -float("inf")))
        return {"log_answer": log_answer, "hypothesis_predictions": predictions}

    def hypothesis_answer_logits(self, features, programs: torch.Tensor, question_rows):
        """The answer logits of every hypothesis row, WITH a graph and without a loss: what a loss that weighs a question's
        programs itself takes (``joint_importance_weighted_bound``, whose kernel computes log p(a | z, image) and its
        gradient from them).  Not in the reference, which scores one sampled program per question (nmn.py:245-269).

        ``features``, ``programs`` [R, T], ``question_rows`` [R]: the arguments of ``marginal_answer_loss``, under its rules.
        The NMN runs over the R hypothesis rows in ONE trunk pass with gradient tracking, as in ``answer_log_likelihood``:
        each row reads its question's feature map where it lies, the stem runs once per hypothesis row.  No metric moves,
        and the ``train()`` / ``eval()`` state is not touched.

        Returns ``"answer_logits"`` fp32 [R, A] (differentiable) and ``"valid"`` int32 [R] (0 for a row whose program is
        invalid: its logits mean nothing)."""
        from probnmn import _hip
        from probnmn.data.feature_store import ResidentRows

        dev, G, R, A, programs, qrows = self._hypothesis_arguments(features, programs, question_rows)
        if R == 0 or G == 0:  # (no row anywhere: nothing to run the network on)
            return {"answer_logits": torch.empty(0, A, dtype=torch.float32, device=dev),
                    "valid": torch.empty(0, dtype=torch.int32, device=dev)}
        if isinstance(features, ResidentRows):
            trunk = self.forward_trunk(features.subset(qrows), programs)
        else:
            trunk = self.forward_trunk(features, programs, rows=_hip.to_device(qrows, dev).view(torch.long))
        logits, _, valid = self._answer_logits(trunk)
        return {"answer_logits": logits, "valid": valid}

    def begin(self, features: torch.Tensor, rows: Optional[torch.Tensor] = None):
        """Launch the program-independent part of ``forward`` (feature layout + stem) ahead of time;
        pass the returned token as ``forward(..., started=token)`` with the same ``features``.  ``rows`` (int64
        device tensor): the pass runs on ``features[rows]`` -- programs / answers of ``forward`` then belong to
        those examples -- without the gathered copy of the feature maps."""
        # (what ``_Trunk.forward`` will ask ``run_forward_tokens`` for: ``ctx.needs_input_grad`` reports ``requires_grad``
        # whatever the grad mode, so under ``torch.no_grad()`` a token begun for "no backward" was refused there)
        trains = any(p.requires_grad for p in self.parameters())
        return self._engine.begin_forward(features, trains, rows)

    def get_metrics(self, reset: bool = True) -> Dict[str, float]:
        return {
            "answer_accuracy": self._answer_accuracy.get_metric(reset=reset),
            "average_invalid": self._average_invalid_programs.get_metric(reset=reset),
        }
