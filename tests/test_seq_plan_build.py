"""The build of the seq2seq launch plan (probnmn.runtime.seq_plan) on the CPU, against a stand-in for the library that
records calls: every prepared call matches its prototype of the header, every pointer it holds (directly or inside a record
passed by address) lies in memory the plan keeps alive, each loss backward has the forward it belongs to, and the launch
order of an iteration is the one written out below."""
import ctypes

import numpy as np
import pytest
import torch

DERIVED = ("l0.hh", "l0.hhT", "l0.b", "l1.hh", "l1.hhT", "l1.b", "l1.ih", "l1.ihT", "d.c", "d.hh", "d.cT", "d.hhT", "d.b")
LISTS = ("fwd_pg_enc", "fwd_pg", "fwd_pg_finish", "fwd_qr", "fwd_prior", "bwd_a", "bwd_b")


class StandInLibrary:
    """Any entry point: records its call; a ``*_bytes`` query answers a positive size, a launch succeeds."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def entry(*args):
            self.log.append((name, args))
            return 4096 if name.endswith("_bytes") else 0
        return entry


def build_plan(monkeypatch, dropout, stack, n=24, m=7, tq=20, tp=12, lib=None):
    from probnmn import _hip
    from probnmn.models import ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.modules.seq2seq_base import Seq2SeqBase
    from probnmn.runtime import seq_plan
    from probnmn.vocabulary import Vocabulary

    lib = lib or StandInLibrary()

    def derived(model):
        return model.__dict__.setdefault("_stand_in_derived", {k: torch.zeros(16) for k in DERIVED})

    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "stream_ptr", lambda dev: 0)
    monkeypatch.setattr(_hip, "decoder_workspace_bytes", lambda rows, backward: 4096)
    monkeypatch.setattr(Seq2SeqBase, "_derived", derived)
    monkeypatch.setattr(ProgramPrior, "_derived", derived)
    monkeypatch.setattr(seq_plan, "USE_STACK", stack)
    vocab = Vocabulary.clevr()
    models = [ProgramGenerator(vocab, dropout=dropout), QuestionReconstructor(vocab, dropout=dropout), ProgramPrior(vocab, hidden_size=256)]
    models[2].eval()  # (as the trainers keep it)
    return seq_plan.Seq2SeqPlan(*models, torch.device("cpu"), n, m, tq, tp), models, lib


def regions(plan, models):
    """name -> (first byte, size) of everything a call of the plan may point into."""
    out = {name: t for name, t in plan._bufs.items()}
    for tag, mm in (("pg", plan.pg), ("qr", plan.qr)):
        out[tag + ".gflat"] = mm.gflat
    for tag, model in zip(("pg", "qr", "pr"), models):
        out.update({"%s.param.%s" % (tag, k): p for k, p in model.named_parameters()})
        out.update({"%s.derived.%s" % (tag, k): t for k, t in model._derived().items()})
    out = {name: (t.data_ptr(), t.numel() * t.element_size()) for name, t in out.items()}
    out.update({"record%d" % i: (r.ctypes.data, r.nbytes) for i, r in enumerate(plan._keep + [plan.pair_jobs])})
    return out


def resolve(where, pointer):
    hits = [(name, pointer - lo) for name, (lo, size) in where.items() if lo <= pointer < lo + size]
    assert hits, "pointer %#x lies in nothing the plan keeps" % pointer
    return min(hits, key=lambda h: h[1])  # (a gradient view lies in its gflat: one answer, the innermost)


def calls_of(plan, lib, name):
    """(entry point, argument tuple) of a call list; an ``add_fn`` closure is run against the stand-in to see its call."""
    out = []
    for fn, args, entry in getattr(plan, name):
        if not args:
            del lib.log[:]
            assert fn() == 0 and len(lib.log) == 1 and lib.log[0][0] == entry
            args = lib.log[0][1]
        out.append((entry, args))
    return out


def expected_order(drop, stack):
    """An iteration's launches, list by list (entry points without their ``pnmn_`` prefix)."""
    stack_fwd = ["lstm_stack_fwd_dropout" if drop else "lstm_stack_fwd"]
    layers = ["lstm_seq_fwd"] + ["lstm_dropout"] * drop + ["gemm_cus", "lstm_seq_fwd"]  # a launch per layer, the input product between
    layers_bwd = ["lstm_seq_bwd", "gemm_cus"] + ["lstm_dropout"] * drop + ["lstm_seq_bwd"]
    table_grads = ["embedding_grad", "token_table_bwd"]
    return {
        "fwd_pg_enc": ["token_prep", "token_table_fwd"] + (stack_fwd if stack else layers) + ["mask_last_fwd"],
        "fwd_pg": ["token_prep", "token_table_fwd", "attn_lstm_fwd_group", "trim_predictions"],
        "fwd_pg_finish": ["gemm_cus", "seq_nll_fwd", "seq_nll_fwd"],
        # (the reconstructor's encoder and the prior's in one launch; per layer, the prior's layers drop nothing)
        "fwd_qr": ["token_rows", "token_prep", "token_table_fwd", "token_prep", "token_table_fwd"]
                  + (stack_fwd if stack else layers + ["lstm_seq_fwd", "gemm_cus", "lstm_seq_fwd"])
                  + ["mask_last_fwd", "token_prep", "token_table_fwd", "attn_lstm_fwd_group", "gemm_cus", "seq_nll_fwd"],
        "fwd_prior": ["gemm_cus", "gemm_cus", "seq_nll_fwd"],
        "bwd_a": ["seq_nll_bwd"] * 3 + ["gemm_cus", "attn_lstm_bwd_group"] + ["attn_denc"] * 3,
        # (the generator's decoder table takes two passes' gate gradients)
        "bwd_b": ["mask_last_bwd"] * 2 + layers_bwd * 2 + ["embedding_grad"] + table_grads * 4 + ["gemm_cus"] * 3,
    }


@pytest.mark.parametrize("stack", [True, False])
@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_plan_build(monkeypatch, dropout, stack):
    from probnmn import _hip

    plan, models, lib = build_plan(monkeypatch, dropout, stack)
    where = regions(plan, models)
    calls = {name: calls_of(plan, lib, name) for name in LISTS}
    for name in LISTS:
        assert [entry[len("pnmn_"):] for entry, _ in calls[name]] == expected_order(dropout > 0, stack)[name], name
        for entry, args in calls[name]:
            kinds = _hip.SIGNATURES[entry]
            assert len(args) == len(kinds), entry
            for a, kind in zip(args, kinds):
                if kind is ctypes.c_void_p:
                    assert a is None or type(a) is int, (entry, a)
                    if a:
                        resolve(where, a)
                else:
                    assert type(a) is (float if kind in (ctypes.c_float, ctypes.c_double) else int), (entry, a)
    for rec in plan._keep + [plan.pair_jobs]:
        for field in rec.dtype.names:
            if rec.dtype[field] == np.uint64:  # (pointer fields, and the seeds an iteration sets: zero in a fresh plan)
                for pointer in rec[field][rec[field] != 0]:
                    resolve(where, int(pointer))
    if dropout == 0.0 and stack:
        assert sum(map(len, calls.values())) == 54 and len(plan._bufs) == 125
    # a loss's backward is the backward of one of the forward losses: logits, strides, tokens, padding, lse, shape and eps
    forward = [a[:7] + a[8:13] for name in LISTS[:5] for entry, a in calls[name] if entry == "pnmn_seq_nll_fwd"]
    backward = [a[:8] + a[11:15] for entry, a in calls["bwd_a"] if entry == "pnmn_seq_nll_bwd"]
    assert len(forward) == 4 and len(backward) == 3 and all(b in forward for b in backward)
