"""Prior sampling without a device: the host references on the very inputs of tests/test_prior_sample_gpu.py leave at most
half as many rows ambiguous as the GPU tests may excuse, and the argument checks of ``ProgramPrior.sample`` /
``sample_programs``, which all come before the first device call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import constrained_choice as cc  # noqa: E402
import filtered_inputs as fi  # noqa: E402
import prior_inputs as pi  # noqa: E402
from filtered_choice import filtered_sample_ref, kernel_uniform  # noqa: E402

PAD, UNK, START, END = pi.PAD, pi.UNK, pi.START, pi.END


@pytest.mark.parametrize("B,T,V", pi.SHAPES)
def test_the_reference_leaves_few_rows_ambiguous_on_the_gpu_tests_inputs(B, T, V):
    """The GPU test excuses at most ``excused_cap(rows)`` rows of a case; the reference itself, on the same prior run in fp64 on
    the host under its own draws (the device's rows up to round-off), must need at most half of that."""
    w = pi.prior_weights(B, T, V)
    for filt, seed, row_offset in pi.prior_filter_cases(V):
        rows = row_offset + np.arange(B, dtype=np.uint64)
        z, _, _ = pi.emulate_prior_logits(
            w, B, T, lambda logits, t: filtered_sample_ref(logits, kernel_uniform(seed, rows, t), PAD, UNK, START, *filt)[0])
        _, margin, _ = filtered_sample_ref(z, pi.uniforms(seed, row_offset, B, T), PAD, UNK, START, *filt)
        n = int((margin < fi.DECODER_DELTA).sum())
        spread = float(z.std(1).mean())
        print("prior %dx%d V=%d filter=%s: %d of %d rows within %g (half cap %d); mean logit spread %.2f" % (
            B, T, V, filt, n, B * T, fi.DECODER_DELTA, fi.excused_cap(B * T) // 2, spread))
        assert n <= fi.excused_cap(B * T) // 2, (B, T, V, filt, n)


def _grammar():
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    assert vocab.get_vocab_size("programs") == 44 and vocab.get_token_index("@end@", namespace="programs") == END
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    auto = comp.decoding_automaton(exclude=(PAD, UNK, START, END))
    return vocab, comp, auto


@pytest.mark.parametrize("B,T", pi.CONSTRAINED_SHAPES)
def test_the_constrained_reference_leaves_few_rows_ambiguous(B, T):
    _, comp, auto = _grammar()
    tab = cc.Tables(auto, END)
    T = pi.shortest_steps(tab.min_left) if T is None else T
    V = 44
    w = pi.prior_weights(B, T, V)
    for filt, seed, row_offset in pi.constrained_cases():
        if filt is None:
            continue  # (a greedy row has no margin: the GPU test holds it to validity)
        rows = row_offset + np.arange(B, dtype=np.uint64)
        run = {"state": np.zeros(B, np.int64), "finished": np.zeros(B, bool), "margin": []}

        def choose(logits, t):
            mask = cc.allowed_mask(tab, run["state"], run["finished"], t, T, V, PAD, UNK, START)
            tok, margin, _ = cc.constrained_sample_ref(logits, kernel_uniform(seed, rows, t), mask, PAD, UNK, START, *filt)
            run["state"], run["finished"] = cc.advance(tab, run["state"], run["finished"], tok)
            run["margin"].append(margin)
            return tok

        _, _, tok = pi.emulate_prior_logits(w, B, T, choose)
        n = int((np.stack(run["margin"], 1) < fi.DECODER_DELTA).sum())
        print("constrained prior %dx%d filter=%s: %d of %d rows within %g" % (B, T, filt, n, B * T, fi.DECODER_DELTA))
        assert n <= fi.excused_cap(B * T) // 2, (B, T, filt, n)
        for row in tok.tolist():
            assert comp.compile(cc.cut_at_end(row, END)).valid, row


def test_sample_refuses_values_out_of_range_before_any_device_call():
    from probnmn.evaluators import sample_programs
    from probnmn.models import ProgramPrior

    vocab, comp, auto = _grammar()
    prior = ProgramPrior(vocab, hidden_size=256).eval()  # on the CPU
    bad = [dict(temperature=0.0), dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5),
           dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(greedy=True, top_k=5)]
    for kw in bad:
        with pytest.raises(ValueError):
            prior.sample(4, 28, **kw)
        with pytest.raises(ValueError):
            sample_programs(prior, vocab, 4, **kw)
    with pytest.raises(ValueError):  # tables of another vocabulary
        prior.sample(4, 28, constraint=cc.trivial_tables(40, END)[1])
    with pytest.raises(ValueError):  # no accepted string fits the steps
        long = cc.trivial_tables(44, END)[1]
        long.min_left = np.array([30], np.uint8)
        prior.sample(4, 28, constraint=long)
    with pytest.raises(ValueError):
        sample_programs(prior, vocab, 4, constrained=True)
    # a CPU model keeps the torch loop, which has none of the options
    for kw in (dict(seed=5), dict(top_k=5), dict(temperature=0.7), dict(constraint=auto), dict(greedy=True)):
        with pytest.raises(NotImplementedError):
            prior.sample(4, 28, **kw)
    with pytest.raises(NotImplementedError):
        prior.sample(2, 5, torch.full((2, 4), 9), seed=5)
    out = prior.sample(3, 6)  # ... and still samples as before
    assert sorted(out) == ["loss", "predictions"] and out["predictions"].shape == (3, 5)
    out = prior.sample(2, 5, torch.tensor([[9, 9, END, 9], [END, 9, 9, 9]]))
    assert sorted(out["predictions"].tolist()) == [[0, 0, 0, 0], [9, 9, END, 0]]
