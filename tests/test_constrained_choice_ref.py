"""The host reference of the grammar-constrained token choice (tests/helpers/constrained_choice.py) that the GPU tests
measure against, held to the rule's own consequences without a device: free running through the fp64 decoder emulation every
row is a valid program (where the unconstrained reference emits invalid ones), the trivial automaton constrains nothing, and
the reference leaves few rows of the GPU test's inputs ambiguous."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import constrained_choice as cc  # noqa: E402
import filtered_inputs as fi  # noqa: E402
from filtered_choice import filtered_sample_ref, kernel_uniform  # noqa: E402

PAD, UNK, START, END = fi.PAD, fi.UNK, fi.START, 3
V = 44
IDENTITY = (1.0, 0, 1.0)
SHAPES = [(1, 1, 1), (7, 5, 3), (17, 12, 20), (64, 12, 20), (130, 9, 27), (33, 2, 5), (33, 30, 40)]  # (B, T, S)


@pytest.fixture(scope="module")
def grammar():
    """(compiler, automaton, its tables) of the CLEVR program vocabulary: V = 44, end = 3, 11 states x 6 classes."""
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    assert vocab.get_vocab_size("programs") == V and vocab.get_token_index("@end@", namespace="programs") == END
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    auto = comp.decoding_automaton(exclude=(PAD, UNK, START, END))
    return comp, auto, cc.Tables(auto, END)


def free_run(tab, d, B, T, seed, row_offset, filt, greedy=False):
    """The reference free running through the fp64 decoder emulation: (tokens [B, T], logits [B * T, V], the allowed set of
    every (row, step) [B * T, V]).  ``tab`` None: the unconstrained reference."""
    rows = row_offset + np.arange(B, dtype=np.uint64)
    run = {"s": np.zeros(B, np.int64), "f": np.zeros(B, bool), "tok": [], "mask": []}

    def choose(logits, t):
        u = kernel_uniform(seed, rows, t)
        if tab is None:
            tok = filtered_sample_ref(logits, u, PAD, UNK, START, *filt)[0]
        else:
            mask = cc.allowed_mask(tab, run["s"], run["f"], t, T, V, PAD, UNK, START)
            assert mask.any(1).all()  # (A_c is never empty)
            tok = cc.constrained_greedy_ref(logits, mask)[0] if greedy else \
                cc.constrained_sample_ref(logits, u, mask, PAD, UNK, START, *filt)[0]
            assert mask[np.arange(B), tok].all()
            run["s"], run["f"] = cc.advance(tab, run["s"], run["f"], tok)
            run["mask"].append(mask)
        run["tok"].append(tok)
        return tok

    z = fi.emulate_decoder_logits(d, T, choose)
    masks = np.stack(run["mask"], 1).reshape(B * T, V) if tab is not None else None
    return np.stack(run["tok"], 1), z, masks


def _valid(comp, auto, tokens):
    return [auto.accepts(cc.cut_at_end(row, END)) and comp.compile(cc.cut_at_end(row, END)).valid for row in tokens]


@pytest.mark.parametrize("B,T,S", SHAPES)
def test_every_free_running_row_is_a_valid_program(grammar, B, T, S):
    comp, auto, tab = grammar
    d = fi.decoder_inputs(B, S, V, B + T + S + V)
    invalid_unconstrained = 0
    for filt, seed, row_offset in [(IDENTITY, 99, 16)] + fi.decoder_filter_cases():
        tokens, _, _ = free_run(tab, d, B, T, seed, row_offset, filt)
        assert all(_valid(comp, auto, tokens)), (filt, seed)
        for row in tokens:  # after a row's first end: end
            row = row.tolist()
            assert END not in row or set(row[row.index(END):]) == {END}
        plain, _, _ = free_run(None, d, B, T, seed, row_offset, filt)
        invalid_unconstrained += len(plain) - sum(_valid(comp, auto, plain))
    tokens, _, _ = free_run(tab, d, B, T, 0, 0, IDENTITY, greedy=True)
    assert all(_valid(comp, auto, tokens))
    assert invalid_unconstrained > 0  # (the inputs discriminate: the same seeds unconstrained leave invalid rows)


@pytest.mark.parametrize("B,T,S", [s for s in SHAPES if s[0] >= 7])
def test_the_trivial_automaton_reproduces_the_unconstrained_reference(B, T, S):
    tab, _ = cc.trivial_tables(V, END)
    d = fi.decoder_inputs(B, S, V, B + T + S + V)
    for filt, seed, row_offset in [(IDENTITY, 99, 16)] + fi.decoder_filter_cases()[:2]:
        got, _, _ = free_run(tab, d, B, T, seed, row_offset, filt)
        want, _, _ = free_run(None, d, B, T, seed, row_offset, filt)
        for g, w in zip(got.tolist(), want.tolist()):
            n = w.index(END) + 1 if END in w else T  # up to and including the row's first end
            assert g[:n] == w[:n] and set(g[n:]) <= {END}


def test_the_allowed_set_follows_the_rule(grammar):
    comp, auto, tab = grammar
    T = 6
    for t in range(T):
        for s in range(auto.n_states):
            mask = cc.allowed_mask(tab, [s], [False], t, T, V, PAD, UNK, START)[0]
            for v in range(V):
                if v == END:
                    want = auto.min_left[s] == 0
                else:
                    want = v not in (PAD, UNK, START) and auto.min_left[auto.next_state[s, auto.token_class[v]]] <= T - 1 - t
                assert mask[v] == want, (t, s, v)
            done = cc.allowed_mask(tab, [s], [True], t, T, V, PAD, UNK, START)[0]
            assert np.flatnonzero(done).tolist() == [END]
    s, f = cc.advance(tab, [0, 0, 4], [False, False, True], [END, 7, 9])
    assert s.tolist() == [0, int(auto.next_state[0, auto.token_class[7]]), 4] and f.tolist() == [True, False, True]


def test_greedy_reference_is_the_first_largest_logit_inside_the_set():
    z = np.array([[9.0, 1.0, 5.0, 5.0, 2.0], [np.nan, 1.0, np.nan, 0.0, 3.0], [1.0, 2.0, 3.0, 4.0, 5.0]])
    mask = np.array([[False, True, True, True, False], [False, True, True, True, True], [True, False, False, False, False]])
    tok, gap = cc.constrained_greedy_ref(z, mask)
    assert tok.tolist() == [2, 2, 0]
    assert gap[0] == 0.0 and np.isnan(gap[1]) and gap[2] == np.inf


@pytest.mark.parametrize("filt", [IDENTITY] + fi.FILTERS)
def test_the_reference_leaves_few_rows_ambiguous_on_the_gpu_tests_inputs(grammar, filt):
    """The GPU test excuses at most 5 % (+ 5) of a case's rows; the reference itself needs at most 2.5 % on exactly those
    inputs (the fp64 emulation of the decoder under the reference's own draws: the device's rows up to round-off), as a
    share of the LIVE (row, step) pairs: a finished row emits end whatever the logits are.  The shapes of 1 and 35 rows have
    no percentage and are pooled with the rest."""
    comp, auto, tab = grammar
    cases = [(IDENTITY, 99, 16)] + fi.decoder_filter_cases()
    pooled_n = pooled_rows = 0
    for B, T, S in SHAPES:
        d = fi.decoder_inputs(B, S, V, B + T + S + V)
        for f, seed, row_offset in cases:
            if f != filt:
                continue
            tokens, z, masks = free_run(tab, d, B, T, seed, row_offset, filt)
            rows = row_offset + np.arange(B, dtype=np.uint64)
            u = kernel_uniform(seed, rows[:, None], np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
            _, margin, _ = cc.constrained_sample_ref(z, u, masks, PAD, UNK, START, *filt)
            n = int((margin < fi.DECODER_DELTA).sum())
            live = int((~cc.states_of(tab, tokens)[1]).sum())
            print("decoder %dx%d S=%d filter=%s: %d of %d live rows within %g" % (B, T, S, filt, n, live, fi.DECODER_DELTA))
            if B * T not in (1, 35):
                assert n <= 0.025 * live, (B, T, S, filt, n, live)
            pooled_n, pooled_rows = pooled_n + n, pooled_rows + live
    assert pooled_n <= 0.025 * pooled_rows, (filt, pooled_n, pooled_rows)


def test_python_layer_refuses_bad_constrained_calls(grammar):
    """Every check below comes before the first device call."""
    import torch

    from probnmn.evaluators import predict_answers
    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    comp, auto, _ = grammar
    model = ProgramGenerator(Vocabulary.clevr(), max_decoding_steps=12)
    q = torch.zeros(2, 5, dtype=torch.long)
    for strategy in ("constrained_sampling", "constrained_greedy"):
        with pytest.raises(ValueError):
            model(q, decoding_strategy=strategy)  # no constraint
        with pytest.raises(ValueError):
            model(q, q, decoding_strategy=strategy, constraint=auto)  # target tokens
        with pytest.raises(ValueError):
            model.decode({}, decoding_strategy=strategy)
    with pytest.raises(ValueError):
        model(q, decoding_strategy="constrained_greedy", constraint=auto, top_k=3)
    with pytest.raises(ValueError):
        model.decode_constrained({}, auto, greedy=True, temperature=0.5)
    with pytest.raises(ValueError):
        model.decode_constrained({}, None)
    for strategy in ("sampling", "greedy"):  # (the old refusal stays)
        with pytest.raises(ValueError):
            model(q, decoding_strategy=strategy, constraint=auto)
    with pytest.raises(ValueError):
        predict_answers(None, None, [], None, beam_size=4, constrained_sampling=True)
    with pytest.raises(ValueError):
        predict_answers(None, None, [], None, constrained=True)
    from probnmn import _hip

    for name in ("pnmn_attn_lstm_fwd", "pnmn_attn_lstm_fwd_group", "pnmn_attn_lstm_beam"):
        assert name in _hip.SIGNATURES
        assert name + "_constrained" not in _hip.SIGNATURES  # (an option is an argument, not a second entry point)
