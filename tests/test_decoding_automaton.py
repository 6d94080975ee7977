"""``ProgramCompiler.decoding_automaton``: the left-to-right automaton the constrained beam kernel decodes under accepts
exactly what the program compiler calls valid, its ``min_left`` is the true shortest completion, and the host reference
of the constrained search (tests/helpers/constrained_beam_reference.py) -- pinned here on its own, no GPU -- returns only
finite, valid hypotheses on a model whose unconstrained best program is never valid."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import beam_reference as br  # noqa: E402
import constrained_beam_reference as cbr  # noqa: E402

from oracle.seq2seq_oracle import END, PAD, START, UNK  # noqa: E402
from probnmn.runtime import program_compiler as pc  # noqa: E402
from probnmn.vocabulary import Vocabulary  # noqa: E402

EXCLUDE = (PAD, UNK, START, END)
NEG = float("-inf")


@pytest.fixture(scope="module")
def vocab():
    return Vocabulary.clevr()


@pytest.fixture(scope="module", params=[128, 8])
def compiler(request, vocab):
    return pc.ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"), module_channels=request.param)


def _accepts(auto, tokens):
    """Run the three tables by hand (not ``DecodingAutomaton.accepts``): state 0, one step per token, accepting iff min_left == 0."""
    s = 0
    for t in tokens:
        s = int(auto.next_state[s, auto.token_class[t]])
    return int(auto.min_left[s]) == 0


def _random_strings(V, count, seed):
    rng = np.random.Generator(np.random.Philox(seed))
    lengths = rng.integers(0, 9, count)
    soup = rng.integers(0, V, (count, 8))
    return soup, lengths


def test_shape_and_dtype_contracts(compiler, vocab):
    auto = compiler.decoding_automaton(exclude=EXCLUDE)
    V = vocab.get_vocab_size("programs")
    n_states, n_classes = auto.next_state.shape
    assert auto.token_class.shape == (V,) and auto.min_left.shape == (n_states,)
    for a in (auto.token_class, auto.next_state, auto.min_left):
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"] and not a.flags["WRITEABLE"]
    assert 1 <= n_states <= 32 and 1 <= n_classes <= 16
    assert n_states == 11 and n_classes <= 8  # six register states reversed and determinised, the dead state included
    assert int(auto.token_class.max()) < n_classes and int(auto.next_state.max()) < n_states
    assert int(auto.min_left[0]) == 0  # the empty program is valid
    assert (auto.n_states, auto.n_classes) == (n_states, n_classes)
    with pytest.raises(AttributeError):
        auto.min_left = auto.min_left
    with pytest.raises(ValueError):
        auto.min_left[0] = 1
    # cached on the compiler, per set of excluded tokens
    assert compiler.decoding_automaton(exclude=list(EXCLUDE)) is auto
    assert compiler.decoding_automaton(exclude=EXCLUDE[::-1]) is auto
    assert compiler.decoding_automaton() is compiler.decoding_automaton(exclude=())
    # exactly one dead state, and it is a sink
    dead = [s for s in range(n_states) if int(auto.min_left[s]) == 255]
    assert len(dead) == 1 and bool((auto.next_state[dead[0]] == dead[0]).all())
    # tokens of one kind share a class; pad / unk / start / end behave like any skipped token
    for kind in range(9):
        assert len({int(auto.token_class[t]) for t in range(V) if compiler.kinds[t] == kind}) <= 1
    assert len({int(auto.token_class[t]) for t in EXCLUDE}) == 1


def test_limits_are_enforced():
    ok = pc.DecodingAutomaton([0, 1], [[0, 1], [1, 1]], [0, 255])
    assert ok.accepts([0, 0]) and not ok.accepts([1]) and not ok.accepts([5])
    for bad in (dict(token_class=[0], next_state=np.zeros((33, 1)), min_left=np.zeros(33)),
                dict(token_class=[0], next_state=np.zeros((1, 17)), min_left=[0]),
                dict(token_class=[0], next_state=np.zeros((0, 1)), min_left=[]),
                dict(token_class=[2], next_state=[[0, 0]], min_left=[0]),      # class out of range
                dict(token_class=[0], next_state=[[1]], min_left=[0]),         # state out of range
                dict(token_class=[0], next_state=[[0], [0]], min_left=[0])):   # min_left of the wrong length
        with pytest.raises(ValueError):
            pc.DecodingAutomaton(**bad)
    # a grammar that needs more than the kernel's tables hold is refused when it is built
    saved = pc.MAX_AUTOMATON_STATES
    pc.MAX_AUTOMATON_STATES = 4
    try:
        with pytest.raises(ValueError, match="at most"):
            pc.ProgramCompiler(Vocabulary.clevr().get_index_to_token_vocabulary("programs")).decoding_automaton()
    finally:
        pc.MAX_AUTOMATON_STATES = saved


def test_every_string_over_one_token_per_kind_up_to_length_six(compiler):
    auto = compiler.decoding_automaton(exclude=EXCLUDE)
    reps = [compiler.kinds.index(kind) for kind in range(9)]  # (SKIP: @@PADDING@@)
    n = n_valid = 0
    for length in range(7):
        for s in itertools.product(reps, repeat=length):
            want = compiler._compile(s).valid
            assert _accepts(auto, s) == want, s
            n += 1
            n_valid += want
    assert n == sum(9 ** i for i in range(7)) and 1000 < n_valid < n // 2


def test_random_strings_against_the_python_rules(compiler, vocab):
    auto = compiler.decoding_automaton(exclude=EXCLUDE)
    soup, lengths = _random_strings(vocab.get_vocab_size("programs"), 200000, 17)
    disagree = n_valid = 0
    for row, n in zip(soup.tolist(), lengths.tolist()):
        want = compiler._compile(tuple(row[:n])).valid
        disagree += _accepts(auto, row[:n]) != want
        n_valid += want
    assert disagree == 0
    assert 2000 < n_valid < 100000  # both verdicts are exercised
    assert auto.accepts(soup[0, : lengths[0]].tolist()) == _accepts(auto, soup[0, : lengths[0]].tolist())


def test_random_strings_against_the_native_host_compiler(compiler, vocab):
    """The same sample through ``compile_batch`` (pnmn_compile_programs), right-padded: padding is a skipped token."""
    auto = compiler.decoding_automaton(exclude=EXCLUDE)
    soup, lengths = _random_strings(vocab.get_vocab_size("programs"), 200000, 17)
    soup = np.where(np.arange(8)[None, :] < lengths[:, None], soup, PAD)
    # all 200 000 rows in one vectorised pass over the tables
    state = np.zeros(len(soup), np.int64)
    for t in range(8):
        state = auto.next_state[state, auto.token_class[soup[:, t]]].astype(np.int64)
    got = auto.min_left[state] == 0
    want = np.asarray([p.valid for p in compiler.compile_batch(soup)])
    assert int((got != want).sum()) == 0 and 2000 < int(want.sum()) < 100000


@pytest.mark.parametrize("fixture", ["nmn_validity.json", "nmn_validity_28.json"])
def test_the_reference_interpreters_verdicts(golden_dir, vocab, fixture):
    with open(os.path.join(golden_dir, fixture)) as f:
        table = json.load(f)
    comp = pc.ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"), module_channels=8)
    auto = comp.decoding_automaton(exclude=EXCLUDE)
    assert len(table) >= 20 and 0 < sum(bool(v) for v in table.values()) < len(table)
    for case, valid in table.items():
        ids = [vocab.get_token_index(t, "programs") for t in case.split()]
        assert _accepts(auto, ids) == bool(valid), case
        assert _accepts(auto, ids + [END, PAD, PAD]) == bool(valid), case


def test_gold_programs_are_accepted(compiler, vocab):
    from probnmn.data.synthetic import synthetic_batch

    auto = compiler.decoding_automaton(exclude=EXCLUDE)
    for row in synthetic_batch(vocab, 300, seed=5, with_image=False)["program"].tolist():
        assert _accepts(auto, row), row


def test_min_left_is_the_shortest_completion(compiler, vocab):
    """Breadth-first over TOKENS (not classes) from every state, the excluded ones left out; and what excluding does: a
    state that only @end@-like tokens could complete has no completion."""
    V = vocab.get_vocab_size("programs")
    for exclude in (EXCLUDE, (), tuple(t for t in range(V) if compiler.kinds[t] == pc.SCENE) + EXCLUDE):
        auto = compiler.decoding_automaton(exclude=exclude)
        n_states = auto.next_state.shape[0]
        emit = [t for t in range(V) if t not in exclude]
        accepting = {s for s in range(n_states) if compiler.decoding_automaton().min_left[s] == 0}
        for s0 in range(n_states):
            frontier, seen, depth, found = {s0}, {s0}, 0, None
            while frontier:
                if frontier & accepting:
                    found = depth
                    break
                frontier = {int(auto.next_state[s, auto.token_class[t]]) for s in frontier for t in emit} - seen
                seen |= frontier
                depth += 1
            assert int(auto.min_left[s0]) == (255 if found is None else found), (exclude, s0)
    # without `scene` only programs of skipped tokens are valid: every other live state is cut off
    assert sorted(set(auto.min_left.tolist())) == [0, 255]


# ---- the reference search on its own ------------------------------------------------------------------------------------
STEPS = 12


@pytest.fixture(scope="module")
def fixture_model(vocab):
    """The trained generator of tests/test_beam_gpu.py (seed 0, 100 host Adam steps on the synthetic task), the 128
    sources of seed 1234, the automaton and a compiler to judge with."""
    from probnmn.models import ProgramGenerator

    v_src, v_tgt = vocab.get_vocab_size("questions"), vocab.get_vocab_size("programs")
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, max(1, threads)))
    try:
        torch.manual_seed(0)
        fresh = {k: v.detach().clone() for k, v in ProgramGenerator(vocab, max_decoding_steps=STEPS).state_dict().items()}
        trained = br.train_on_host(fresh, v_src, v_tgt, steps=100, rows=64)
    finally:
        torch.set_num_threads(threads)
    src = br.synthetic_task(v_src, v_tgt, 128, torch.Generator().manual_seed(1234))[0]
    comp = pc.ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    return trained, src, comp.decoding_automaton(exclude=EXCLUDE), comp


def _valid(comp, tokens):
    return np.asarray([comp.compile(row).valid for row in tokens.reshape(-1, tokens.size(-1)).tolist()])


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
def test_reference_search_returns_only_valid_programs(fixture_model, K):
    sd, src, auto, comp = fixture_model
    out = cbr.beam_search(sd, src, K, STEPS, auto.token_class, auto.next_state, auto.min_left)
    assert out["tokens"].shape == (128, K, STEPS)
    assert bool(torch.isfinite(out["scores"]).all()), "every hypothesis is finite"
    assert bool(_valid(comp, out["tokens"]).all()), "every hypothesis is valid"
    assert bool((auto.min_left[out["states"].numpy()] == 0).all())
    assert not bool(((out["tokens"] == PAD) | (out["tokens"] == UNK) | (out["tokens"] == START)).any())
    assert bool((out["scores"][:, :-1] >= out["scores"][:, 1:]).all())  # best first
    # the K hypotheses of a question are different programs
    for b in range(128):
        assert len({tuple(r) for r in out["tokens"][b].tolist()}) == K
    # the fixture's premise: without the constraint the best program of every question is invalid
    free = br.beam_search(sd, src, K, STEPS)
    assert not bool(_valid(comp, free["tokens"][:, 0]).any())
    # replaying the search's own trace gives the search's tables
    tables = cbr.replay(sd, src, out["trace_tokens"], out["trace_backptr"], auto.token_class, auto.next_state, auto.min_left)
    for t, cand in enumerate(tables):
        tok, bp, sc, _ = br.select(cand, K)
        assert torch.equal(tok, out["trace_tokens"][:, t]) and torch.equal(bp, out["trace_backptr"][:, t])
        assert torch.equal(sc, out["trace_scores"][:, t])
    print("reference K=%d: %d/128 questions below the margin 1e-4 * T" % (K, int((out["margin"] < 1e-4 * STEPS).sum())))


@pytest.mark.parametrize("T", [1, 2, 3])
def test_reference_search_at_the_shortest_horizons(fixture_model, vocab, T):
    """The step budget decides almost every token.  The valid programs of at most T tokens are counted by brute force
    with the compiler: a beam holds min(K, that many) finite hypotheses, all valid, the best in slot 0."""
    sd, src, auto, comp = fixture_model
    emit = [t for t in range(vocab.get_vocab_size("programs")) if t not in EXCLUDE]
    n_programs = sum(comp._compile(s).valid for n in range(T + 1) for s in itertools.product(emit, repeat=n))
    assert n_programs >= 2  # the empty program, and `unique`
    free = br.beam_search(sd, src, 1, T)  # (cut this short, a few of the model's best programs happen to be valid)
    assert not bool(_valid(comp, free["tokens"][:, 0]).all()), "fixture: the constraint changes nothing at this horizon"
    for K in (1, 2, 16):
        out = cbr.beam_search(sd, src, K, T, auto.token_class, auto.next_state, auto.min_left)
        finite = torch.isfinite(out["scores"])
        assert bool((finite.sum(1) == min(K, n_programs)).all()), (T, K, n_programs)
        assert bool(finite[:, 0].all())
        assert bool(_valid(comp, out["tokens"])[finite.reshape(-1).numpy()].all())
        assert bool((out["scores"][~finite] == NEG).all())
        # replaying the search's own trace gives the search's tables: an empty slot stays empty in the later steps
        given = out["trace_scores"] > NEG
        for live in (None, given):
            tables = cbr.replay(sd, src, out["trace_tokens"], out["trace_backptr"], auto.token_class, auto.next_state,
                                auto.min_left, live=live)
            for t, cand in enumerate(tables):
                tok, bp, sc, _ = br.select(cand, K)
                assert torch.equal(tok, out["trace_tokens"][:, t]) and torch.equal(bp, out["trace_backptr"][:, t])
                assert torch.equal(sc, out["trace_scores"][:, t])


def test_a_trivial_automaton_changes_nothing(fixture_model):
    sd, src, _, _ = fixture_model
    V = sd["_output_projection_layer.weight"].size(0)
    for K in (1, 4):
        free = br.beam_search(sd, src[:32], K, STEPS)
        same = cbr.beam_search(sd, src[:32], K, STEPS, np.zeros(V, np.uint8), [[0]], [0])
        for key in ("tokens", "scores", "trace_tokens", "trace_backptr", "trace_scores", "margin"):
            assert torch.equal(free[key], same[key]), key
