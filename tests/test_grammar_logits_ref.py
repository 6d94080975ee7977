"""The grammar-normalised distribution q_c without a device: the host reference of ``pnmn_grammar_logits``
(tests/helpers/grammar_logits_reference.py) held to the rule's own consequences -- q_c sums to one over the valid programs of
the horizon, every string in its support compiles, the teacher-forced @end@ behind a full-length program is free -- the
reference's own properties, the binding of the extension header, and the argument rules of the strategy and the trainers."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import constrained_choice as cc  # noqa: E402
import filtered_inputs as fi  # noqa: E402
import grammar_logits_reference as gr  # noqa: E402

PAD, UNK, START, END = fi.PAD, fi.UNK, fi.START, 3
V = 44


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


@pytest.fixture(scope="module")
def leaves(grammar):
    """horizon -> the support of q_c (``enumerate_leaves``), computed once."""
    _, _, tab = grammar
    return {h: gr.enumerate_leaves(tab, h, V, PAD, UNK, START, seed=5) for h in (2, 3, 4)}


@pytest.mark.parametrize("horizon", [2, 3, 4])
def test_q_c_sums_to_one_over_valid_programs(grammar, leaves, horizon):
    comp, auto, tab = grammar
    found = leaves[horizon]
    assert len({lf[0] for lf in found}) == len(found)
    if horizon in (2, 3):
        assert len(found) == {2: 11, 3: 298}[horizon]
    total = np.exp(np.array([lf[1] for lf in found])).sum()
    assert abs(total - 1.0) <= 1e-12, total
    for tokens, _, ended in found:
        program = cc.cut_at_end(tokens, END)
        assert len(program) <= horizon and (ended or len(tokens) == horizon)
        assert auto.accepts(program) and comp.compile(program).valid, tokens


@pytest.mark.parametrize("horizon", [2, 3, 4])
def test_reference_scores_the_leaves_as_the_enumeration_does(grammar, leaves, horizon):
    """The leaves teacher forced through ``grammar_logits_ref``, one step longer than the horizon: the same log q_c, the
    appended @end@ of a full-length program at t >= horizon costs nothing, and no leaf has a token outside its set."""
    _, _, tab = grammar
    found = leaves[horizon]
    T = horizon + 1
    tokens = np.full((len(found), T), PAD, np.int64)
    logits = np.zeros((len(found), T, V))
    for i, (toks, _, ended) in enumerate(found):
        row = list(toks) + ([] if ended else [END])
        tokens[i, :len(row)] = row
        for t in range(T):
            logits[i, t] = gr.prefix_logits(tuple(row[:t]), V, seed=5)
    masked, sets, log_mass, outside = gr.grammar_logits_ref(logits, tokens, tab, horizon, PAD, UNK, START)
    assert (outside == 0).all()
    step = gr.log_softmax_at(masked, tokens) * (tokens != PAD)
    np.testing.assert_allclose(step.sum(1), [lf[1] for lf in found], rtol=0, atol=1e-12)
    full = np.array([not lf[2] for lf in found])
    assert full.any() and (step[full, horizon] == 0.0).all()       # the @end@ behind `horizon` tokens: log-probability 0
    assert (sets[full, horizon].sum(1) == 1).all() and sets[full, horizon, END].all()
    assert (log_mass <= 0).all() and np.isfinite(masked).any(2).all()
    # per step q_c >= q: the lse over the set is at most the lse over the row
    plain = gr.log_softmax_at(logits, tokens) * (tokens != PAD)
    assert (step >= plain - 1e-12).all()
    np.testing.assert_allclose(plain.sum(1), (step + log_mass * (tokens != PAD)).sum(1), rtol=0, atol=1e-10)


def _random_rows(tab, B, T, horizon, seed):
    """Rows a constrained sampler could emit (a uniform walk through the allowed sets), @end@ repeated behind the first."""
    rng = np.random.default_rng(seed)
    s, f = np.zeros(B, np.int64), np.zeros(B, bool)
    tokens = np.zeros((B, T), np.int64)
    for t in range(T):
        mask = cc.allowed_mask(tab, s, f, t, horizon, V, PAD, UNK, START)
        assert mask.any(1).all()
        tokens[:, t] = [rng.choice(np.flatnonzero(m)) for m in mask]
        s, f = cc.advance(tab, s, f, tokens[:, t])
    return tokens


def test_reference_properties(grammar):
    _, auto, tab = grammar
    rng = np.random.default_rng(3)
    B, T = 12, 9
    tokens = _random_rows(tab, B, T, T, 11)
    logits = rng.normal(0, 3, (B, T, V))
    masked, sets, log_mass, outside = gr.grammar_logits_ref(logits, tokens, tab, T, PAD, UNK, START)
    assert (outside == 0).all()                                    # rows a constrained sample could be
    assert all(auto.accepts(cc.cut_at_end(row, END)) for row in tokens)
    assert np.isfinite(masked).any(2).all() and (log_mass <= 0).all() and (log_mass < 0).any()
    assert (masked[sets] == logits[sets]).all() and np.isneginf(masked[~sets]).all()
    # the trimmed rows (padding behind the first @end@) score the same and are still inside
    trimmed = tokens.copy()
    for row in trimmed:
        ends = np.flatnonzero(row == END)
        if ends.size:  # (a program of all T tokens has no @end@ in the row)
            row[ends[0] + 1:] = PAD
    assert (gr.grammar_logits_ref(logits, trimmed, tab, T, PAD, UNK, START)[3] == 0).all()
    # one illegal token mid-row: @start@ is in no allowed set; the step stays finite and the token is in its set
    bad = tokens.copy()
    live = np.flatnonzero((bad[:, :2] != END).all(1))
    assert live.size
    bad[live, 1] = START
    m2, s2, lm2, out2 = gr.grammar_logits_ref(logits, bad, tab, T, PAD, UNK, START)
    assert (out2[live] > 0).all() and s2[live, 1, START].all() and np.isfinite(m2).any(2).all() and (lm2 <= 0).all()
    # a row longer than the horizon
    assert (tokens[:, :4] != END).all(1).any()
    out3 = gr.grammar_logits_ref(logits, tokens, tab, 4, PAD, UNK, START)[3]
    assert (out3[(tokens[:, :4] != END).all(1)] > 0).all()
    # a token outside [0, V): counted, added to no set, the state left alone
    far = tokens.copy()
    far[:, 0] = V + 5
    m4, s4, lm4, out4 = gr.grammar_logits_ref(logits, far, tab, T, PAD, UNK, START)
    assert (out4 > 0).all() and np.isfinite(m4).any(2).all()
    first_set = cc.allowed_mask(tab, np.zeros(B, np.int64), np.zeros(B, bool), 0, T, V, PAD, UNK, START)
    still_start = cc.allowed_mask(tab, np.zeros(B, np.int64), np.zeros(B, bool), 1, T, V, PAD, UNK, START)
    still_start[np.arange(B), tokens[:, 1]] = True
    assert (s4[:, 0] == first_set).all() and (s4[:, 1] == still_start).all()
    neg = tokens.copy()
    neg[:, 2] = -1
    assert (gr.grammar_logits_ref(logits, neg, tab, T, PAD, UNK, START)[3] >= 0).all()
    # an all-padding row: pad is never counted; every step finite
    pads = np.full((2, T), PAD, np.int64)
    m5, _, lm5, out5 = gr.grammar_logits_ref(logits[:2], pads, tab, T, PAD, UNK, START)
    assert (out5 == 0).all() and np.isfinite(m5).any(2).all() and (lm5 <= 0).all()
    # the trivial automaton removes pad / unk / start alone
    triv, _ = cc.trivial_tables(V, END)
    _, s6, _, out6 = gr.grammar_logits_ref(logits, tokens, triv, T, PAD, UNK, START)
    first = s6[:, 0]
    assert (first.sum(1) == V - 3).all() and not first[:, [PAD, UNK, START]].any() and (out6 == 0).all()


def test_an_empty_set_is_copied_unmasked():
    """A state without completion and a token outside [0, V): nothing is allowed and nothing joins, so the step is the
    logits' own and its log_mass exactly 0."""
    auto = SimpleNamespace(token_class=np.zeros(7, np.uint8), next_state=np.array([[1], [1]], np.uint8),
                           min_left=np.array([1, 255], np.uint8))
    tab = cc.Tables(auto, 3)
    logits = np.random.default_rng(0).normal(0, 1, (1, 3, 7))
    tokens = np.array([[4, 99, 99]])
    masked, sets, log_mass, outside = gr.grammar_logits_ref(logits, tokens, tab, 3, PAD, UNK, START)
    assert sets[0, 1].all() and sets[0, 2].all() and (masked[0, 1:] == logits[0, 1:]).all()
    assert (log_mass[0, 1:] == 0.0).all() and outside[0] == 3


def test_extension_header_reads_and_leaves_the_core_binding_alone():
    import ctypes

    from probnmn import _hip, _hip_grammar

    assert _hip.ABI_VERSION == 14 and len(_hip.SIGNATURES) == 103
    sigs, restypes, records, constants = _hip.read_header(_hip_grammar.HEADER_PATH)
    assert set(sigs) == {"pnmn_grammar_logits", "pnmn_grammar_logits_bwd"} and not records and not constants
    assert not set(sigs) & set(_hip.SIGNATURES) and "pnmn_grammar_logits" not in _hip.SIGNATURES
    assert len(sigs["pnmn_grammar_logits"]) == 22 and len(sigs["pnmn_grammar_logits_bwd"]) == 20
    assert all(r is ctypes.c_int for r in restypes.values())
    fwd = sigs["pnmn_grammar_logits"]
    assert [i for i, t in enumerate(fwd) if t is ctypes.c_int64] == [1, 3, 5]
    assert all(fwd[i] is ctypes.c_void_p for i in (0, 2, 4, 6, 7, 16, 17, 18, 21)) and fwd[8:16] == (ctypes.c_int,) * 8
    lib = _hip_grammar.lib()
    assert lib is _hip.lib() and lib.pnmn_grammar_logits.argtypes == list(fwd)


def test_entry_points_are_bound_and_check_their_arguments_without_a_device(grammar):
    from probnmn import _hip, _hip_grammar
    from probnmn.modules.seq2seq_base import constraint_tables

    _, auto, _ = grammar
    lib = _hip_grammar.lib()
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)
    good = constraint_tables(auto, V, END)

    def tables(tc=None, ns=None, ml=None):
        tc, ns, ml = (good[0] if tc is None else tc), (good[1] if ns is None else ns), (good[2] if ml is None else ml)
        return dict(tc=tc.ctypes.data, ns=ns.ctypes.data, ml=ml.ctypes.data, n_states=ns.shape[0], n_classes=ns.shape[1], keep=(tc, ns, ml))

    def forward(x=p, tokens=p, y=p, B=2, T=3, Vv=V, horizon=5, end=END, t=None, **over):
        t = dict(tables() if t is None else t, **over)
        return lib.pnmn_grammar_logits(x, Vv * T, tokens, T, y, Vv * T, 0, 0, B, T, Vv, horizon, PAD, UNK, START, end,
                                       t["tc"], t["ns"], t["ml"], t["n_states"], t["n_classes"], 0)

    def backward(x=p, tokens=p, y=p, B=2, T=3, Vv=V, horizon=5, end=END, t=None, **over):
        t = dict(tables() if t is None else t, **over)
        return lib.pnmn_grammar_logits_bwd(x, Vv * T, tokens, T, y, Vv * T, B, T, Vv, horizon, PAD, UNK, START, end,
                                           t["tc"], t["ns"], t["ml"], t["n_states"], t["n_classes"], 0)

    for call in (forward, backward):
        for missing in ("x", "tokens", "y"):
            assert call(**{missing: 0}) == _hip.EINVAL, missing
        for missing in ("tc", "ns", "ml"):                                  # some but not all tables, and none
            assert call(**{missing: 0}) == _hip.EINVAL, missing
        assert call(tc=0, ns=0, ml=0) == _hip.EINVAL
        bad_class, bad_next = good[0].copy(), good[1].copy()
        bad_class[V - 1] = good[1].shape[1]
        bad_next[0, 0] = good[1].shape[0]
        assert call(t=tables(tc=bad_class)) == _hip.EINVAL and call(t=tables(ns=bad_next)) == _hip.EINVAL
        assert call(n_states=0) == _hip.EINVAL and call(n_states=33) == _hip.EINVAL
        assert call(n_classes=0) == _hip.EINVAL and call(n_classes=17) == _hip.EINVAL
        assert call(end=-1) == _hip.EINVAL and call(end=V) == _hip.EINVAL
        assert call(horizon=0) == _hip.EINVAL and call(horizon=-3) == _hip.EINVAL
        two_steps = good[2].copy()
        two_steps[0] = 2
        assert call(horizon=1, t=tables(ml=two_steps)) == _hip.EINVAL and call(horizon=2, B=0, t=tables(ml=two_steps)) == 0  # min_left[0] > horizon
        assert call(B=-1) == _hip.EINVAL and call(T=-1) == _hip.EINVAL and call(Vv=-1) == _hip.EINVAL and call(Vv=0) == _hip.EINVAL
        wide = np.zeros(200, np.uint8)
        assert call(Vv=129, t=tables(tc=wide)) == _hip.ESHAPE and call(Vv=4000, t=tables(tc=wide)) == _hip.ESHAPE
        # an empty batch launches nothing, whatever else is given
        assert call(B=0) == 0 and call(T=0) == 0 and call(B=0, x=0, tokens=0, y=0, tc=0, horizon=0) == 0


def test_strategy_argument_rules(grammar):
    """Every check below comes before the first device call."""
    import torch

    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    _, auto, _ = grammar
    model = ProgramGenerator(Vocabulary.clevr(), max_decoding_steps=12)
    q = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises(ValueError):
        model(q, decoding_strategy="grammar_sampling")                       # no constraint
    with pytest.raises(ValueError):
        model.decode({}, decoding_strategy="grammar_sampling")
    with pytest.raises(ValueError):
        model.decode_grammar({}, None)
    for filt in (dict(temperature=0.5), dict(top_k=3), dict(top_p=0.9)):     # it takes no filter
        with pytest.raises(ValueError):
            model(q, decoding_strategy="grammar_sampling", constraint=auto, **filt)
        with pytest.raises(ValueError):
            model.decode({}, decoding_strategy="grammar_sampling", constraint=auto, **filt)
    state = {"enc": torch.zeros(2, 5, 256), "h": torch.zeros(2, 256), "fmask": torch.ones(2, 5)}
    other = SimpleNamespace(token_class=np.zeros(V + 1, np.uint8), next_state=np.zeros((1, 1), np.uint8), min_left=np.zeros(1, np.uint8))
    with pytest.raises(ValueError):
        model.decode_grammar(state, other)                                   # tables of another vocabulary
    short = ProgramGenerator(Vocabulary.clevr(), max_decoding_steps=1)
    two_steps = SimpleNamespace(token_class=np.zeros(V, np.uint8), next_state=np.array([[1], [1]], np.uint8),
                                min_left=np.array([2, 0], np.uint8))
    with pytest.raises(ValueError):
        short.decode_grammar(state, two_steps)                               # its shortest string takes two tokens
    long_state = dict(state, enc=torch.zeros(2, 65, 256))
    with pytest.raises(NotImplementedError):
        model.decode_grammar(long_state, auto)                               # outside the persistent kernels
    for strategy in ("sampling", "greedy"):                                  # (the old refusal stays)
        with pytest.raises(ValueError):
            model(q, decoding_strategy=strategy, constraint=auto)
    with pytest.raises(ValueError):
        model.decode({}, decoding_strategy="grammar")


def test_trainer_argument_rules(grammar):
    from probnmn.trainers.joint_training import JointTrainingStep, QuestionCodingStep, check_constraint
    from probnmn.trainers.marginal_training import MarginalJointStep, marginal_joint_options

    _, auto, _ = grammar

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the options are checked before any model is touched (%s)" % name)

    u = Untouchable()
    for bad in (object(), 3, "clevr", SimpleNamespace(token_class=np.zeros(V, np.uint8))):
        with pytest.raises(ValueError):
            QuestionCodingStep(u, u, u, constraint=bad)
        with pytest.raises(ValueError):
            JointTrainingStep(u, u, u, u, constraint=bad)
    assert check_constraint(None) is None and check_constraint(auto) is auto
    assert QuestionCodingStep.constraint is None and JointTrainingStep.constraint is None
    for options in (dict(grammar_normalised=True), dict(grammar_normalised=True, constrained=False),
                    dict(grammar_normalised=1, constrained=True), dict(grammar_normalised=None, constrained=True)):
        with pytest.raises(ValueError):
            MarginalJointStep(u, u, **options)
    with pytest.raises(ValueError):
        marginal_joint_options(4, False, False, 1.0, True, True)
    assert marginal_joint_options(4, True, False, 1.0, True, True) == 1.0
    assert marginal_joint_options(4, True, False, 0.5, True) == 0.5 and marginal_joint_options(4, False, False, 1.0, True, False) == 1.0
