"""The host reference of stochastic beam search (tests/stochastic_beam_ref.py) on its own, the importance weights of
``evaluators.without_replacement_weights`` against a direct fp64 evaluation, and the argument rules of the surface above
them -- no device, no model is ever called.

Exactness is checked on a tree small enough to enumerate: 4 tokens of which one is @end@, T = 3, hence 40 leaves, with
random conditional logits.  Over 200 000 seeds at K = 2 no question may hold a sequence twice, the first-ranked leaf is
distributed as p(leaf), and leaf i is included with probability p_i + sum_{j != i} p_j p_i / (1 - p_j): chi-square over
the leaves with an expected count >= 50 at the 1 - 1e-6 quantile, at a fixed seed."""
import itertools

import numpy as np
import pytest
import torch

import stochastic_beam_ref as ref

V, T, END = 4, 3, 3
NEG = -np.inf


@pytest.fixture(scope="module")
def tree():
    """Random conditional logits for every prefix of the tree, as arrays [4 ** t, V] per depth; the 40 leaves as token
    rows padded with @end@, their probabilities, and a vectorised ``prefixes -> logits``."""
    rng = np.random.default_rng(5)
    depth = [rng.normal(0.0, 1.5, size=(V ** t, V)) for t in range(T)]

    def code(prefix):
        c = 0
        for tok in prefix:
            c = c * V + int(tok)
        return c

    def logits(prefixes):
        t = prefixes.shape[-1]
        c = np.zeros(prefixes.shape[:-1], dtype=np.int64)
        for i in range(t):
            c = c * V + prefixes[..., i]
        return depth[t][c]

    leaves, probs = [], []
    for seq in itertools.product(range(V), repeat=T):
        if any(seq[i] == END and seq[i + 1] != END for i in range(T - 1)):
            continue  # after @end@ only @end@
        logp = 0.0
        for t in range(T):
            if t > 0 and seq[t - 1] == END:
                break
            row = depth[t][code(seq[:t])]
            logp += row[seq[t]] - np.log(np.exp(row).sum())
        leaves.append(seq)
        probs.append(np.exp(logp))
    probs = np.array(probs)
    assert len(leaves) == 40 and abs(probs.sum() - 1.0) < 1e-12
    index = {code(s): i for i, s in enumerate(leaves)}
    lookup = np.full(V ** T, -1, dtype=np.int64)
    for c, i in index.items():
        lookup[c] = i

    def leaf_of(tokens):  # [..., T] -> leaf index
        c = np.zeros(tokens.shape[:-1], dtype=np.int64)
        for i in range(T):
            c = c * V + tokens[..., i]
        return lookup[c]

    return {"logits": logits, "leaves": np.array(leaves), "p": probs, "leaf_of": leaf_of, "depth": depth}


@pytest.fixture(scope="module")
def run_k2(tree):
    """200 000 seeds at K = 2 on the tree, shared by the tests below and left unchanged."""
    n = 200_000
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)
    return ref.search(tree["logits"], 2, T, V, seeds, np.zeros(n, dtype=np.int64), END)


def test_the_uniform_is_an_odd_multiple_of_2_to_the_minus_24():
    for x0 in (0, 511, 512, 2 ** 32 - 1):
        u = float(ref.uniform_from_word(x0))
        m = u * 2 ** 24
        assert m == int(m) and int(m) % 2 == 1 and 0.0 < u < 1.0, (x0, u)
        assert float(np.float32(u)) == u and np.float32(u) < np.float32(1.0) and np.float32(u) > np.float32(0.0)
        assert np.isfinite(np.log(-np.log(u)))
    assert float(ref.uniform_from_word(0)) == 2.0 ** -24 and float(ref.uniform_from_word(2 ** 32 - 1)) == 1.0 - 2.0 ** -24
    assert float(ref.uniform_from_word(511)) == float(ref.uniform_from_word(0))  # the low nine bits do not count
    # the words are those of the sampling decoders' stream
    from token_choice import kernel_uniform
    seed, row, step = 77, np.arange(5), 3
    assert np.array_equal(ref.philox_words(seed, row, step) >> np.uint32(8),
                          (kernel_uniform(seed, row, step) * 2 ** 24).astype(np.uint32))


def test_a_beam_of_one_follows_the_gumbel_argmax(tree):
    out = ref.search(tree["logits"], 1, T, V, np.arange(500, dtype=np.uint64), np.arange(500) % 7, END)
    assert np.array_equal(out["G"], np.zeros((500, 1))) and np.array_equal(out["trace_perturbed"], np.zeros((500, T, 1)))
    tok, am = out["trace_tokens"][:, :, 0], out["trace_gumbel_argmax"][:, :, 0]
    live = am >= 0
    assert np.array_equal(tok[live], am[live]) and bool((tok[~live] == END).all())
    assert np.array_equal(out["tokens"][:, 0], tok)
    # phi is the log-probability of the leaf that came out
    assert np.allclose(out["phi"][:, 0], np.log(tree["p"][tree["leaf_of"](out["tokens"][:, 0])]), atol=1e-12)


def test_no_sequence_twice_and_phi_is_the_leaf_probability(tree, run_k2):
    leaf = tree["leaf_of"](run_k2["tokens"])
    assert bool((leaf >= 0).all()) and bool(np.isfinite(run_k2["phi"]).all())
    assert not bool((leaf[:, 0] == leaf[:, 1]).any()), "a question holds the same sequence twice"
    assert np.allclose(run_k2["phi"], np.log(tree["p"][leaf]), atol=1e-12)
    assert bool((run_k2["G"][:, 0] == 0.0).all()) and bool((run_k2["G"][:, 1] < 0.0).all())  # best first; the first keeps G = 0


def _chi_square(counts, expected, variance_scale=None):
    """Pearson statistic over the cells with an expected count >= 50 and the bar for its degrees of freedom."""
    big = expected >= 50
    assert int(big.sum()) >= 15
    var = expected if variance_scale is None else expected * variance_scale
    z = (counts[big] - expected[big]) / np.sqrt(var[big])
    return float((z ** 2).sum()), ref.chi_square_quantile(int(big.sum())), float(np.abs(z).max())


def test_the_first_ranked_leaf_is_distributed_as_p(tree, run_k2):
    n = run_k2["tokens"].shape[0]
    counts = np.bincount(tree["leaf_of"](run_k2["tokens"][:, 0]), minlength=40).astype(np.float64)
    stat, bar, worst = _chi_square(counts, n * tree["p"])
    print("first-ranked leaf: chi-square %.1f (bar %.1f), largest |z| %.2f" % (stat, bar, worst))
    assert stat < bar


def test_inclusion_probabilities_at_k2(tree, run_k2):
    n = run_k2["tokens"].shape[0]
    p = tree["p"]
    pi = p + np.array([sum(p[j] * p[i] / (1.0 - p[j]) for j in range(40) if j != i) for i in range(40)])
    assert abs(pi.sum() - 2.0) < 1e-9
    counts = np.bincount(tree["leaf_of"](run_k2["tokens"]).reshape(-1), minlength=40).astype(np.float64)
    stat, bar, worst = _chi_square(counts, n * pi, variance_scale=1.0 - pi)  # a leaf is in a question's sample or not
    print("inclusion: chi-square %.1f (bar %.1f), largest |z| %.2f" % (stat, bar, worst))
    assert stat < bar


def test_a_mask_that_leaves_fewer_than_k_sequences(tree):
    """Only @end@ or token 0 first, then only @end@: two sequences exist; K = 4 holds them and two empty slots."""
    def allowed(prefixes, t):
        ok = np.zeros(prefixes.shape[:-1] + (V,), dtype=bool)
        ok[..., END] = True
        if t == 0:
            ok[..., 0] = True
        return ok

    out = ref.search(tree["logits"], 4, T, V, np.arange(50, dtype=np.uint64), np.arange(50), END, allowed=allowed)
    assert bool(np.isfinite(out["phi"][:, :2]).all()) and bool(np.isfinite(out["G"][:, :2]).all())
    assert bool((out["phi"][:, 2:] == NEG).all()) and bool((out["G"][:, 2:] == NEG).all())
    assert bool((out["trace_tokens"][:, :, 2:] == END).all()) and bool((out["trace_backpointers"][:, :, 2:] == 0).all())
    assert bool((out["G"][:, -1] == NEG).all())  # kappa = -inf
    assert np.allclose(np.exp(out["phi"][:, :2]).sum(1), 1.0)  # the whole (renormalised) support
    first = {tuple(r) for r in out["tokens"][:, :2].reshape(-1, T).tolist()}
    assert first == {(END, END, END), (0, END, END)}
    lw = ref.without_replacement_log_weights(out["phi"], out["G"])
    assert np.array_equal(lw, out["phi"])
    from probnmn.evaluators import without_replacement_weights
    got = without_replacement_weights(torch.from_numpy(out["phi"]), torch.from_numpy(out["G"])).numpy()
    assert np.array_equal(got, out["phi"])


def test_a_table_of_logits_is_taken_like_a_callable(tree):
    table = {}
    for t in range(T):
        for prefix in itertools.product(range(V), repeat=t):
            c = 0
            for tok in prefix:
                c = c * V + tok
            table[prefix] = tree["depth"][t][c]
    seeds, q = np.arange(20, dtype=np.uint64) + np.uint64(9), np.arange(20) + 3
    a = ref.search(tree["logits"], 2, T, V, seeds, q, END)
    b = ref.search(table, 2, T, V, seeds, q, END)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_without_replacement_weights_against_fp64():
    from probnmn.evaluators import without_replacement_weights

    phi = np.array([[-0.5, -1.5, -3.0, -4.0],
                    [-0.1, -2.5, NEG, NEG],        # the whole support: kappa = -inf
                    [-40.0, -45.0, -50.0, -80.0],
                    [-1.0, -2.0, -3.0, -4.0],      # phi - kappa = +40 and below
                    [-60.0, -61.0, -62.0, -63.0],  # phi - kappa = -40 and below
                    [-0.7, NEG, -2.0, -2.5]])
    G = np.array([[0.0, -0.3, -1.1, -2.0],
                  [0.0, -1.0, NEG, NEG],
                  [0.0, -2.0, -3.0, -41.0],
                  [0.0, -10.0, -20.0, -41.0],
                  [0.0, -5.0, -10.0, -20.0],
                  [0.0, NEG, -1.0, -3.0]])
    want = ref.without_replacement_log_weights(phi, G)  # direct numerical integration
    # the weight lies between the paper's for the conditioned threshold with and without the root's share:
    # p / (1 - exp(-p e^-kappa)) <= w <= p / (1 - exp(-p (e^-kappa - 1)))
    lower = phi[0, :3] - np.log(-np.expm1(-np.exp(phi[0, :3] - G[0, 3])))
    upper = phi[0, :3] - np.log(-np.expm1(-np.exp(phi[0, :3]) * np.expm1(-G[0, 3])))
    assert bool((lower < want[0, :3]).all()) and bool((want[0, :3] < upper).all()) and want[0, 3] == NEG
    assert np.array_equal(want[1], [phi[1, 0], phi[1, 1], NEG, NEG])
    assert abs(want[3, 0] - phi[3, 0]) < 1e-9 and abs(want[4, 0] - G[4, 3]) < 1e-8  # q = 1; and w = p / q with q ~ e^(phi - kappa)
    assert want[5, 1] == NEG
    for dtype, tol in ((torch.float64, 1e-10), (torch.float32, 2e-5)):
        got = without_replacement_weights(torch.from_numpy(phi).to(dtype), torch.from_numpy(G).to(dtype))
        assert got.dtype == dtype and got.shape == (6, 4)
        got = got.double().numpy()
        assert not np.isnan(got).any() and not (got == np.inf).any()
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], atol=tol, rtol=tol), (dtype, np.abs(got[fin] - want[fin]).max())
    with pytest.raises(ValueError):
        without_replacement_weights(torch.zeros(3, 4), torch.zeros(3, 5))


def test_importance_weights_estimate_expectations(tree):
    """The mean over seeds of sum_i w_i f(i) approaches E_p[f] for an indicator f, within 5 standard errors of the run.

    The weights have to allow for the search's start: G = 0 at the root conditions every G on the largest being 0, and the
    paper's p_i / q_i(kappa) taken at the returned kappa comes out low (sum_i w_i averages 0.982 here, 0.745 at K = 2; this
    indicator 6.5 standard errors low).  ``without_replacement_weights`` averages the paper's weight over the root's free value
    instead; measured here: within 1 standard error, sum_i w_i = 1.0006."""
    from probnmn.evaluators import without_replacement_weights

    n = 40_000
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(7)
    out = ref.search(tree["logits"], 4, T, V, seeds, np.zeros(n, dtype=np.int64), END)
    w = np.exp(without_replacement_weights(torch.from_numpy(out["phi"]), torch.from_numpy(out["G"])).numpy())
    assert bool((w[:, -1] == 0.0).all())
    leaf = tree["leaf_of"](out["tokens"])
    for first_token in (0, 1, END):
        f = (tree["leaves"][:, 0] == first_token).astype(np.float64)
        truth = float((tree["p"] * f).sum())
        est = (w * f[leaf]).sum(1)
        err, se = abs(est.mean() - truth), est.std(ddof=1) / np.sqrt(n)
        print("E[first token == %d] = %.4f: estimate %.4f, %.2f standard errors" % (first_token, truth, est.mean(), err / se))
        assert err < 5.0 * se


def test_argument_rules():
    from probnmn.evaluators import evaluate_marginal_answer_accuracy, predict_answers
    from probnmn.models import ProgramGenerator
    from probnmn.modules.seq2seq_base import Seq2SeqBase
    from probnmn.vocabulary import Vocabulary

    model = ProgramGenerator(Vocabulary.clevr())  # on the host: every call below is refused before it looks at its state
    for fn in (lambda **kw: predict_answers(None, None, [], None, **kw),
               lambda **kw: evaluate_marginal_answer_accuracy(None, None, [], **kw)):
        for bad in (3, 1, 32, 6, None, True, 4.0):
            with pytest.raises(ValueError, match=r"\(2, 4, 8, 16\)"):
                fn(num_programs=bad, without_replacement=True)
        with pytest.raises(ValueError, match="beam_size"):
            fn(beam_size=4, without_replacement=True)
        with pytest.raises(ValueError, match="without_replacement"):
            fn(num_programs=4, sample_weights="importance")
        with pytest.raises(ValueError, match="sample_weights"):
            fn(num_programs=4, without_replacement=True, sample_weights="uniform")
    with pytest.raises(ValueError, match="beam_size"):
        predict_answers(None, None, [], None, beam_size=4, marginal=True, without_replacement=True)
    with pytest.raises(ValueError, match="filter"):
        predict_answers(None, None, [], None, num_programs=4, without_replacement=True, top_k=3)
    # the strategy: accepted where "beam" is, with its argument rules, and named where the strategies are listed
    with pytest.raises(ValueError, match="stochastic_beam"):
        Seq2SeqBase._check_beam_arguments(torch.zeros(1, 2, dtype=torch.long), 4, "stochastic_beam")
    for bad in (3, 0, 32, 2.0, None, True):
        with pytest.raises(ValueError, match="beam_size"):
            model.decode({}, decoding_strategy="stochastic_beam", beam_size=bad)
        with pytest.raises(ValueError, match="beam_size"):
            model.decode_stochastic_beam({}, beam_size=bad)
    with pytest.raises(ValueError, match="target_tokens"):
        model.decode({}, torch.zeros(1, 2, dtype=torch.long), decoding_strategy="stochastic_beam")
    with pytest.raises(ValueError, match="does not sample"):
        model.decode({}, decoding_strategy="stochastic_beam", temperature=0.5)
    with pytest.raises(ValueError, match="'stochastic_beam'"):
        model.decode({}, decoding_strategy="beams")
    with pytest.raises(ValueError, match="'stochastic_beam'"):
        model.decode({}, decoding_strategy="greedy", constraint=object())
