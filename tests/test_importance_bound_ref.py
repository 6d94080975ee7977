"""The importance-weighted bound and its VIMCO estimator without a device: the host statement of ``pnmn_importance_bound``
(tests/helpers/importance_bound_reference.py) is unbiased by exhaustive enumeration and keeps the identities of the bound;
the extension header reads, the library exports the entry point and checks its arguments in the stated order before any HIP
call; the option rules of ``importance_weighted_bound``, ``ImportanceWeightedCodingStep`` and ``evaluate_question_evidence``
are ``ValueError``s that touch no device."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from importance_bound_reference import importance_bound_reference, question_statistics  # noqa: E402


# ---- the estimator ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("beta", [1.0, 0.1])
@pytest.mark.parametrize("samples", [1, 2, 3, 4])
def test_estimator_is_unbiased_by_enumeration(samples, beta):
    """Over all 3^K tuples of a three-outcome q: sum q(tuple) sum_k (signal_k - beta share_k) grad log q(z_k) is the gradient
    torch autograd gives of the enumerated E[bound] in fp64 -- where both q(tuple) and log w depend on q's logits."""
    rng = np.random.default_rng(7 + samples)
    theta0 = rng.normal(size=3)
    lx, lp = rng.normal(size=3) * 2.0 - 3.0, np.log(rng.dirichlet(np.ones(3)))
    theta = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    log_q = torch.log_softmax(theta, 0)
    log_w = torch.tensor(lx) + beta * (torch.tensor(lp) - log_q)
    tuples = list(itertools.product(range(3), repeat=samples))
    expected_bound = 0.0
    for z in tuples:
        z = list(z)
        expected_bound = expected_bound + log_q[z].sum().exp() * (torch.logsumexp(log_w[z], 0) - np.log(samples))
    (exact,) = torch.autograd.grad(expected_bound, theta)
    q = log_q.exp().detach().numpy()
    score = np.eye(3) - q[None, :]  # d log q(z) / d theta, row z
    w = log_w.detach().numpy()
    estimate = np.zeros(3)
    for z in tuples:
        z = list(z)
        bound, share, _, signal = question_statistics(w[z])
        assert bound >= w[z].mean() - 1e-12                       # the bound is at least the mean log-weight (the ELBO)
        estimate += np.prod(q[z]) * ((signal - beta * share)[:, None] * score[z]).sum(0)
    assert np.abs(estimate - exact.numpy()).max() <= 1e-10


def _random_terms(G, K, seed, Tx=4, Tp=3, Tq=3, Vx=7, Vq=5):
    rng = np.random.default_rng(seed)
    R = G * K

    def term(T, V):
        logits = rng.standard_normal((R, T, V)) * 2
        tokens = rng.integers(1, V, (R, T)).astype(np.int64)
        tokens[rng.random((R, T)) < 0.25] = 0
        return logits, tokens, 0

    return term(Tx, Vx), term(Tq, Vq), term(Tp, Vq)


@pytest.mark.parametrize("samples", [1, 2, 5, 64])
def test_identities_of_the_reference(samples):
    x, q, p = _random_terms(6, samples, samples)
    for beta, prior in ((1.0, p), (0.1, p), (1.0, None), (0.0, p)):
        ref = importance_bound_reference(x, q, prior, beta, samples, gradients=True)
        assert (ref["support"] == samples).all()
        lw = ref["log_weight"].reshape(6, samples)
        assert (ref["bound"] >= lw.mean(1) - 1e-12).all()
        np.testing.assert_allclose(ref["share"].reshape(6, samples).sum(1), 1.0, rtol=0, atol=1e-12)
        assert (ref["ess"] >= 1 - 1e-12).all() and (ref["ess"] <= samples + 1e-12).all()
        if samples == 1:
            assert np.array_equal(ref["signal"], ref["bound"]) and np.array_equal(ref["bound"], ref["log_weight"])
        # log w is the stated combination of the terms that enter
        want = ref["log_px"].copy()
        if beta != 0.0:
            want -= beta * ref["log_q"]
            if prior is not None:
                want += beta * ref["log_pz"]
        np.testing.assert_allclose(ref["log_weight"], want, rtol=0, atol=1e-12)
        assert (ref["log_pz"] is None) == (prior is None or beta == 0.0)
        # the x gradient is the derivative of -bound: a finite difference of one logit
        r, t = 1, int(np.argmax(x[1][1] != 0))
        bumped = x[0].copy()
        bumped[r, t, 2] += 1e-6
        moved = importance_bound_reference((bumped, x[1], x[2]), q, prior, beta, samples)
        g = r // samples
        assert abs(-(moved["bound"][g] - ref["bound"][g]) / 1e-6 - ref["d_x"][r, t, 2]) <= 1e-5
        # every gradient row sums to zero over the vocabulary and is zero on the padding steps
        for name, term in (("d_x", x), ("d_q", q)):
            assert np.abs(ref[name].sum(2)).max() <= 1e-12 and (ref[name][term[1] == 0] == 0).all()


@pytest.mark.parametrize("samples", [1, 2, 3, 8])
def test_the_exact_posterior_makes_every_weight_the_evidence(samples):
    """A three-valued latent: q(z | x) = p(x | z) p(z) / p(x) makes log w = log p(x) for every sample, so the bound is
    log p(x) for every K, no sample carries a learning signal and every sample counts in full."""
    rng = np.random.default_rng(3)
    prior = rng.dirichlet(np.ones(3))
    likelihood = rng.dirichlet(np.ones(2), 3)          # p(x | z), x in {0, 1}
    G = 4
    observed = rng.integers(0, 2, G)
    z = rng.integers(0, 3, (G, samples))
    R = G * samples
    x_logits, p_logits, q_logits = np.zeros((R, 1, 2)), np.zeros((R, 1, 3)), np.zeros((R, 1, 3))
    x_tokens, z_tokens = np.zeros((R, 1), np.int64), np.zeros((R, 1), np.int64)
    evidence = np.zeros(G)
    for g in range(G):
        joint = likelihood[:, observed[g]] * prior
        evidence[g] = np.log(joint.sum())
        for k in range(samples):
            r = g * samples + k
            x_logits[r, 0], x_tokens[r, 0] = np.log(likelihood[z[g, k]]), observed[g]
            p_logits[r, 0], z_tokens[r, 0] = np.log(prior), z[g, k]
            q_logits[r, 0] = np.log(joint / joint.sum())
    ref = importance_bound_reference((x_logits, x_tokens, -1), (q_logits, z_tokens, -1), (p_logits, z_tokens, -1), 1.0, samples)
    np.testing.assert_allclose(ref["log_weight"], np.repeat(evidence, samples), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["bound"], evidence, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["ess"], samples, rtol=0, atol=1e-9)
    if samples >= 2:
        assert np.abs(ref["signal"]).max() <= 1e-12


def test_a_token_that_is_no_index_rules_out_its_question_alone():
    K = 3
    x, q, p = _random_terms(5, K, 11)
    base = importance_bound_reference(x, q, p, 1.0, K, gradients=True)
    for which, bad_token in ((0, 99), (1, -4), (2, 99)):
        terms = [(t[0], t[1].copy(), t[2]) for t in (x, q, p)]
        terms[which][1][2 * K + 1, 0] = bad_token      # question 2, its second sample
        ref = importance_bound_reference(terms[0], terms[1], terms[2], 1.0, K, gradients=True)
        assert ref["support"].tolist() == [K, K, K - 1, K, K] and np.isneginf(ref["bound"][2])
        rows = slice(2 * K, 3 * K)
        assert (ref["share"][rows] == 0).all() and (ref["signal"][rows] == 0).all() and ref["ess"][2] == 0
        assert np.isneginf(ref["log_weight"][2 * K + 1]) and np.isfinite(np.delete(ref["log_weight"], 2 * K + 1)).all()
        for name in ("d_x", "d_q", "d_p"):
            assert (ref[name][rows] == 0).all()
        others = np.r_[0:2 * K, 3 * K:5 * K]
        for name in ("share", "signal", "log_weight", "d_x", "d_q", "d_p"):
            assert np.array_equal(ref[name][others], base[name][others]), name
    # with beta == 0 the generator's term leaves log w: a generator token that is no index rules nothing out
    terms_q = (q[0], q[1].copy(), q[2])
    terms_q[1][2 * K + 1, 0] = 99
    ref = importance_bound_reference(x, terms_q, p, 0.0, K)
    assert (ref["support"] == K).all() and np.isneginf(ref["log_q"][2 * K + 1]) and ref["log_pz"] is None


# ---- the header and the library -------------------------------------------------------------------------------------------

def test_extension_header_reads_and_leaves_the_other_bindings_alone():
    import ctypes

    from probnmn import _hip, _hip_grammar, _hip_importance

    assert len(_hip.SIGNATURES) == 103
    sigs, restypes, records, constants = _hip.read_header(_hip_importance.HEADER_PATH)
    assert os.path.basename(_hip_importance.HEADER_PATH) == "probnmn_importance.h"
    assert set(sigs) == {"pnmn_importance_bound"} and not records and not constants
    assert "pnmn_importance_bound" not in _hip.SIGNATURES and "pnmn_importance_bound" not in _hip_grammar.SIGNATURES
    sig = sigs["pnmn_importance_bound"]
    assert len(sig) == 34 and restypes["pnmn_importance_bound"] is ctypes.c_int
    term = (ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int)
    assert sig[:18] == term * 3 and sig[18:21] == (ctypes.c_float, ctypes.c_int, ctypes.c_int)
    assert sig[21:] == (ctypes.c_void_p,) * 13
    lib = _hip_importance.lib()
    assert lib is _hip.lib() and lib is _hip_grammar.lib()
    assert lib.pnmn_importance_bound.argtypes == list(sig)
    assert set(_hip_grammar.SIGNATURES) == {"pnmn_grammar_logits", "pnmn_grammar_logits_bwd"}
    assert lib.pnmn_grammar_logits.argtypes == list(_hip_grammar.SIGNATURES["pnmn_grammar_logits"])


def test_entry_point_checks_its_arguments_in_order_without_a_device():
    from probnmn import _hip, _hip_importance

    lib = _hip_importance.lib()
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)

    def call(n=2, samples=3, beta=1.0, x=(p, p), prior=(p, p), q=(p, p), Tx=2, Vx=4, Tp=2, Vp=4, Tq=2, Vq=4,
             required=(p, p, p, p), d=(0, 0, 0)):
        log_weight, share, signal, bound = required
        return lib.pnmn_importance_bound(x[0], x[1], Tx, 0, Tx, Vx, prior[0], prior[1], Tp, 0, Tp, Vp, q[0], q[1], Tq, 0, Tq, Vq,
                                         beta, n, samples, 0, 0, 0, log_weight, share, signal, bound, 0, 0, d[0], d[1], d[2], 0)

    # 1. the counts, before anything else
    assert call(n=-1) == _hip.EINVAL
    for samples in (0, -1, 65, 1 << 20):
        assert call(samples=samples) == _hip.EINVAL and call(samples=samples, n=0) == _hip.EINVAL
    # 2. no question: 0, whatever else is given
    assert call(n=0) == 0
    assert call(n=0, x=(0, 0), q=(0, 0), required=(0, 0, 0, 0), beta=-1.0, Tx=0, Vx=5000, d=(0, p, 0), prior=(0, 0)) == 0
    # 3. pointers, shapes of the given terms, beta
    assert call(x=(0, p)) == _hip.EINVAL and call(x=(p, 0)) == _hip.EINVAL
    assert call(q=(0, p)) == _hip.EINVAL and call(q=(p, 0)) == _hip.EINVAL
    for missing in range(4):
        assert call(required=tuple(0 if i == missing else p for i in range(4))) == _hip.EINVAL, missing
    assert call(prior=(p, 0)) == _hip.EINVAL                    # logits without their tokens
    assert call(prior=(0, 0), d=(0, p, 0)) == _hip.EINVAL       # a gradient without its logits
    assert call(x=(0, p), d=(p, 0, 0)) == _hip.EINVAL and call(q=(0, p), d=(0, 0, p)) == _hip.EINVAL
    for shape in (dict(Tx=0), dict(Vx=0), dict(Tq=0), dict(Vq=-1), dict(Tp=0), dict(Vp=0)):
        assert call(**shape) == _hip.EINVAL, shape
    for beta in (-0.5, float("inf"), float("-inf"), float("nan")):
        assert call(beta=beta) == _hip.EINVAL, beta
    # ... all of them before the shape: an argument error with a vocabulary that is too wide is still an argument error
    assert call(Vx=1025, beta=-1.0) == _hip.EINVAL and call(Vq=4000, required=(p, p, p, 0)) == _hip.EINVAL
    # 4. the shape
    for shape in (dict(Vx=1025), dict(Vq=1025), dict(Vp=1025), dict(Vx=1 << 20)):
        assert call(**shape) == _hip.ESHAPE, shape
    assert call(n=1 << 30, samples=64) == _hip.ESHAPE           # more rows than an int32 counts


# ---- the option rules -----------------------------------------------------------------------------------------------------

class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the options are checked before any model is touched (%s)" % name)


def test_option_rules_of_the_loss():
    from probnmn import _hip
    from probnmn.modules.importance_weighted import importance_weighted_bound

    def term(R=6, T=2, V=4, dtype=torch.float32):
        return torch.zeros(R, T, V, dtype=dtype), torch.zeros(R, T, dtype=torch.long), 0

    x, q, p = term(), term(T=3), term()
    for samples in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            importance_weighted_bound(x, q, p, samples=samples)
    for beta in (-1.0, float("nan"), float("inf"), "much", None, True):
        with pytest.raises(ValueError):
            importance_weighted_bound(x, q, p, samples=2, beta=beta)
    with pytest.raises(ValueError):
        importance_weighted_bound(x, q, p, samples=4)                                   # 6 rows are not questions of 4
    with pytest.raises(ValueError):
        importance_weighted_bound(x, term(R=8), p, samples=2)                           # the terms disagree on the rows
    with pytest.raises(ValueError):
        importance_weighted_bound(term(dtype=torch.float64), q, p, samples=2)
    with pytest.raises(ValueError):
        importance_weighted_bound((x[0], x[1][:, :1], 0), q, p, samples=2)              # tokens that do not fit the logits
    with pytest.raises(ValueError):
        importance_weighted_bound((torch.zeros(6, 0, 4), torch.zeros(6, 0, dtype=torch.long), 0), q, p, samples=2)
    with pytest.raises(ValueError):
        importance_weighted_bound(None, q, p, samples=2)
    with pytest.raises(ValueError):
        importance_weighted_bound(x, None, p, samples=2)
    with pytest.raises(_hip.HipLibraryError):
        importance_weighted_bound(x, q, p, samples=2)                                   # well formed, on the host: no CPU path
    with pytest.raises(_hip.HipLibraryError):
        importance_weighted_bound(x, q, None, samples=3, beta=0.0)


def test_option_rules_of_the_trainer_and_the_evaluator():
    from types import SimpleNamespace

    from probnmn import trainers
    from probnmn.evaluators import evaluate_question_evidence
    from probnmn.models import ProgramGenerator
    from probnmn.trainers.importance_weighted import ImportanceWeightedCodingStep, importance_weighted_options
    from probnmn.vocabulary import Vocabulary

    assert trainers.ImportanceWeightedCodingStep is ImportanceWeightedCodingStep
    u = _Untouchable()
    half = SimpleNamespace(token_class=np.zeros(4, np.uint8))
    for options in (dict(num_samples=1), dict(num_samples=0), dict(num_samples=65), dict(num_samples=4.0), dict(num_samples=True),
                    dict(beta=-0.1), dict(beta=float("nan")), dict(beta=float("inf")), dict(beta="0.1x"),
                    dict(constraint=3), dict(constraint=half)):
        with pytest.raises(ValueError):
            ImportanceWeightedCodingStep(u, u, u, **options)
    assert importance_weighted_options(2, 0, None) == (2, 0.0, None) and importance_weighted_options(64, 0.1, None)[0] == 64
    # samples and scores must come from one q: encoder dropout in the generator is refused, before the other models are touched
    with pytest.raises(ValueError, match="dropout"):
        ImportanceWeightedCodingStep(ProgramGenerator(Vocabulary.clevr(), dropout=0.2), u, u)
    for options in (dict(num_samples=0), dict(num_samples=65), dict(num_samples=2.5), dict(num_samples=False),
                    dict(constraint="clevr"), dict(constraint=half)):
        with pytest.raises(ValueError):
            evaluate_question_evidence(u, u, u, u, **options)
