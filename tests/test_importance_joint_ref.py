"""The joint importance-weighted bound -- the answer likelihood inside the weight -- and its VIMCO estimator without a device:
the host statement of ``pnmn_importance_bound_joint`` (tests/helpers/importance_joint_reference.py) is unbiased by exhaustive
enumeration, its answer gradient is the derivative of -bound, and it keeps the identities of the bound; the extension header
reads, the library exports the entry point and checks its arguments in the stated order before any HIP call; the option
rules of ``joint_importance_weighted_bound``, ``ImportanceWeightedJointStep`` and ``evaluate_joint_evidence`` are
``ValueError``s that touch no device."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from importance_bound_reference import importance_bound_reference  # noqa: E402
from importance_joint_reference import importance_joint_reference  # noqa: E402


# ---- the estimator ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", [1.0, 0.5])
@pytest.mark.parametrize("beta", [1.0, 0.1])
@pytest.mark.parametrize("samples", [1, 2, 3, 4])
def test_estimator_is_unbiased_by_enumeration(samples, beta, gamma):
    """Over all 3^K tuples of a three-outcome q: sum q(tuple) sum_k (signal_k - beta share_k) grad log q(z_k) is the gradient
    torch autograd gives of the enumerated E[bound] in fp64, with gamma log p(a | z) inside log w."""
    rng = np.random.default_rng(70 + samples)
    theta0 = rng.normal(size=3)
    likelihood = rng.dirichlet(np.ones(2), 3) ** 2.0                      # p(x | z) of two questions, per outcome z (rows
    likelihood /= likelihood.sum(1, keepdims=True)                        # renormalised: the terms are log-softmaxes)
    answering = rng.dirichlet(np.ones(4), 3)                              # p(a | z) of four answers
    lx, la, lp = np.log(likelihood[:, 0]), np.log(answering[:, 1]), np.log(rng.dirichlet(np.ones(3)))
    theta = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    log_q = torch.log_softmax(theta, 0)
    log_w = torch.tensor(lx) + gamma * torch.tensor(la) + beta * (torch.tensor(lp) - log_q)
    tuples = list(itertools.product(range(3), repeat=samples))
    expected_bound = 0.0
    for z in tuples:
        z = list(z)
        expected_bound = expected_bound + log_q[z].sum().exp() * (torch.logsumexp(log_w[z], 0) - np.log(samples))
    (exact,) = torch.autograd.grad(expected_bound, theta)
    q = log_q.exp().detach().numpy()
    score = np.eye(3) - q[None, :]  # d log q(z) / d theta, row z
    estimate = np.zeros(3)
    zeros = np.zeros((samples, 1), np.int64)
    for z in tuples:
        z = list(z)
        # one question of K one-step rows through the reference: the observed question is token 0, the answer is 1
        tokens = np.array(z, np.int64)[:, None]
        ref = importance_joint_reference((np.log(likelihood)[z][:, None, :], zeros, -1),
                                         (np.tile(np.log(q), (samples, 1))[:, None, :], tokens, -1),
                                         (np.tile(lp, (samples, 1))[:, None, :], tokens, -1), beta, samples,
                                         (np.log(answering)[z], np.ones(1, np.int64), None), answer_weight=gamma)
        np.testing.assert_allclose(ref["log_weight"], log_w.detach().numpy()[z], rtol=0, atol=1e-12)
        assert ref["bound"][0] >= ref["log_weight"].mean() - 1e-12       # the bound is at least the mean log-weight
        estimate += np.prod(q[z]) * ((ref["signal"] - beta * ref["share"])[:, None] * score[z]).sum(0)
    assert np.abs(estimate - exact.numpy()).max() <= 1e-10


def _random_terms(G, K, seed, Tx=4, Tp=3, Tq=3, Vx=7, Vq=5, A=6):
    rng = np.random.default_rng(seed)
    R = G * K

    def term(T, V):
        logits = rng.standard_normal((R, T, V)) * 2
        tokens = rng.integers(1, V, (R, T)).astype(np.int64)
        tokens[rng.random((R, T)) < 0.25] = 0
        return logits, tokens, 0

    x, q, p = term(Tx, Vx), term(Tq, Vq), term(Tp, Vq)
    answer = (rng.standard_normal((R, A)) * 2, rng.integers(0, A, G).astype(np.int64), None)
    return x, q, p, answer


@pytest.mark.parametrize("samples", [1, 2, 5, 64])
def test_identities_of_the_reference(samples):
    G = 6
    x, q, p, answer = _random_terms(G, samples, samples)
    for beta, gamma, prior in ((1.0, 1.0, p), (0.1, 0.5, p), (1.0, 2.0, None), (0.0, 1.0, p)):
        ref = importance_joint_reference(x, q, prior, beta, samples, answer, answer_weight=gamma, gradients=True)
        assert (ref["support"] == samples).all()
        lw = ref["log_weight"].reshape(G, samples)
        assert (ref["bound"] >= lw.mean(1) - 1e-12).all()
        np.testing.assert_allclose(ref["share"].reshape(G, samples).sum(1), 1.0, rtol=0, atol=1e-12)
        assert (ref["ess"] >= 1 - 1e-12).all() and (ref["ess"] <= samples + 1e-12).all()
        if samples == 1:
            assert np.array_equal(ref["signal"], ref["bound"]) and np.array_equal(ref["bound"], ref["log_weight"])
        # log w is the question-only weight with gamma la added to it
        base = importance_bound_reference(x, q, prior, beta, samples)
        np.testing.assert_allclose(ref["log_weight"], base["log_weight"] + gamma * ref["log_pa"], rtol=0, atol=1e-12)
        want = np.array([answer[0][r, answer[1][r // samples]] - np.log(np.exp(answer[0][r]).sum()) for r in range(G * samples)])
        np.testing.assert_allclose(ref["log_pa"], want, rtol=0, atol=1e-12)
        assert np.array_equal(ref["row_predictions"], answer[0].argmax(1))
        # the answer gradient is the derivative of -bound: a finite difference of one answer logit
        for r, c in ((1, 2), (samples * 2, int(answer[1][2]))):
            bumped = answer[0].copy()
            bumped[r, c] += 1e-6
            moved = importance_joint_reference(x, q, prior, beta, samples, (bumped, answer[1], None), answer_weight=gamma)
            g = r // samples
            assert abs(-(moved["bound"][g] - ref["bound"][g]) / 1e-6 - ref["d_a"][r, c]) <= 1e-5
        assert np.abs(ref["d_a"].sum(1)).max() <= 1e-12                  # every gradient row sums to zero over the answers
        np.testing.assert_allclose(ref["coefficient_a"], gamma * ref["share"], rtol=0, atol=0)
    # gamma == 0 reproduces the question-only reference exactly, whatever the answer holds
    bad = (answer[0], np.full(G, 99, np.int64), np.zeros(G * samples, np.int32))
    for beta, prior in ((1.0, p), (0.1, None), (0.0, p)):
        ref = importance_joint_reference(x, q, prior, beta, samples, bad, answer_weight=0.0, invalid_log_answer=-np.inf, gradients=True)
        base = importance_bound_reference(x, q, prior, beta, samples, gradients=True)
        for name, value in base.items():
            assert (value is None and ref[name] is None) or np.array_equal(ref[name], value), name
        assert (ref["d_a"] == 0).all() and np.isneginf(ref["log_pa"]).all() and (ref["row_predictions"] == 0).all()


@pytest.mark.parametrize("samples", [1, 2, 3, 8])
def test_the_exact_posterior_makes_every_weight_the_joint_evidence(samples):
    """A three-valued latent: q(z | x) = p(x | z) p(z) p(a | z) / p(x, a) makes log w = log p(x, a) for every sample, so the
    bound is log p(x, a) for every K and no sample carries a learning signal."""
    rng = np.random.default_rng(3)
    prior = rng.dirichlet(np.ones(3))
    likelihood = rng.dirichlet(np.ones(2), 3)          # p(x | z), x in {0, 1}
    answering = rng.dirichlet(np.ones(4), 3)           # p(a | z), a in {0 .. 3}
    G = 4
    observed, answers = rng.integers(0, 2, G), rng.integers(0, 4, G).astype(np.int64)
    z = rng.integers(0, 3, (G, samples))
    R = G * samples
    x_logits, p_logits, q_logits, a_logits = np.zeros((R, 1, 2)), np.zeros((R, 1, 3)), np.zeros((R, 1, 3)), np.zeros((R, 4))
    x_tokens, z_tokens = np.zeros((R, 1), np.int64), np.zeros((R, 1), np.int64)
    evidence = np.zeros(G)
    for g in range(G):
        joint = likelihood[:, observed[g]] * prior * answering[:, answers[g]]
        evidence[g] = np.log(joint.sum())
        for k in range(samples):
            r = g * samples + k
            x_logits[r, 0], x_tokens[r, 0] = np.log(likelihood[z[g, k]]), observed[g]
            p_logits[r, 0], z_tokens[r, 0] = np.log(prior), z[g, k]
            q_logits[r, 0] = np.log(joint / joint.sum())
            a_logits[r] = np.log(answering[z[g, k]]) + 1.5          # (any shift: the term is a log-softmax)
    ref = importance_joint_reference((x_logits, x_tokens, -1), (q_logits, z_tokens, -1), (p_logits, z_tokens, -1), 1.0, samples,
                                     (a_logits, answers, None))
    np.testing.assert_allclose(ref["log_weight"], np.repeat(evidence, samples), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["bound"], evidence, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["ess"], samples, rtol=0, atol=1e-9)
    if samples >= 2:
        assert np.abs(ref["signal"]).max() <= 1e-12


def test_rows_and_answers_that_rule_out_their_question_alone():
    K, G, A = 3, 5, 6
    x, q, p, answer = _random_terms(G, K, 11, A=A)
    base = importance_joint_reference(x, q, p, 1.0, K, answer, gradients=True)
    marked, rows = 2 * K + 1, slice(2 * K, 3 * K)      # question 2, its second sample
    others = np.r_[0:2 * K, 3 * K:G * K]
    names = ("share", "signal", "log_weight", "log_pa", "row_predictions", "d_x", "d_q", "d_p", "d_a")
    valid = np.ones(G * K, np.int32)
    valid[marked] = 0

    # an invalid row with a finite log p(a | z) (the default, -log A): the question still counts, the row's d_a is zeros
    ref = importance_joint_reference(x, q, p, 1.0, K, (answer[0], answer[1], valid), gradients=True, unknown_index=4)
    assert (ref["support"] == K).all() and ref["log_pa"][marked] == -np.log(A) and ref["row_predictions"][marked] == 4
    assert (ref["d_a"][marked] == 0).all() and ref["coefficient_a"][marked] == 0 and ref["share"][marked] > 0
    assert np.abs(ref["d_a"][2 * K]).max() > 0 and np.isfinite(ref["bound"]).all()
    for name in names:
        assert np.array_equal(ref[name][others], base[name][others]), name

    def ruled_out(ref):
        assert ref["support"].tolist() == [K, K, K - 1, K, K] and np.isneginf(ref["bound"][2]) and ref["ess"][2] == 0
        assert (ref["share"][rows] == 0).all() and (ref["signal"][rows] == 0).all()
        for name in ("d_x", "d_q", "d_p", "d_a"):
            assert (ref[name][rows] == 0).all(), name
        for name in names:
            assert np.array_equal(ref[name][others], base[name][others]), name
        assert np.isfinite(ref["log_weight"][others]).all()

    # the same row with -inf
    ref = importance_joint_reference(x, q, p, 1.0, K, (answer[0], answer[1], valid), invalid_log_answer=-np.inf, gradients=True)
    ruled_out(ref)
    assert np.isneginf(ref["log_weight"][marked]) and np.isfinite(np.delete(ref["log_weight"], marked)).all()
    # a -inf logit at the answer, in one row
    logits = answer[0].copy()
    logits[marked, answer[1][2]] = -np.inf
    ref = importance_joint_reference(x, q, p, 1.0, K, (logits, answer[1], None), gradients=True)
    ruled_out(ref)
    assert np.isneginf(ref["log_pa"][marked]) and np.isfinite(np.delete(ref["log_pa"], marked)).all()
    # an answer that is no index: every row of its question, and it is never a padding value either
    for bad in (A, -1, -2, 1 << 40):
        answers = answer[1].copy()
        answers[2] = bad
        ref = importance_joint_reference(x, q, p, 1.0, K, (answer[0], answers, None), gradients=True)
        assert ref["support"].tolist() == [K, K, 0, K, K] and np.isneginf(ref["log_pa"][rows]).all()
        ref["support"][2] = K - 1
        ruled_out(ref)


# ---- the header and the library -------------------------------------------------------------------------------------------

def test_extension_header_reads_and_leaves_the_other_bindings_alone():
    import ctypes

    from probnmn import _hip, _hip_grammar, _hip_importance, _hip_importance_joint

    name = "pnmn_importance_bound_joint"
    sigs, restypes, records, constants = _hip.read_header(_hip_importance_joint.HEADER_PATH)
    assert os.path.basename(_hip_importance_joint.HEADER_PATH) == "probnmn_importance_joint.h"
    assert set(sigs) == {name} and not records and not constants
    # the core, grammar and importance bindings are what they were
    assert len(_hip.SIGNATURES) == 103 and name not in _hip.SIGNATURES
    assert set(_hip_importance.SIGNATURES) == {"pnmn_importance_bound"}
    assert set(_hip_grammar.SIGNATURES) == {"pnmn_grammar_logits", "pnmn_grammar_logits_bwd"}
    # everything pnmn_importance_bound takes, in its order, then the answer term, then the stream
    sig, theirs = sigs[name], _hip_importance.SIGNATURES["pnmn_importance_bound"]
    assert restypes[name] is ctypes.c_int and sig[:33] == theirs[:33] and len(theirs) == 34
    p = ctypes.c_void_p
    assert sig[33:] == (p, p, p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, p, p, p, p)
    lib = _hip_importance_joint.lib()
    assert lib is _hip.lib() and lib is _hip_importance.lib() and lib is _hip_grammar.lib()
    assert lib.pnmn_importance_bound_joint.argtypes == list(sig)           # the shared handle exports the symbol
    assert lib.pnmn_importance_bound.argtypes == list(theirs)


def test_entry_point_checks_its_arguments_in_order_without_a_device():
    from probnmn import _hip, _hip_importance_joint

    lib = _hip_importance_joint.lib()
    p = np.zeros(64, np.float32).ctypes.data  # (never read: every call below returns before a launch)
    inf, nan = float("inf"), float("nan")

    def call(n=2, samples=3, beta=1.0, x=(p, p), prior=(p, p), q=(p, p), Tx=2, Vx=4, Tp=2, Vp=4, Tq=2, Vq=4,
             required=(p, p, p, p), d=(0, 0, 0, 0), a_logits=p, answers=p, valid=0, A=4, gamma=1.0, invalid=-1.0):
        log_weight, share, signal, bound = required
        return lib.pnmn_importance_bound_joint(
            x[0], x[1], Tx, 0, Tx, Vx, prior[0], prior[1], Tp, 0, Tp, Vp, q[0], q[1], Tq, 0, Tq, Vq, beta, n, samples, 0, 0, 0,
            log_weight, share, signal, bound, 0, 0, d[0], d[1], d[2], a_logits, valid, answers, A, gamma, invalid, 0, 0, 0, d[3], 0)

    # 1. the counts, before anything else
    assert call(n=-1) == _hip.EINVAL
    for samples in (0, -1, 65, 1 << 20):
        assert call(samples=samples) == _hip.EINVAL and call(samples=samples, n=0) == _hip.EINVAL
    # 2. no question: 0, whatever else is given
    assert call(n=0) == 0
    assert call(n=0, x=(0, 0), q=(0, 0), required=(0, 0, 0, 0), beta=-1.0, Tx=0, Vx=5000, d=(0, p, 0, p), prior=(0, 0),
                a_logits=0, answers=0, A=5000, gamma=-1.0, invalid=nan) == 0
    # 3. the entry point's own pointers, shapes of the given terms, beta -- before the answer term's
    assert call(x=(0, p)) == _hip.EINVAL and call(x=(p, 0)) == _hip.EINVAL
    assert call(q=(0, p)) == _hip.EINVAL and call(q=(p, 0)) == _hip.EINVAL
    for missing in range(4):
        assert call(required=tuple(0 if i == missing else p for i in range(4))) == _hip.EINVAL, missing
    assert call(prior=(p, 0)) == _hip.EINVAL and call(prior=(0, 0), d=(0, p, 0, 0)) == _hip.EINVAL
    for shape in (dict(Tx=0), dict(Vx=0), dict(Tq=0), dict(Vq=-1), dict(Tp=0), dict(Vp=0)):
        assert call(**shape) == _hip.EINVAL, shape
    for beta in (-0.5, inf, -inf, nan):
        assert call(beta=beta) == _hip.EINVAL, beta
    # 4. - 7. the answer term: its pointers, the number of answers, the weight, log p(a | an invalid program)
    assert call(a_logits=0) == _hip.EINVAL and call(answers=0) == _hip.EINVAL
    assert call(a_logits=0, d=(0, 0, 0, p)) == _hip.EINVAL
    for A in (0, -3):
        assert call(A=A) == _hip.EINVAL, A
    for gamma in (-0.5, inf, -inf, nan):
        assert call(gamma=gamma) == _hip.EINVAL, gamma
    for invalid in (nan, 0.5, inf):
        assert call(invalid=invalid) == _hip.EINVAL, invalid
    # ... all of them before any shape: an argument error with a width that is too large is still an argument error
    for wide in (dict(Vx=1025), dict(A=1025), dict(n=1 << 30, samples=64)):
        assert call(beta=-1.0, **wide) == _hip.EINVAL and call(answers=0, **wide) == _hip.EINVAL
        assert call(gamma=nan, **wide) == _hip.EINVAL and call(invalid=1.0, **wide) == _hip.EINVAL
    assert call(A=0, Vq=4000) == _hip.EINVAL
    # 8. the shapes
    for shape in (dict(A=1025), dict(A=1 << 20), dict(Vx=1025), dict(Vq=1025), dict(Vp=1025)):
        assert call(**shape) == _hip.ESHAPE, shape
    assert call(n=1 << 30, samples=64) == _hip.ESHAPE           # more rows than an int32 counts
    # what passes every check is not tried here: it would launch.  0 and -inf are allowed values of invalid_log_answer and 0
    # of the weight -- shown by a shape error, which comes after them
    assert call(invalid=0.0, A=1025) == _hip.ESHAPE and call(invalid=-inf, A=1025) == _hip.ESHAPE
    assert call(gamma=0.0, A=1025) == _hip.ESHAPE


# ---- the option rules -----------------------------------------------------------------------------------------------------

class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the options are checked before any model is touched (%s)" % name)


def test_option_rules_of_the_loss():
    from probnmn import _hip
    from probnmn.modules.importance_weighted import joint_importance_weighted_bound

    def term(R=6, T=2, V=4, dtype=torch.float32):
        return torch.zeros(R, T, V, dtype=dtype), torch.zeros(R, T, dtype=torch.long), 0

    def answer(R=6, G=3, A=5, dtype=torch.float32, answers_dtype=torch.long, valid=None):
        return torch.zeros(R, A, dtype=dtype), torch.zeros(G, dtype=answers_dtype), valid

    x, q, p = term(), term(T=3), term()
    for samples in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            joint_importance_weighted_bound(x, q, p, answer=answer(), samples=samples)
    for beta in (-1.0, float("nan"), float("inf"), "much", None, True):
        with pytest.raises(ValueError):
            joint_importance_weighted_bound(x, q, p, answer=answer(), samples=2, beta=beta)
    for weight in (-1.0, float("nan"), float("inf"), "much", None, True):
        with pytest.raises(ValueError):
            joint_importance_weighted_bound(x, q, p, answer=answer(), samples=2, answer_weight=weight)
    for invalid in (0.5, float("nan"), float("inf"), "low", True):
        with pytest.raises(ValueError):
            joint_importance_weighted_bound(x, q, p, answer=answer(), samples=2, invalid_log_answer=invalid)
    for bad in (None, answer()[:2], answer(dtype=torch.float64), answer(answers_dtype=torch.int32), answer(G=6), answer(A=0),
                answer(A=1025), answer(R=8, G=4), answer(valid=torch.ones(6, dtype=torch.long)),
                answer(valid=torch.ones(5, dtype=torch.int32)), (torch.zeros(6, 1, 5), torch.zeros(3, dtype=torch.long), None)):
        with pytest.raises(ValueError):
            joint_importance_weighted_bound(x, q, p, answer=bad, samples=2)
    with pytest.raises(ValueError):
        joint_importance_weighted_bound(x, q, p, answer=answer(), samples=4)            # 6 rows are not questions of 4
    with pytest.raises(ValueError):
        joint_importance_weighted_bound(x, term(R=8), p, answer=answer(), samples=2)    # the terms disagree on the rows
    with pytest.raises(ValueError):
        joint_importance_weighted_bound(term(dtype=torch.float64), q, p, answer=answer(), samples=2)
    with pytest.raises(ValueError):
        joint_importance_weighted_bound(None, q, p, answer=answer(), samples=2)
    with pytest.raises(TypeError):
        joint_importance_weighted_bound(x, q, p, samples=2)                             # the answer is not optional
    with pytest.raises(_hip.HipLibraryError):
        joint_importance_weighted_bound(x, q, p, answer=answer(), samples=2)            # well formed, on the host: no CPU path
    with pytest.raises(_hip.HipLibraryError):
        joint_importance_weighted_bound(x, q, None, answer=answer(G=2, valid=torch.ones(6, dtype=torch.int32)), samples=3, beta=0.0,
                                        answer_weight=0.0, invalid_log_answer=-float("inf"))


def test_option_rules_of_the_trainer_and_the_evaluator():
    from types import SimpleNamespace

    from probnmn import trainers
    from probnmn.evaluators import evaluate_joint_evidence
    from probnmn.models import ProgramGenerator
    from probnmn.trainers.importance_weighted import ImportanceWeightedJointStep, importance_weighted_joint_options
    from probnmn.vocabulary import Vocabulary

    assert trainers.ImportanceWeightedJointStep is ImportanceWeightedJointStep
    u = _Untouchable()
    half = SimpleNamespace(token_class=np.zeros(4, np.uint8))
    for options in (dict(num_samples=1), dict(num_samples=0), dict(num_samples=65), dict(num_samples=4.0), dict(num_samples=True),
                    dict(beta=-0.1), dict(beta=float("nan")), dict(beta=float("inf")), dict(beta="0.1x"),
                    dict(answer_weight=-0.1), dict(answer_weight=float("nan")), dict(answer_weight=float("inf")),
                    dict(answer_weight=None), dict(constraint=3), dict(constraint=half), dict(train_modules=1),
                    dict(train_modules=None)):
        with pytest.raises(ValueError):
            ImportanceWeightedJointStep(u, u, u, u, **options)
    assert importance_weighted_joint_options(2, 0, 0, None, False) == (2, 0.0, 0.0, None, False)
    assert importance_weighted_joint_options(64, 0.1, 2, None, True)[::2] == (64, 2.0, True)
    # samples and scores must come from one q: encoder dropout in the generator is refused, before the other models are touched
    with pytest.raises(ValueError, match="dropout"):
        ImportanceWeightedJointStep(ProgramGenerator(Vocabulary.clevr(), dropout=0.2), u, u, u)
    for options in (dict(num_samples=0), dict(num_samples=65), dict(num_samples=2.5), dict(num_samples=False),
                    dict(constraint="clevr"), dict(constraint=half), dict(answer_weight=-1.0), dict(answer_weight=float("nan")),
                    dict(answer_weight="x")):
        with pytest.raises(ValueError):
            evaluate_joint_evidence(u, u, u, u, u, **options)
