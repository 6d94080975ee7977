"""K sampled programs per unsupervised question in the question-coding and joint-training steps (``num_samples=K``) on the
MI355X.

Plumbing: with the moving baseline a K-sample step IS the one-sample step of the batch whose unsupervised rows were
physically replicated K-fold, in the same order -- identical programs, the same objective and gradients -- for plain-tensor
and resident features, and through the launch plan as through the eager passes.

Estimator: with the leave-one-out baseline (the default for K > 1) the step's objective and gradients are the host
statement (tests/helpers/loo_reference.py) applied to the step's own per-row losses, the moving baseline stays where it
was, and a question's replicas draw different programs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from loo_reference import loo_objective_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ELBO_KEYS = ("elbo", "kl_divergence", "reconstruction_likelihood", "reinforce_reward")


def _models(seed, nmn=False):
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    ms = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256)]
    if nmn:
        ms.append(NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64))
    return vocab, [m.to(DEV) for m in ms]


def _twin(seed, nmn=False):
    """Two sets of models with the same weights."""
    vocab, a = _models(seed, nmn)
    _, b = _models(seed + 100, nmn)
    for d, s in zip(b, a):
        d.load_state_dict(s.state_dict())
    return vocab, a, b


def _grads(models):
    return {"%d.%s" % (i, n): p.grad.detach().clone() for i, m in enumerate(models) for n, p in m.named_parameters()
            if p.grad is not None}


def _params(models):
    return {"%d.%s" % (i, n): p.detach().clone() for i, m in enumerate(models) for n, p in m.named_parameters()}


def _to_device(batch):
    out = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    out["supervision"] = batch["supervision"]  # host copy: no sync for the split
    return out


def _replicated(batch, K):
    """The batch with every unsupervised row K times, adjacent, everything else in place: its own unsupervised index list
    is the question-major replica list of the original's."""
    take = []
    for i, s in enumerate(batch["supervision"].tolist()):
        take += [i] * (1 if s else K)
    take = torch.tensor(take)
    return {k: (v.subset(take) if not isinstance(v, torch.Tensor) else v[take]) for k, v in batch.items()}


def _compare_with_replicated_batch(make_step, models_a, models_b, batch, K, lr, nmn_index=None):
    """``make_step(models, num_samples, baseline)``.  Tolerances: those of the grouped / ungrouped comparison of
    tests/test_joint_gpu.py -- the objective equal, every seq2seq gradient within 2e-6 of its largest entry (the embedding
    gradients are summed by atomics) -- and, for the NMN, whose weight gradients are sums by atomics, the 1e-4 of
    tests/test_feature_store_gpu.py.  After the Adam step no parameter is further than two steps of lr from its twin
    (the first Adam step moves every element by lr * sign(g), whatever the size of g)."""
    outs, grads = [], []
    for models, b, k in ((models_a, batch, K), (models_b, _replicated(batch, K), 1)):
        step = make_step(models, k, "moving")
        torch.manual_seed(21)
        outs.append(step.step(_to_device(b)))
        torch.cuda.synchronize()
        grads.append(_grads(models))
        outs[-1]["baseline"] = float(step.elbo._reinforce._baseline)
        step.close()
    n_unsup = int((batch["supervision"] == 0).sum())
    assert outs[0]["samples_per_question"] == K and outs[1]["samples_per_question"] == 1
    assert outs[0]["programs"].shape[0] == n_unsup * K
    assert torch.equal(outs[0]["programs"], outs[1]["programs"])
    assert "reward_variance" not in outs[0]["elbo"]
    print("objective", float(outs[0]["objective"]), float(outs[1]["objective"]))
    assert float(outs[0]["objective"]) == float(outs[1]["objective"])
    for k in ELBO_KEYS:
        assert float(outs[0]["elbo"][k]) == float(outs[1]["elbo"][k]), k
    assert outs[0]["baseline"] == outs[1]["baseline"]
    assert sorted(grads[0]) == sorted(grads[1]) and len(grads[0]) > 20
    for name in grads[0]:
        scale = float(grads[1][name].abs().max())
        bar = 1e-4 if (nmn_index is not None and name.startswith("%d." % nmn_index)) else 2e-6
        worst = float((grads[0][name] - grads[1][name]).abs().max())
        assert worst <= bar * scale + 1e-12, (name, worst, scale)
    pa, pb = _params(models_a), _params(models_b)
    for name in pa:
        assert float((pa[name] - pb[name]).abs().max()) <= 2.05 * lr, name


def _question_coding(models, num_samples, baseline, lr=1e-3):
    from probnmn.trainers.joint_training import QuestionCodingStep

    return QuestionCodingStep(*models[:3], objective="ours", alpha=100.0, beta=0.1, delta=0.99, lr=lr, num_samples=num_samples,
                              baseline=baseline)


def _joint(models, num_samples, baseline, lr=1e-4):
    from probnmn.trainers.joint_training import JointTrainingStep

    return JointTrainingStep(*models, objective="ours", alpha=100.0, beta=0.1, gamma=1.0, delta=0.99, lr=lr,
                             num_samples=num_samples, baseline=baseline)


def test_question_coding_three_samples_is_the_step_of_the_replicated_batch():
    from probnmn.data.synthetic import synthetic_batch

    vocab, a, b = _twin(1)
    batch = synthetic_batch(vocab, 12, seed=4, with_image=False)
    batch["supervision"] = torch.tensor([1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1])
    _compare_with_replicated_batch(_question_coding, a, b, batch, 3, 1e-3)


@pytest.mark.parametrize("resident", [False, True])
def test_joint_three_samples_is_the_step_of_the_replicated_batch(resident):
    from probnmn.data.feature_store import DeviceFeatureStore
    from probnmn.data.synthetic import synthetic_batch

    vocab, a, b = _twin(2, nmn=True)
    batch = synthetic_batch(vocab, 8, seed=6)
    batch["supervision"] = torch.tensor([0, 1, 0, 0, 1, 1, 0, 1])
    if resident:
        store = DeviceFeatureStore(batch["image"].numpy(), DEV)
        batch["image"] = store.batch(torch.tensor([5, 0, 3, 3, 7, 1, 2, 6]))  # (out of order, one row twice)
    _compare_with_replicated_batch(_joint, a, b, batch, 3, 1e-4, nmn_index=3)


@pytest.mark.parametrize("kind", ["question_coding", "joint"])
def test_two_samples_through_the_plan_equal_the_eager_passes(kind):
    """K = 2 with ``use_plan`` on and off (tolerances of tests/test_seq_plan_gpu.py): the plan takes the replicated index
    list as it is and is cached under n K sampled rows."""
    from probnmn.data.synthetic import synthetic_batch

    joint = kind == "joint"
    vocab, a, b = _twin(3, nmn=joint)
    batch = synthetic_batch(vocab, 14, seed=9, with_image=joint)
    batch["supervision"] = torch.tensor([0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0])
    n_unsup, n_sup = 8, 6
    outs, grads, plans = [], [], []
    for models, plan in ((a, True), (b, False)):
        step = (_joint if joint else _question_coding)(models, 2, None, lr=0.0)
        assert step.baseline == "leave_one_out"
        step.use_plan = plan
        torch.manual_seed(31)
        outs.append(step.step(_to_device(batch)))
        torch.cuda.synchronize()
        grads.append(_grads(models[:2]))
        plans.append(dict(step.__dict__.get("_plans") or {}))
        step.close()
    assert plans[0] and all(p is not False for p in plans[0].values()) and not plans[1]  # (the plan DID run ...)
    assert [(key[1], key[2]) for key in plans[0]] == [(2 * n_unsup, n_sup)]              # (... over n K sampled rows)
    assert outs[0]["programs"].shape[0] == 2 * n_unsup
    assert torch.equal(outs[0]["programs"], outs[1]["programs"])
    for k in ELBO_KEYS + ("reward_variance",):
        assert float(outs[0]["elbo"][k]) == pytest.approx(float(outs[1]["elbo"][k]), rel=2e-5, abs=2e-5), k
    assert float(outs[0]["objective"]) == pytest.approx(float(outs[1]["objective"]), rel=2e-5, abs=1e-4)
    if joint:
        assert float(outs[0]["loss"]["nmn"]) == pytest.approx(float(outs[1]["loss"]["nmn"]), rel=1e-5, abs=1e-5)
    assert sorted(grads[0]) == sorted(grads[1])
    for name in grads[0]:
        scale = float(grads[1][name].abs().max()) + 1e-12
        assert float((grads[0][name] - grads[1][name]).abs().max()) / scale < 2e-4, name


def test_question_coding_four_samples_is_the_leave_one_out_estimator():
    """``num_samples=4`` defaults to leave-one-out.  An eager twin with the same seeds captures its own per-row losses where
    the step hands them to ``elbo.objective`` and backpropagates the HOST statement's per-row derivatives through them; the
    step's objective is the host statement's, its gradients are the twin's (the step runs the launch plan, the twin the
    eager passes: the 2e-4 of tests/test_seq_plan_gpu.py, which the host statement's fp64 derivatives do not add to)."""
    from probnmn.data.synthetic import synthetic_batch

    K = 4
    vocab, a, b = _twin(5)
    batch = synthetic_batch(vocab, 12, seed=11, with_image=False)
    batch["supervision"] = torch.tensor([0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1])
    nq, m = 6, 6

    step = _question_coding(a, K, None, lr=0.0)
    assert step.baseline == "leave_one_out" and step.elbo.leave_one_out
    step.elbo._reinforce._baseline = torch.tensor(0.25, device=DEV)
    torch.manual_seed(41)
    out = step.step(_to_device(batch))
    torch.cuda.synchronize()
    assert float(step.elbo._reinforce._baseline) == 0.25  # the moving baseline is unchanged by the step
    assert out["samples_per_question"] == K and out["programs"].shape[0] == nq * K
    got = _grads(a[:2])

    twin = _question_coding(b, K, None, lr=0.0)
    twin.use_plan = False
    seen = {}

    def host_objective(pg, qr_rows, prior, nmn, pg_sup, w_u, w_s, alpha, gamma, n, m_):
        assert (n, m_, nmn) == (nq * K, m, None)
        f = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
        ref = seen["ref"] = loo_objective_reference(f(pg), f(qr_rows), f(prior), None, f(pg_sup), float(w_u), float(w_s), alpha,
                                                    twin.elbo._beta, gamma, nq, K, m)
        coef = {k: torch.from_numpy(v).to(DEV, torch.float32) for k, v in ref["grads"].items()}
        J = (coef["pg"] * pg).sum() + (coef["qr"] * qr_rows).sum() + (coef["pg_sup"] * pg_sup).sum()
        return J, {k: torch.tensor(v, device=DEV) for k, v in ref["stats"].items()}

    twin.elbo.objective = host_objective
    torch.manual_seed(41)
    out_b = twin.step(_to_device(batch))
    torch.cuda.synchronize()
    want, ref = _grads(b[:2]), seen["ref"]
    assert torch.equal(out["programs"], out_b["programs"])
    print("objective %.8g (host %.8g)" % (float(out["objective"]), ref["J"]))
    assert float(out["objective"]) == pytest.approx(ref["J"], rel=2e-5, abs=1e-4)
    for k in ELBO_KEYS + ("reward_variance",):
        assert float(out["elbo"][k]) == pytest.approx(ref["stats"][k], rel=2e-5, abs=2e-5), k
    assert ref["stats"]["reward_variance"] > 0.0
    assert sorted(got) == sorted(want) and len(got) > 20
    for name in got:
        scale = float(want[name].abs().max()) + 1e-12
        assert float((got[name] - want[name]).abs().max()) / scale < 2e-4, name


def test_replicas_of_a_question_draw_different_programs():
    """A freshly initialised generator over the CLEVR vocabularies, 16 questions, K = 4: the sampling decoder draws per row
    position, so at least one question's four programs are not all the same."""
    from probnmn.data.synthetic import synthetic_batch

    vocab, models = _models(7)
    batch = synthetic_batch(vocab, 16, seed=13, with_image=False)
    batch["supervision"][:] = 0
    step = _question_coding(models, 4, None, lr=0.0)
    torch.manual_seed(51)
    out = step.step(_to_device(batch))
    torch.cuda.synchronize()
    z = out["programs"].cpu().reshape(16, 4, -1)
    differing = sum(1 for q in range(16) if not all(torch.equal(z[q, 0], z[q, k]) for k in range(1, 4)))
    assert differing >= 1, differing
    assert "reward_variance" in out["elbo"] and float(out["elbo"]["reward_variance"]) > 0.0
