"""The multi-sample ELBO estimator with the leave-one-out baseline, without a GPU: the host statement
(tests/helpers/loo_reference.py) is unbiased by exhaustive enumeration, the CPU path of ``probnmn.modules.elbo.*.combine``
is that statement (values and autograd gradients), the constructors refuse what has no meaning, the defaults leave today's
outputs alone, and under data parallelism (gloo, two ranks) no rank waits in a baseline collective another rank skipped."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from loo_reference import leave_one_out_centre, loo_objective_reference  # noqa: E402


def _categorical(seed):
    rng = np.random.default_rng(seed)
    theta = rng.normal(size=3)
    q = np.exp(theta - theta.max())
    q /= q.sum()
    return theta, q, rng.normal(size=3) * 3.0 + 1.0  # logits, probabilities, arbitrary rewards


@pytest.mark.parametrize("samples", [2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_estimator_is_unbiased_by_enumeration(samples, seed):
    """E over all 3^K sample tuples of mean_i c_i grad log q(z_i) is the exact gradient of sum_z q(z) R(z) (R held constant):
    the baseline of a sample is a function of the OTHER samples only."""
    theta, q, R = _categorical(seed)
    score = np.eye(3) - q[None, :]  # d log q(z) / d theta, row z
    exact = q * (R - float(q @ R))  # d (sum_z q(z) R(z)) / d theta
    expected = np.zeros(3)
    for z in itertools.product(range(3), repeat=samples):
        z = list(z)
        c = leave_one_out_centre(R[z], samples).reshape(-1)
        expected += np.prod(q[z]) * (c[:, None] * score[z]).mean(0)
    assert np.abs(expected - exact).max() < 1e-12


@pytest.mark.parametrize("samples", [2, 3])
def test_product_cpu_path_is_unbiased_by_enumeration(samples):
    """The same through ``QuestionCodingElbo.combine`` on CPU tensors in fp64: the expected gradient of mean(kl) -- the only
    term of -elbo that reaches the generator -- is the exact gradient (the -beta logq term has expectation zero)."""
    from probnmn.modules.elbo import QuestionCodingElbo

    theta0, _, rewards = _categorical(5)
    beta = 0.1
    elbo = QuestionCodingElbo(None, None, None, beta=beta, num_samples=samples, baseline="leave_one_out")
    theta = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    logq_all = torch.log_softmax(theta, 0)
    q = logq_all.exp().detach().numpy()
    # R(z) = rec(z) + beta (logprior(z) - logq(z)) is to be `rewards`: pick rec, with a zero prior term
    rec = torch.tensor(rewards) + beta * logq_all.detach()
    expected = torch.zeros(3, dtype=torch.float64)
    for z in itertools.product(range(3), repeat=samples):
        z = torch.tensor(z)
        out = elbo.combine(-logq_all[z], -rec[z], torch.zeros(samples, dtype=torch.float64))
        (g,) = torch.autograd.grad(out["kl_divergence"], theta, retain_graph=True)
        expected += float(np.prod(q[z.numpy()])) * g
    exact = q * (rewards - float(q @ rewards))
    assert np.abs(expected.numpy() - exact).max() < 1e-12


def test_equal_rewards_centre_to_exactly_zero():
    for samples in (2, 3, 7, 64):
        R = np.full((4, samples), 1.2345678)
        assert (leave_one_out_centre(R, samples) == 0.0).all()
    ref = loo_objective_reference([0.5] * 6, [0.25] * 6, [0.125] * 6, None, None, 1.0, 1.0, 100.0, 0.1, 0.0, 2, 3, 0)
    assert (ref["c"] == 0.0).all() and ref["stats"]["reward_variance"] == 0.0


def _rows(n, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g, dtype=torch.float64) * 3 + 0.1).to(dtype)


@pytest.mark.parametrize("kind", ["joint", "question_coding"])
def test_cpu_combine_is_the_host_statement(kind):
    from probnmn.modules.elbo import JointTrainingElbo, QuestionCodingElbo

    K, nq, beta, gamma = 3, 4, 0.1, 1.5
    n = nq * K
    pg, qr = _rows(n, 1, torch.float64).requires_grad_(True), _rows(n, 2, torch.float64).requires_grad_(True)
    prior, nmn = _rows(n, 3, torch.float64), _rows(n, 4, torch.float64).requires_grad_(True)
    if kind == "joint":
        elbo = JointTrainingElbo(None, None, None, None, beta=beta, gamma=gamma, num_samples=K, baseline="leave_one_out")
        out = elbo.combine(pg, qr, prior, {"loss": nmn})
        J = gamma * out["nmn_loss"] - out["elbo"]
    else:
        gamma = 0.0
        elbo = QuestionCodingElbo(None, None, None, beta=beta, num_samples=K, baseline="leave_one_out")
        out = elbo.combine(pg, qr, prior)
        J = -out["elbo"]
    J.backward()
    ref = loo_objective_reference(pg.detach(), qr.detach(), prior, nmn.detach() if kind == "joint" else None, None,
                                  1.0, 1.0, 0.0, beta, gamma, nq, K, 0)
    assert float(J.detach()) == pytest.approx(ref["J"], rel=1e-12, abs=1e-12)
    keys = ["reconstruction_likelihood", "kl_divergence", "elbo", "reinforce_reward", "reward_variance"]
    keys += ["nmn_loss"] if kind == "joint" else []
    assert sorted(out) == sorted(keys)
    for k in keys:
        assert float(out[k]) == pytest.approx(ref["stats"][k], rel=1e-12, abs=1e-12), k
    np.testing.assert_allclose(pg.grad.numpy(), ref["grads"]["pg"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(qr.grad.numpy(), ref["grads"]["qr"], rtol=1e-12, atol=1e-14)
    if kind == "joint":
        np.testing.assert_allclose(nmn.grad.numpy(), ref["grads"]["nmn"], rtol=1e-12, atol=1e-14)
    assert elbo._reinforce._baseline is None  # the moving baseline was never touched


def test_constructors_refuse_what_has_no_meaning():
    from probnmn.modules.elbo import JointTrainingElbo, QuestionCodingElbo
    from probnmn.trainers.joint_training import JointTrainingStep, QuestionCodingStep

    for make in (lambda **kw: QuestionCodingElbo(None, None, None, **kw), lambda **kw: JointTrainingElbo(None, None, None, None, **kw)):
        with pytest.raises(ValueError):
            make(num_samples=1, baseline="leave_one_out")
        with pytest.raises(ValueError):
            make(baseline="leave_one_out")
        with pytest.raises(ValueError):
            make(num_samples=2, baseline="leave_oneout")
        with pytest.raises(ValueError):
            make(num_samples=0)
        for baseline in ("moving", "leave_one_out"):  # one bound for the modules and the trainers, under either baseline
            with pytest.raises(ValueError):
                make(num_samples=65, baseline=baseline)
            assert make(num_samples=64, baseline=baseline)._num_samples == 64
        assert make(num_samples=4, baseline="moving")._num_samples == 4
    with pytest.raises(ValueError):
        JointTrainingElbo(None, None, None, None, objective="baseline", num_samples=2)
    # the trainers: refused before a model is touched
    with pytest.raises(ValueError):
        JointTrainingStep(None, None, None, None, objective="baseline", num_samples=2)
    with pytest.raises(ValueError):
        JointTrainingStep(None, None, None, None, num_samples=1, baseline="leave_one_out")
    for baseline in (None, "moving", "leave_one_out"):
        with pytest.raises(ValueError):
            QuestionCodingStep(None, None, None, num_samples=65, baseline=baseline)
    with pytest.raises(ValueError):
        QuestionCodingStep(None, None, None, num_samples=2, baseline="loo")


def test_trainer_defaults_pick_the_baseline_by_sample_count():
    from probnmn.trainers.joint_training import _estimator, _replicate

    assert _estimator(1, None) == (1, "moving")
    assert _estimator(4, None) == (4, "leave_one_out")
    assert _estimator(4, "moving") == (4, "moving")
    nosup = torch.tensor([5, 2, 9])
    assert _replicate(nosup, 1) is nosup
    assert _replicate(nosup, 3).tolist() == [5, 5, 5, 2, 2, 2, 9, 9, 9]  # question-major


def test_defaults_give_todays_outputs():
    """num_samples=1, baseline="moving" -- spelled out or left to the defaults -- is the reference's estimator: the oracle's
    values, gradients and moving baseline over two calls."""
    from oracle import elbo_oracle
    from probnmn.modules.elbo import JointTrainingElbo

    n = 6
    for kwargs in ({}, {"num_samples": 1, "baseline": "moving"}):
        got = JointTrainingElbo(None, None, None, None, beta=0.1, gamma=1.5, baseline_decay=0.9, **kwargs)
        r = elbo_oracle.Reinforce(0.9)
        for call in range(2):
            a = [_rows(n, 10 + call), _rows(n, 20 + call), _rows(n, 30 + call), _rows(n, 40 + call)]
            b = [t.clone() for t in a]
            for t in (a[0], a[1], a[3], b[0], b[1], b[3]):
                t.requires_grad_(True)
            out = got.combine(a[0], a[1], a[2], {"loss": a[3]})
            want = elbo_oracle.joint_training_elbo(r, 0.1, 1.5, "ours", b[0], b[1], b[2], b[3])
            assert sorted(out) == sorted(want)
            (1.5 * out["nmn_loss"] - out["elbo"]).backward()
            (1.5 * want["nmn_loss"] - want["elbo"]).backward()
            for k in want:
                assert float(out[k]) == float(want[k]), k
            for x, y in zip(a, b):
                if x.requires_grad:
                    assert torch.equal(x.grad, y.grad)
            assert got._reinforce._reinforce_baseline == pytest.approx(r.baseline, abs=1e-7)


def test_multi_sample_forward_replicates_question_major():
    """``forward`` with num_samples=K hands the models K adjacent copies of every question (and answer, and image row)."""
    from probnmn.modules.elbo import JointTrainingElbo

    seen = {}

    def generator(question_tokens, decoding_strategy=None):
        seen["question"] = question_tokens
        n = question_tokens.size(0)
        return {"predictions": torch.zeros(n, 3, dtype=torch.long), "loss": _rows(n, 1).requires_grad_(True)}

    def other(key):
        def run(*args, **kw):
            seen[key] = args
            n = args[0].size(0)
            return {"loss": _rows(n, len(key))}
        return run

    elbo = JointTrainingElbo(generator, other("qr"), other("prior"), other("nmn"), beta=0.1, gamma=1.0, num_samples=3,
                             baseline="leave_one_out")
    question = torch.arange(8).reshape(4, 2)
    image = torch.arange(4.0).reshape(4, 1, 1, 1)
    answer = torch.tensor([7, 8, 9, 10])
    out = elbo(question, image, answer)
    assert seen["question"].tolist() == question.repeat_interleave(3, 0).tolist()
    assert seen["qr"][1].tolist() == question.repeat_interleave(3, 0).tolist()
    assert seen["nmn"][0].flatten().tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert seen["nmn"][2].tolist() == [7, 7, 7, 8, 8, 8, 9, 9, 9, 10, 10, 10]
    assert out["elbo"].ndim == 0 and "reward_variance" in out


# ---- data parallel, gloo on CPU ------------------------------------------------------------------------------------------
SUPERVISION = [1, 1, 1, 1, 0, 0, 1, 0]  # rank 0 = rows 0-2 holds no unsupervised row, rank 1 = rows 3-7


def _two_sample_step(kind="question_coding"):
    import test_parallel_trainers as base

    toy, _ = base._make(kind, "ours")  # (for its class: the product step over differentiable stand-ins of the model passes)
    pg, qr, prior = base._Toy(1), base._Toy(2), base._Toy(3)
    step = type(toy)(pg, qr, prior, objective="ours", alpha=100.0, beta=0.1, delta=0.5, num_samples=2)
    assert step.baseline == "leave_one_out"
    return step, (pg, qr)


def _run_two_samples(rows):
    import test_parallel_trainers as base

    step, models = _two_sample_step()
    out = step.step(base._batch(rows, SUPERVISION))
    assert out["samples_per_question"] == 2
    assert step.elbo._reinforce._baseline is None
    return [torch.zeros_like(p) if p.grad is None else p.grad.clone() for m in models for p in m.parameters()]


def _loo_worker(rank, world, port, out_path):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    grads = _run_two_samples(list(range(0, 3)) if rank == 0 else list(range(3, 8)))
    torch.save(grads, out_path + str(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_finish_a_two_sample_step_with_equal_gradients(tmp_path):
    """num_samples=2 (leave-one-out by default) on two gloo ranks, one of which holds no unsupervised row: both finish -- no
    rank sits in a baseline all-reduce the other one skipped -- with the same averaged gradient, which is the
    single-process gradient of the whole batch."""
    import torch.multiprocessing as mp

    import test_parallel_trainers as base

    out = str(tmp_path / "r")
    mp.spawn(_loo_worker, args=(2, base._free_port(), out), nprocs=2, join=True)
    got0, got1 = torch.load(out + "0"), torch.load(out + "1")
    want = _run_two_samples(list(range(8)))
    assert len(got0) == len(got1) == len(want) > 0
    for a, b, w in zip(got0, got1, want):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
        torch.testing.assert_close(a, w, rtol=1e-5, atol=1e-6)
