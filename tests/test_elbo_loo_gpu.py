"""The leave-one-out kernel behind ``pnmn_joint_objective`` (no baseline pointer; the flag's place holds K) -- K sampled
programs per question, each reward centred by the mean reward of the question's other samples -- on the MI355X: against
the fp64 host statement (tests/helpers/loo_reference.py) through ``elbo.objective`` / ``J.backward()`` and through
``combine``, the same bits for a question alone and in a batch, and the argument checks of the entry point."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from loo_reference import loo_objective_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA, BETA, DECAY, B0 = 100.0, 0.1, 0.9, 0.37


def _inputs(nq, K, m, with_nmn, requires_grad=True):
    """Per-row losses of nq * K sampled and m supervised rows (fp32 on the device, the values the reference reads)."""
    g = torch.Generator().manual_seed(nq * 131 + K * 17 + m)
    n = nq * K
    rows = lambda k: (torch.rand(k, generator=g) * 3 + 0.1).to(DEV).requires_grad_(requires_grad)  # noqa: E731
    return {"pg": rows(n), "prior": rows(n).detach(), "nmn": rows(n) if with_nmn else None, "pg_sup": rows(m), "qr": rows(n + m)}


def _reference(x, w_u, w_s, gamma, nq, K, m):
    host = lambda t: None if t is None else t.detach().cpu().double().numpy()  # noqa: E731
    return loo_objective_reference(host(x["pg"]), host(x["qr"]), host(x["prior"]), host(x["nmn"]), host(x["pg_sup"]),
                                   w_u, w_s, ALPHA, BETA, gamma, nq, K, m)


CASES = [(1, 2, 0, True, False), (3, 3, 5, False, True), (5, 16, 0, True, True), (0, 4, 9, False, False),
         (300, 4, 212, True, True)]  # the last: more rows than the workgroup has threads


@pytest.mark.parametrize("nq,K,m,with_nmn,weighted", CASES)
def test_kernel_equals_the_host_statement(nq, K, m, with_nmn, weighted):
    """Statistics, reward variance, objective and every per-row gradient (tolerances of tests/test_elbo_gpu.py for
    pnmn_joint_objective); the moving baseline is left alone."""
    from probnmn.modules.elbo import JointTrainingElbo

    n = nq * K
    x = _inputs(nq, K, m, with_nmn)
    gamma = 1.5 if with_nmn else 0.0
    # (fp32 weights, as the kernel reads them)
    wu, ws = (float(np.float32(0.8)), float(np.float32(1.3))) if weighted else (1.0, 1.0)
    w_u = torch.tensor(wu, device=DEV) if weighted else 1.0
    w_s = torch.tensor(ws, device=DEV) if weighted else 1.0
    elbo = JointTrainingElbo(None, None, None, None, beta=BETA, gamma=gamma, baseline_decay=DECAY, num_samples=K,
                             baseline="leave_one_out")
    elbo._reinforce._baseline = torch.tensor(B0, device=DEV)
    J, stats = elbo.objective(x["pg"] if n else None, x["qr"], x["prior"] if n else None, x["nmn"] if n else None,
                              x["pg_sup"] if m else None, w_u, w_s, ALPHA, gamma, n, m)
    J.backward()
    ref = _reference(x, wu, ws, gamma, nq, K, m)
    print("J %.8g (host %.8g)" % (float(J.detach()), ref["J"]))
    assert float(elbo._reinforce._baseline) == float(np.float32(B0))  # neither read nor written
    keys = ["program_generation_gt", "question_reconstruction_gt"] if m else []
    keys += ["reconstruction_likelihood", "kl_divergence", "elbo", "reinforce_reward", "reward_variance"] if n else []
    keys += ["nmn_loss"] if (n and with_nmn) else []
    for k in keys:
        print("%s %.8g (host %.8g)" % (k, float(stats[k]), ref["stats"][k]))
        assert float(stats[k]) == pytest.approx(ref["stats"][k], rel=1e-5, abs=1e-5), k
    if not n:
        assert float(stats["reward_variance"]) == 0.0 and float(stats["elbo"]) == 0.0
    assert float(J.detach()) == pytest.approx(ref["J"], rel=1e-5, abs=1e-4)
    for name in ("pg", "qr", "nmn", "pg_sup"):
        leaf, want = x[name], ref["grads"][name]
        if leaf is None or leaf.numel() == 0 or leaf.grad is None:
            assert leaf is None or leaf.numel() == 0 or (name == "nmn" and not n), name
            continue
        torch.testing.assert_close(leaf.grad.cpu().double(), torch.from_numpy(want), rtol=1e-5, atol=1e-6,
                                   msg=lambda msg, name=name: "%s: %s" % (name, msg))


@pytest.mark.parametrize("with_nmn", [False, True])
def test_device_combine_has_the_keys_and_gradients_of_the_fused_path(with_nmn):
    """``combine`` on device tensors under leave-one-out: the kernel with w_u = 1 and m = 0; d mean(elbo) / d pg, d qr and
    d mean(nmn) / d nmn against the host statement, the moving baseline untouched."""
    from probnmn.modules.elbo import JointTrainingElbo, QuestionCodingElbo

    nq, K = 7, 3
    x = _inputs(nq, K, 0, with_nmn)
    gamma = 2.0 if with_nmn else 0.0
    if with_nmn:
        elbo = JointTrainingElbo(None, None, None, None, beta=BETA, gamma=gamma, num_samples=K, baseline="leave_one_out")
        out = elbo.combine(x["pg"], x["qr"], x["prior"], {"loss": x["nmn"]})
        (gamma * out["nmn_loss"] - out["elbo"]).backward()
    else:
        elbo = QuestionCodingElbo(None, None, None, beta=BETA, num_samples=K, baseline="leave_one_out")
        out = elbo.combine(x["pg"], x["qr"], x["prior"])
        (-out["elbo"]).backward()
    ref = _reference(x, 1.0, 1.0, gamma, nq, K, 0)
    want_keys = ["reconstruction_likelihood", "kl_divergence", "elbo", "reinforce_reward", "reward_variance"] + (["nmn_loss"] if with_nmn else [])
    assert sorted(out) == sorted(want_keys)
    for k in want_keys:
        assert float(out[k].detach()) == pytest.approx(ref["stats"][k], rel=1e-5, abs=1e-5), k
    for name in ("pg", "qr") +(("nmn",) if with_nmn else ()):
        torch.testing.assert_close(x[name].grad.cpu().double(), torch.from_numpy(ref["grads"][name]), rtol=1e-5, atol=1e-6)
    assert elbo._reinforce._baseline is None
    with pytest.raises(ValueError):  # rows that are no whole number of groups
        elbo.combine(x["pg"][:-1], x["qr"][:-1], x["prior"][:-1], *([{"loss": x["nmn"][:-1]}] if with_nmn else []))


def test_device_combine_of_an_empty_batch_goes_backward():
    """No sampled rows at all (an idle shard): zeros out, and backward hands every input an empty gradient."""
    from probnmn.modules.elbo import JointTrainingElbo

    x = _inputs(0, 3, 0, True)
    elbo = JointTrainingElbo(None, None, None, None, beta=BETA, gamma=2.0, num_samples=3, baseline="leave_one_out")
    out = elbo.combine(x["pg"], x["qr"], x["prior"], {"loss": x["nmn"]})
    assert all(float(v.detach()) == 0.0 for v in out.values())
    (2.0 * out["nmn_loss"] - out["elbo"]).backward()
    for name in ("pg", "qr", "nmn"):
        assert x[name].grad is not None and x[name].grad.numel() == 0, name


def _call(x, nq, K, m, w_u=None, gamma=1.5, d_pg="own", samples=None, rows=None):
    """The entry point itself: (return code, stats[11], J, d_pg, d_qr)."""
    from probnmn import _hip

    n = nq * K
    ptr = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    stats = torch.zeros(12, device=DEV)
    g_pg, g_qr = torch.zeros(max(n, 1), device=DEV), torch.zeros(max(n + m, 1), device=DEV)
    g_nmn, g_pgs = torch.zeros(max(n, 1), device=DEV), torch.zeros(max(m, 1), device=DEV)
    rc = _hip.lib().pnmn_joint_objective(
        ptr(x["pg"]), ptr(x["qr"]), ptr(x["prior"]), ptr(x["nmn"]), ptr(x["pg_sup"]), 0, ptr(w_u), 0, ALPHA, BETA, gamma, 0.0,
        K if samples is None else samples, n if rows is None else rows, m, stats.data_ptr(), stats.data_ptr() + 44,
        g_pg.data_ptr() if d_pg == "own" else 0,
        g_qr.data_ptr(), g_nmn.data_ptr() if x["nmn"] is not None else 0, g_pgs.data_ptr(), _hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, stats[:11].cpu(), float(stats[11]), g_pg[:n].cpu(), g_qr[:n + m].cpu()


def test_a_question_has_the_same_bits_alone_and_in_a_batch():
    """Question 7's d_pg rows out of the 300-question call against a call holding that question alone.  A row sees the batch
    only through the factor s = w_u / N, which the kernel hands back as d_qr of a sampled row: the lone call gets
    w_u' = 4 s with N' = 4, so s' = s exactly."""
    nq, K, m, q = 300, 4, 212, 7
    x = _inputs(nq, K, m, True, requires_grad=False)
    w_u = torch.tensor(0.8, device=DEV)
    rc, stats, J, d_pg, d_qr = _call(x, nq, K, m, w_u)
    assert rc == 0 and float(stats[9]) == nq * K and J == float(stats[8])
    s = d_qr[0]
    assert bool((d_qr[:nq * K] == s).all())
    rows = slice(q * K, (q + 1) * K)
    alone = {k: (None if v is None else v[rows].contiguous()) for k, v in x.items()}
    alone["pg_sup"] = None
    w_alone = (s * 4.0).to(DEV)  # (a power of two: exact)
    rc, stats1, _, d_pg1, d_qr1 = _call(alone, 1, K, 0, w_alone)
    assert rc == 0 and float(stats1[9]) == K
    assert bool((d_qr1 == s).all())
    assert torch.equal(d_pg1, d_pg[rows])
    assert float(d_pg1.abs().min()) > 0.0
    # sum(c) is zero up to rounding: a row's c carries at most ~(K + 2) roundings of a number of size |S_q| <= K max|R|
    R = _reference(x, 0.8, 1.0, 1.5, nq, K, m)["R"]
    assert abs(float(stats[5])) <= nq * K * (K + 2) * 2.0 ** -24 * K * float(np.abs(R).max())


def test_entry_point_refuses_bad_arguments():
    from probnmn import _hip

    x = _inputs(3, 4, 2, True, requires_grad=False)
    assert _call(x, 3, 4, 2)[0] == 0
    assert _call(x, 3, 4, 2, samples=1)[0] == _hip.EINVAL
    assert _call(x, 3, 4, 2, samples=65)[0] == _hip.EINVAL
    assert _call(x, 0, 4, 2, samples=1)[0] == _hip.EINVAL  # (also without sampled rows)
    assert _call(x, 3, 4, 2, d_pg=None)[0] == _hip.EINVAL  # rows present, nowhere to put their derivative
    assert _call(x, 0, 4, 2, d_pg=None)[0] == 0            # no sampled rows: not needed
    assert _call(x, -1, 4, 2)[0] == _hip.EINVAL
    assert _call(x, 3, 4, 2, rows=11)[0] == _hip.EINVAL    # rows that are no whole number of questions
    for flag in (0, 1):  # what was refused for its missing baseline before there was a second estimator still is
        assert _call(x, 3, 4, 2, samples=flag)[0] == _hip.EINVAL
