"""``pnmn_hypothesis_posterior``'s GRADIENT MODE and the autograd node on it, on the MI355X: the kernel against the fp64
reference of tests/helpers/sequence_marginal_reference.py over ragged groups at the first width of every kernel variant, the
outputs it shares with a plain launch (bitwise), bitwise independence of a group from its batch, clamped group bounds, the
existing sequence-loss kernels as a second reference, and ``_SequenceMarginalLoss`` on leaf tensors.

Tolerance: the project's bar for a posterior share times a softmax difference, ``row_bars`` of tests/test_marginal_loss_gpu.py
-- |w_k| * 2e-5 * (1 + the largest |score| among the group's usable rows), absolute: the gradient is w_k exp(a difference of
scores) times a difference of magnitude <= 1, so it inherits the scores' absolute error.  Zeros and signs are exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from sequence_marginal_cases import DEAD_GROUP, SEEDS, TX, WEIGHTS, ragged_inputs, requirements, satisfies  # noqa: E402
from sequence_marginal_reference import sequence_marginal_reference  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64     # guard words on either side of every output buffer
SHARED = ("log_posterior", "log_evidence", "support")
INVALID_PROGRAM_LOSS = np.float32(3.33)


def launch(x, z, log_q, group_start, weights, slots=("x", "z"), n_rows=None):
    """One ``pnmn_hypothesis_posterior`` launch on numpy inputs: in gradient mode with the given ``slots`` (``d_x`` /
    ``d_z`` where a plain launch has ``log_px`` / ``log_pz``, no ``best_row``), or plain (``slots=None``).  Every output lies
    between GUARD sentinel words, which must come back untouched; the token rows are handed over with a stride wider than T.
    Returns the outputs as numpy (what no group covers keeps the sentinel -777)."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    R = n_rows if n_rows is not None else next(len(a[0]) if isinstance(a, tuple) else len(a) for a in (x, z, log_q) if a is not None)
    G = len(group_start) - 1
    up = lambda t: (t if t.numel() else t.new_zeros(1)).to(dev)  # noqa: E731  (a null pointer means "not given")

    def term(t):
        if t is None:
            return None, (0, 0, 0), (1, 1, 0)
        logits, tokens, pad = t
        wide = torch.full((R, tokens.shape[1] + 2), 12345, dtype=torch.long)
        wide[:, :tokens.shape[1]] = torch.from_numpy(np.ascontiguousarray(tokens))
        d_logits, d_tokens = up(torch.from_numpy(np.ascontiguousarray(logits, np.float32))), up(wide)
        return (d_logits, d_tokens), (d_logits.data_ptr(), d_tokens.data_ptr(), wide.stride(0)), (logits.shape[1], logits.shape[2], pad)

    keep_x, x_args, (Tx, Vx, pad_x) = term(x)
    keep_z, z_args, (Tz, Vz, pad_z) = term(z)
    d_q = None if log_q is None else up(torch.from_numpy(np.ascontiguousarray(log_q, np.float32)))
    d_start = torch.from_numpy(np.asarray(group_start, np.int64)).to(torch.int32).to(dev)
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    grad = slots is not None
    bufs = {"log_posterior": torch.full((R + 2 * GUARD,), -777.0, **f), "log_evidence": torch.full((G + 2 * GUARD,), -777.0, **f),
            "support": torch.full((G + 2 * GUARD,), -777, **i)}
    if grad:
        if "x" in slots:
            bufs["d_x"] = torch.full((R * Tx * Vx + 2 * GUARD,), -777.0, **f)
        if "z" in slots:
            bufs["d_z"] = torch.full((R * Tz * Vz + 2 * GUARD,), -777.0, **f)
    else:
        bufs.update(log_px=torch.full((R + 2 * GUARD,), -777.0, **f), log_pz=torch.full((R + 2 * GUARD,), -777.0, **f),
                    best_row=torch.full((G + 2 * GUARD,), -777, **i))
    ptr = lambda name: bufs[name][GUARD:].data_ptr() if name in bufs else 0  # noqa: E731
    rc = _hip.lib().pnmn_hypothesis_posterior(
        *x_args, *z_args, 0 if d_q is None else d_q.data_ptr(), d_start.data_ptr(), *(float(w) for w in weights), pad_x, pad_z,
        ptr("d_x") if grad else ptr("log_px"), ptr("d_z") if grad else ptr("log_pz"), ptr("log_posterior"), ptr("log_evidence"),
        ptr("best_row"), ptr("support"), G, R, Tx, Vx, Tz, Vz, _hip.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == -777).all() and (host[-GUARD:] == -777).all(), name
        out[name] = host[GUARD:-GUARD]
    if "d_x" in out:
        out["d_x"] = out["d_x"].reshape(R, Tx, Vx)
    if "d_z" in out:
        out["d_z"] = out["d_z"].reshape(R, Tz, Vz)
    return out


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def row_bars(ref, start, w):
    """|w| * 2e-5 * (1 + largest |score| of the group), spread over the group's rows (tests/test_marginal_loss_gpu.py)."""
    per_row = np.zeros(ref["score"].size)
    for g in range(len(start) - 1):
        per_row[start[g]:start[g + 1]] = abs(w) * 2e-5 * (1.0 + ref["max_abs_score"][g])
    return per_row


def check_gradient(d, want, term, usable, bar, w):
    """A term's gradient of a launch whose groups cover every row, against the reference; returns the largest error / bar."""
    logits, tokens, pad = term
    assert not np.isnan(d).any() and (d[~usable] == 0).all() and (d[tokens == pad] == 0).all()  # zeros, exactly
    if w == 0.0:
        assert (d == 0).all()
        return 0.0
    assert (d[np.isneginf(logits)] == 0).all()
    scored = usable[:, None] & (tokens != pad)
    target = np.zeros(d.shape, bool)
    r, t = np.nonzero(scored)
    target[r, t, tokens[r, t]] = True
    assert (d[target] <= 0).all() and (d[scored][~target[scored]] >= 0).all()  # the target pulls down, the others up: exactly
    bars = np.broadcast_to(bar[:, None], tokens.shape)
    assert (np.abs(d.astype(np.float64).sum(-1))[scored] <= bars[scored]).all()  # a scored step of a usable row sums to 0
    err = np.abs(d.astype(np.float64) - want) / np.maximum(bar, 1e-300)[:, None, None]
    worst = float(err[usable].max()) if usable.any() else 0.0
    assert worst <= 1.0, worst
    return worst


@pytest.mark.parametrize("case", sorted(SEEDS))
def test_gradient_kernel_against_fp64_reference(case):
    Vx, Vz, Tx = case
    x, z, log_q, start = ragged_inputs(Vx, Vz, SEEDS[case], Tx=Tx)
    assert len(start) - 1 == 37
    requirements(x, z, log_q, start)
    for weights in WEIGHTS:
        ref = sequence_marginal_reference(x, z, log_q, start, weights)
        assert satisfies(ref) and ref["covered"].all() and ref["support"][0] == 0 and ref["support"][DEAD_GROUP] == 0
        usable, sup = ref["usable"], ref["support"] > 0
        plain = launch(x, z, log_q, start, weights, slots=None)
        for slots in (("x", "z"), ("x",), ("z",)):
            got = launch(x, z, log_q, start, weights, slots=slots)
            assert set(got) == set(SHARED) | {"d_" + k for k in slots}
            for k, term, w in (("x", x, weights[0]), ("z", z, weights[1])):
                if k in slots:
                    worst = check_gradient(got["d_" + k], ref["d_%s_logits" % k], term, usable, row_bars(ref, start, w), w)
                    print("V = %s, Tx = %d, weights %s, slots %s: largest |d_%s_logits - reference| / bar %.3g over %d usable rows"
                          % ((Vx, Vz), Tx, weights, "+".join(slots), k, worst, int(usable.sum())))
            # the loss itself, and every output the two modes share: the bits of a plain launch on the same inputs
            assert (np.abs(got["log_evidence"][sup] - ref["log_evidence"][sup]) <= 1e-5 * (1 + ref["max_abs_score"][sup])).all()
            assert np.isneginf(got["log_evidence"][~sup]).all() and np.array_equal(got["support"], ref["support"])
            assert np.array_equal(np.isfinite(got["log_posterior"]), usable)
            for name in SHARED:
                assert np.array_equal(bits(got[name]), bits(plain[name])), (name, slots)
    # no coefficient on either sequence term: every written value is 0 -- and every row is written
    got = launch(x, z, log_q, start, (0.0, 0.0, 1.0))
    assert (got["d_x"] == 0).all() and (got["d_z"] == 0).all() and (got["support"] > 0).sum() >= 28
    plain = launch(x, z, log_q, start, (0.0, 0.0, 1.0), slots=None)
    for name in SHARED:
        assert np.array_equal(bits(got[name]), bits(plain[name])), name


def test_a_groups_gradient_is_the_same_bits_alone_and_in_a_batch():
    case = (65, 64, TX)
    x, z, log_q, start = ragged_inputs(case[0], case[1], SEEDS[case])
    weights = WEIGHTS[0]
    whole = launch(x, z, log_q, start, weights)
    again = launch(x, z, log_q, start, weights)
    for name in whole:
        assert np.array_equal(bits(whole[name]), bits(again[name])), name
    for g in (0, 3, 4, DEAD_GROUP, 6, 7, 11, 20, 36):
        lo, hi = int(start[g]), int(start[g + 1])
        cut = lambda t: (t[0][lo:hi], t[1][lo:hi], t[2])  # noqa: E731
        alone = launch(cut(x), cut(z), log_q[lo:hi], [0, hi - lo], weights, n_rows=hi - lo)
        for name in ("d_x", "d_z", "log_posterior"):
            assert np.array_equal(bits(alone[name]), bits(whole[name][lo:hi])), (g, name)
        assert bits(alone["log_evidence"])[0] == bits(whole["log_evidence"])[g] and alone["support"][0] == whole["support"][g]


def test_group_bounds_are_clamped_into_the_arrays():
    """The three malformed ``group_start`` cases of tests/test_hypothesis_posterior_gpu.py in gradient mode: every bound is
    clamped into [0, n_rows] with end >= start, so nothing outside the arrays is written (``launch`` checks the guard words)."""
    case = (3, 2, TX)
    x, z, log_q, start = ragged_inputs(case[0], case[1], SEEDS[case])
    R = int(start[-1])
    weights = WEIGHTS[0]
    base = launch(x, z, log_q, start, weights)

    # a last entry beyond n_rows and a first one below 0 clamp to what they should have been: nothing changes
    for last in (R + 1000, 2 ** 31 - 1):
        bad = start.astype(np.int64)
        bad[-1], bad[0] = last, -5
        got = launch(x, z, log_q, bad, weights)
        for name in base:
            assert np.array_equal(bits(got[name]), bits(base[name])), (last, name)

    # every bound out of range on the same side: no group has a row, nothing but the group outputs is written
    for bad in (np.full(38, -9), np.full(38, R + 7)):
        got = launch(x, z, log_q, bad, weights)
        assert (got["support"] == 0).all() and np.isneginf(got["log_evidence"]).all()
        assert all((got[name] == -777).all() for name in ("d_x", "d_z", "log_posterior"))

    # a decreasing pair: start[4] = 30 > start[5] = 22.  Group 3 becomes rows [3, 30), group 4 is empty; groups 3 and 5 share
    # rows 22 .. 29, which either may write: every OTHER group keeps its bits, and a row only one group covers is uncovered
    # by none
    assert start[3] == 3 and start[4] == 6 and start[5] == 22
    bad = start.copy()
    bad[4] = 30
    got = launch(x, z, log_q, bad, weights)
    others = np.array([g for g in range(37) if g not in (3, 4, 5)])
    for name in ("log_evidence", "support"):
        assert np.array_equal(bits(got[name])[others], bits(base[name])[others]), name
    assert got["support"][4] == 0 and np.isneginf(got["log_evidence"][4])
    outside = np.r_[0:3, int(start[6]):R]
    for name in ("d_x", "d_z", "log_posterior"):
        assert np.array_equal(bits(got[name])[outside], bits(base[name])[outside]), name
        assert not (got[name] == -777).any(), name  # (every row is still covered)

    # rows that no group covers are not written
    got = launch(x, z, log_q, [3, 3, 5], weights)
    for name in ("d_x", "d_z", "log_posterior"):
        assert (got[name][:3] == -777).all() and (got[name][5:] == -777).all() and not (got[name][3:5] == -777).any(), name


def test_one_row_per_group_is_the_sequence_loss():
    """One row per group, weights (1, 0, 0): -log_evidence is ``pnmn_seq_nll_fwd``'s loss times (n + eps) and d_x_logits is
    ``pnmn_seq_nll_bwd``'s dlogits with dloss = n + eps, within rtol = atol = 1e-5 (the bar of
    tests/test_hip_kernels.py::test_answer_loss)."""
    from probnmn import _hip

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100)
    n, T, V, eps = 37, 7, 45, 1e-13
    logits = (rng.standard_normal((n, T, V)) * 3).astype(np.float32)
    tokens = rng.integers(1, V, (n, T)).astype(np.int64)
    tokens[rng.random((n, T)) < 0.3] = 0
    tokens[5] = 0  # an all-padding row: both sides give 0
    got = launch((logits, tokens, 0), None, None, np.arange(n + 1), (1.0, 0.0, 0.0), slots=("x",))
    d_logits, d_tokens = torch.from_numpy(logits).to(dev), torch.from_numpy(tokens).to(dev)
    loss, lse = torch.empty(n, device=dev), torch.empty(n, T, device=dev)
    _hip.check(_hip.lib().pnmn_seq_nll_fwd(d_logits.data_ptr(), T * V, d_tokens.data_ptr(), T, d_tokens.data_ptr(), T, 0,
                                           loss.data_ptr(), lse.data_ptr(), n, T, V, eps, _hip.stream_ptr(dev)), "seq_nll_fwd")
    scored = (tokens != 0).sum(1).astype(np.float32) + np.float32(eps)
    dloss, dlogits = torch.from_numpy(scored).to(dev), torch.empty(n, T, V, device=dev)
    _hip.check(_hip.lib().pnmn_seq_nll_bwd(d_logits.data_ptr(), T * V, d_tokens.data_ptr(), T, d_tokens.data_ptr(), T, 0,
                                           lse.data_ptr(), dloss.data_ptr(), dlogits.data_ptr(), T * V, n, T, V, eps,
                                           _hip.stream_ptr(dev)), "seq_nll_bwd")
    torch.cuda.synchronize()
    assert (got["support"] == 1).all() and (got["log_posterior"] == 0).all()
    np.testing.assert_allclose(-got["log_evidence"], loss.cpu().numpy() * scored, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got["d_x"], dlogits.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert (got["d_x"][tokens == 0] == 0).all() and (got["d_x"][tokens != 0] != 0).any() and got["log_evidence"][5] == 0


def test_autograd_node_on_leaf_tensors():
    from probnmn.modules.marginal_likelihood import sequence_marginal_loss

    dev = torch.device("cuda:0")
    case = (64, 45, TX)
    x, z, log_q, start = ragged_inputs(case[0], case[1], SEEDS[case])
    weights = WEIGHTS[0]
    ref = sequence_marginal_reference(x, z, log_q, start, weights)
    usable, sup = ref["usable"], ref["support"] > 0
    d_start = torch.from_numpy(start).to(dev)
    upstream = np.linspace(-2.0, 3.0, 37)
    group_of = np.repeat(np.arange(37), np.diff(start))
    tokens = [torch.from_numpy(t[1]).to(dev) for t in (x, z)]
    for scale in (np.ones(37), upstream):  # loss.sum(), then a different upstream gradient per group
        leaves = [torch.from_numpy(t[0]).to(dev).requires_grad_(True) for t in (x, z)]
        leaf_q = torch.from_numpy(log_q).to(dev).requires_grad_(True)
        loss, log_posterior, support = sequence_marginal_loss(x=(leaves[0], tokens[0], x[2]), z=(leaves[1], tokens[1], z[2]),
                                                              log_q=leaf_q, group_start=d_start, weights=weights)
        assert loss.requires_grad and not log_posterior.requires_grad and not support.requires_grad
        assert loss.grad_fn.buffers == (True, True)
        (loss * torch.from_numpy(scale).to(dev, torch.float32)).sum().backward()
        got = loss.detach().cpu().numpy()
        assert (np.abs(-got[sup] - ref["log_evidence"][sup]) <= 1e-5 * (1 + ref["max_abs_score"][sup])).all()
        assert (got[~sup] == INVALID_PROGRAM_LOSS).all() and np.array_equal(support.cpu().numpy(), ref["support"])
        assert np.array_equal(np.isfinite(log_posterior.cpu().numpy()), usable)
        by = np.maximum(np.abs(scale[group_of]), 1e-300)
        for leaf, name, w in ((leaves[0], "d_x_logits", weights[0]), (leaves[1], "d_z_logits", weights[1])):
            grad = leaf.grad.cpu().numpy().astype(np.float64)
            err = np.abs(grad - ref[name] * scale[group_of][:, None, None]) / (row_bars(ref, start, w) * by)[:, None, None]
            print("upstream %s: largest |%s - reference| / bar %.3g" % ("ones" if scale is not upstream else "per group", name, err[usable].max()))
            assert (err[usable] <= 1.0 + 1e-6).all() and (grad[~usable] == 0).all()  # (1e-6: the one fp32 multiply by the upstream value)
        grad = leaf_q.grad.cpu().numpy().astype(np.float64)
        err = np.abs(grad - ref["d_log_q"] * scale[group_of]) / (row_bars(ref, start, weights[2]) * by)
        print("    largest |d log_q - reference| / bar %.3g" % err[usable].max())
        assert (err[usable] <= 1.0 + 1e-6).all() and (grad[~usable] == 0).all()

    # a term whose logits do not require a gradient gets no buffer; nothing requires one: the plain launch, the same bits
    fixed_x = torch.from_numpy(x[0]).to(dev)
    leaf_z = torch.from_numpy(z[0]).to(dev).requires_grad_(True)
    q = torch.from_numpy(log_q).to(dev)
    only_z = sequence_marginal_loss(x=(fixed_x, tokens[0], x[2]), z=(leaf_z, tokens[1], z[2]), log_q=q, group_start=d_start, weights=weights)
    assert only_z[0].grad_fn.buffers == (False, True)
    only_z[0].sum().backward()
    assert np.array_equal(leaf_z.grad.cpu().numpy(), launch(x, z, log_q, start, weights, slots=("z",))["d_z"])
    none =sequence_marginal_loss(x=(fixed_x, tokens[0], x[2]), z=(leaf_z.detach(), tokens[1], z[2]), log_q=q, group_start=d_start, weights=weights)
    assert not none[0].requires_grad
    leaf_q = q.clone().requires_grad_(True)
    only_q = sequence_marginal_loss(x=(fixed_x, tokens[0], x[2]), z=(leaf_z.detach(), tokens[1], z[2]), log_q=leaf_q, group_start=d_start, weights=weights)
    assert only_q[0].grad_fn.buffers == (False, False)
    only_q[0].sum().backward()
    for a, b in zip(only_q, (loss, log_posterior, support)):  # (the gradient-mode launch of the loop above)
        assert np.array_equal(bits(a.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))
    assert (leaf_q.grad.cpu().numpy()[~usable] == 0).all() and (leaf_q.grad.cpu().numpy()[usable] <= 0).all()
