"""Rows grouped by length in the LSTM layer kernels (pnmn_length_order, pnmn_lstm_seq_fwd_ordered / _bwd_ordered): the order
against numpy's stable sort; the ordered kernels against the unordered entry points of the same kernel variant -- bit for bit
at every valid step, zeros where a tile skips steps, every output buffer pre-filled with NaN so that an element that must be
defined and is not shows; ``masked_lstm`` and one joint-training iteration with the switch on against off."""
import functools

import numpy as np
import pytest
import torch

from probnmn import _hip
from probnmn.modules.seq2seq_base import pack_fragments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 40  # rows of the token table


def _stream():
    return _hip.stream_ptr(torch.device(DEV))


def _length_order(last, T):
    B = last.numel()
    order = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tile_steps = torch.full(((B + 15) // 16,), -1, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pnmn_length_order(last.data_ptr(), B, T, order.data_ptr(), tile_steps.data_ptr(), _stream()), "length_order")
    return order, tile_steps


# name -> (B, T, steps per row); the kernels see last = steps - 1
def _cases():
    rng = np.random.Generator(np.random.Philox(11))
    ragged = rng.integers(1, 8, 40)
    ragged[[0, 5, 17]] = 1          # shortest and longest rows, and runs of equal lengths across tile borders
    ragged[[3, 20, 39]] = 7
    ragged[8:14] = 4
    return {
        "ragged40": (40, 7, ragged),                                   # two full tiles and a partial one
        "full16": (16, 7, np.full(16, 7)),                             # nothing skipped
        "ones16": (16, 7, np.full(16, 1)),
        "identity40": (40, 7, np.sort(ragged)[::-1].copy()),           # already longest first: the order is the identity
        "wide528": (528, 5, rng.integers(1, 6, 528)),                  # 33 tiles: four members per tile
    }


CASES = _cases()
SMALL = ["ragged40", "full16", "ones16", "identity40"]
# (case, kernel variant): one workgroup per tile (no workspace), the multi-CU kernels with 8 and with 4 members per tile
VARIANTS = [(c, v) for c in SMALL for v in ("one", "cluster")] + [("wide528", "cluster")]


def _workspace(B, backward, variant):
    if variant == "one":
        return None
    n = int(_hip.lib().pnmn_lstm_seq_workspace_bytes(B, backward))
    assert n > 0  # (the multi-CU kernels do take this batch)
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _forward(inp, tokens, wp, B, T, variant, order=None, tile_steps=None):
    hs, cs, act = _nan(B, T, 256), _nan(B, T, 256), _nan(B, T, 1024)
    ws = _workspace(B, 0, variant)
    args = (inp.data_ptr(), tokens.data_ptr() if tokens is not None else None, tokens.stride(0) if tokens is not None else 0,
            wp.data_ptr(), hs.data_ptr(), cs.data_ptr(), act.data_ptr(), B, T, 256)
    tail = (ws.data_ptr() if ws is not None else None, _stream())
    if order is None:
        _hip.check(_hip.lib().pnmn_lstm_seq_fwd(*args, *tail), "lstm_seq_fwd")
    else:
        _hip.check(_hip.lib().pnmn_lstm_seq_fwd_ordered(*args, order.data_ptr(), tile_steps.data_ptr(), *tail), "lstm_seq_fwd_ordered")
    torch.cuda.synchronize()
    return hs, cs, act


def _backward(dhs, act, cs, wt, B, T, variant, order=None, tile_steps=None):
    dg = _nan(B, T, 1024)
    ws = _workspace(B, 1, variant)
    args = (dhs.data_ptr(), act.data_ptr(), cs.data_ptr(), wt.data_ptr(), dg.data_ptr(), B, T, 256)
    tail = (ws.data_ptr() if ws is not None else None, _stream())
    if order is None:
        _hip.check(_hip.lib().pnmn_lstm_seq_bwd(*args, *tail), "lstm_seq_bwd")
    else:
        _hip.check(_hip.lib().pnmn_lstm_seq_bwd_ordered(*args, order.data_ptr(), tile_steps.data_ptr(), *tail), "lstm_seq_bwd_ordered")
    torch.cuda.synchronize()
    return dg


@functools.lru_cache(maxsize=None)
def _run(case, variant, tok):
    """Both entry points, forward and backward, on one seeded problem; computed once per (case, variant, tokens?)."""
    B, T, steps = CASES[case]
    g = torch.Generator(device=DEV).manual_seed(1000 + 2 * sorted(CASES).index(case) + int(tok))
    w_hh = (torch.rand(1024, 256, device=DEV, generator=g) - 0.5) * 0.125
    wp, wt = pack_fragments(w_hh), pack_fragments(w_hh.t())
    if tok:
        inp = torch.rand(V, 1024, device=DEV, generator=g) - 0.5
        tokens = torch.randint(0, V, (B, T), device=DEV, generator=g)
    else:
        inp, tokens = torch.rand(B, T, 1024, device=DEV, generator=g) - 0.5, None
    steps_d = torch.from_numpy(steps.astype(np.int64)).to(DEV)
    order, tile_steps = _length_order((steps_d - 1).int(), T)
    valid = torch.arange(T, device=DEV)[None, :] < steps_d[:, None]             # [B, T]: t < steps[b]
    tile_of_row = torch.empty(B, dtype=torch.long, device=DEV)
    tile_of_row[order.long()] = torch.arange(B, device=DEV) // 16
    ran = torch.arange(T, device=DEV)[None, :] < tile_steps.long()[tile_of_row][:, None]  # t < tile_steps of the row's tile
    dhs = torch.randn(B, T, 256, device=DEV, generator=g) * valid[..., None]    # zero past each row's length
    ref_f = _forward(inp, tokens, wp, B, T, variant)
    got_f = _forward(inp, tokens, wp, B, T, variant, order, tile_steps)
    ref_b = _backward(dhs, ref_f[2], ref_f[1], wt, B, T, variant)
    # (the ordered backward reads the ordered forward's act and cs: NaN wherever a tile skipped, which it must not touch)
    got_b = _backward(dhs, got_f[2], got_f[1], wt, B, T, variant, order, tile_steps)
    return dict(order=order, tile_steps=tile_steps, valid=valid, ran=ran, ref_f=ref_f, got_f=got_f, ref_b=ref_b, got_b=got_b)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("B", [1, 16, 40])
def test_length_order_against_numpy(B):
    T = 7
    rng = np.random.Generator(np.random.Philox(B))
    last = rng.integers(-1, T, B)          # -1 .. T - 1
    last[0] = -1                           # an empty row: clamped to one step
    if B > 1:
        last[-1] = T - 1
        last[B // 2] = 0
        last[1:1 + B // 4] = 3             # a run of equal lengths
    if B > 16:
        last[20] = T + 3                   # past the end: clamped to T
        last[30:36] = 5
    steps = np.clip(last + 1, 1, T)
    want = np.argsort(-steps, kind="stable")
    order, tile_steps = _length_order(torch.from_numpy(last.astype(np.int32)).to(DEV), T)
    order, tile_steps = order.cpu().numpy(), tile_steps.cpu().numpy()
    assert sorted(order.tolist()) == list(range(B))
    assert np.array_equal(order, want)
    assert np.array_equal(tile_steps, [steps[want[i:i + 16]].max() for i in range(0, B, 16)])


def test_identity_case_is_the_identity():
    r = _run("identity40", "one", False)
    assert torch.equal(r["order"].cpu(), torch.arange(40, dtype=torch.int32))


@pytest.mark.parametrize("tok", [False, True], ids=["xp", "tokens"])
@pytest.mark.parametrize("case,variant", VARIANTS)
def test_ordered_forward_equals_unordered(case, variant, tok):
    r = _run(case, variant, tok)
    valid, ran = r["valid"], r["ran"]
    assert bool((ran | ~valid).all())  # a tile runs at least as long as each of its rows
    for name, ref, got in zip(("hs", "cs", "act"), r["ref_f"], r["got_f"]):
        assert not bool(torch.isnan(ref).any()), name
        assert torch.equal(_bits(ref)[valid], _bits(got)[valid]), name
    hs = r["got_f"][0]
    assert bool((hs[~ran] == 0).all())
    assert not bool(torch.isnan(hs).any())
    if case == "full16":  # nothing skipped: the whole outputs are the unordered call's
        for ref, got in zip(r["ref_f"], r["got_f"]):
            assert torch.equal(_bits(ref), _bits(got))


@pytest.mark.parametrize("tok", [False, True], ids=["xp", "tokens"])
@pytest.mark.parametrize("case,variant", VARIANTS)
def test_ordered_backward_equals_unordered(case, variant, tok):
    r = _run(case, variant, tok)
    valid = r["valid"]
    ref, got = r["ref_b"], r["got_b"]
    assert not bool(torch.isnan(ref).any())
    assert torch.equal(_bits(ref)[valid], _bits(got)[valid])
    assert bool((got[~valid] == 0).all())  # (NaN compares unequal: every skipped element has been written)
    assert bool((ref[~valid] == 0).all())  # what the unordered kernel computes there: zeros as well


def test_masked_lstm_switch_on_equals_off(monkeypatch):
    """Two layers through ``masked_lstm`` with ``last``: masked outputs, last states, the input gradient and every parameter
    gradient bit for bit the same with rows grouped by length and without.  (The products over all B x T rows see zeros at
    other places of their padded rows, zeros either way.)"""
    from probnmn.modules import seq2seq_base as sb

    B, T = 40, 7
    steps = torch.from_numpy(CASES["ragged40"][2].astype(np.int64)).to(DEV)
    fmask = (torch.arange(T, device=DEV)[None, :] < steps[:, None]).float()
    last = (steps - 1).int()
    torch.manual_seed(21)
    lstm = torch.nn.LSTM(256, 256, 2, batch_first=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(22)
    x0 = torch.randn(B, T, 256, device=DEV, generator=g)
    w_enc, w_last = torch.randn(B, T, 256, device=DEV, generator=g), torch.randn(B, 256, device=DEV, generator=g)
    seen = []
    real = sb.length_order
    monkeypatch.setattr(sb, "length_order", lambda *a: seen.append(1) or real(*a))
    results = []
    for switch in ("1", "0"):
        monkeypatch.setenv("PNMN_LSTM_LENGTH_ORDER", switch)
        lstm.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        before = len(seen)
        enc, hlast = sb.masked_lstm(lstm, x, fmask, last=last)
        assert len(seen) - before == (1 if switch == "1" else 0)  # (the ordered path ran / did not run)
        ((enc * w_enc).sum() + (hlast * w_last).sum()).backward()
        torch.cuda.synchronize()
        results.append(dict(enc=enc.detach(), hlast=hlast.detach(), dx=x.grad, **{n: p.grad for n, p in lstm.named_parameters()}))
    on, off = results
    assert len(on) == 3 + 8
    for name in on:
        assert not bool(torch.isnan(on[name]).any()), name
        assert torch.equal(on[name], off[name]), name


def test_joint_step_switch_on_equals_off(monkeypatch):
    """One joint-training iteration at the smallest batch whose encoder passes run a launch per layer (17 row tiles: one
    more than the wavefront launches take), from the same weights and seed: the seq2seq losses and the sampled programs are
    the same with the plan's encoders ordered by length and without."""
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.trainers.joint_training import JointTrainingStep
    from probnmn.vocabulary import Vocabulary

    dev = torch.device(DEV)
    vocab = Vocabulary.clevr()
    batch = synthetic_batch(vocab, 260, seed=7)
    batch["supervision"][:] = 0
    batch["supervision"][:120] = 1
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    dbatch["supervision"] = batch["supervision"]
    torch.manual_seed(9)
    state = [m.state_dict() for m in (ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256),
                                      NeuralModuleNetwork(vocab))]
    outs = []
    for switch in ("1", "0"):
        monkeypatch.setenv("PNMN_LSTM_LENGTH_ORDER", switch)
        models = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256), NeuralModuleNetwork(vocab)]
        for m, sd in zip(models, state):
            m.load_state_dict(sd)
            m.to(dev)
        step = JointTrainingStep(*models, objective="ours", alpha=100.0, beta=0.1, gamma=1.0, delta=0.99, lr=1e-5)
        torch.manual_seed(5)
        out = step.step(dbatch)
        torch.cuda.synchronize()
        plans = [p for p in step.__dict__.get("_plans", {}).values() if p]
        assert len(plans) == 1  # (the plan ran)
        names = {name for calls in (plans[0].fwd_pg_enc, plans[0].fwd_qr, plans[0].bwd_b) for _, _, name in calls}
        assert ("pnmn_lstm_seq_fwd_ordered" in names) == (switch == "1") and ("pnmn_lstm_seq_bwd_ordered" in names) == (switch == "1")
        assert ("pnmn_lstm_seq_fwd" in names) == (switch == "0")
        keep = lambda v: torch.as_tensor(v).detach().cpu().clone()  # noqa: E731
        outs.append(dict(programs=keep(out["programs"]), pg=keep(out["loss"]["program_generation_gt"]),
                         qr=keep(out["loss"]["question_reconstruction_gt"]),
                         rec=keep(out["elbo"]["reconstruction_likelihood"]), kl=keep(out["elbo"]["kl_divergence"])))
        step.close()
    on, off = outs
    for name in on:
        assert torch.equal(on[name], off[name]), name
