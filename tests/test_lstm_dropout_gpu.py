"""LSTM dropout between the encoders' layers on the MI355X: the standalone kernel against the host mask bit for bit, the
wavefront launch against the per-layer path, the eager encoder / program prior against a float64 torch reference with the
host mask injected between the layers, eval mode and p = 0 as the identity that draws no seed, the launch plan against
the eager passes with dropout on, and reproducibility from a torch seed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lstm_dropout_ref import apply, multiplier
from probnmn import _hip
from probnmn.modules.seq2seq_base import pack_fragments
from test_lstm_stack_gpu import _close, _layer, _seq_bwd, _seq_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x2545_F491_4F6C_DD1D  # a 62-bit seed


def _drop(x, p, seed, row_offset=0, out=None):
    B, T, H = x.shape
    y = torch.empty_like(x) if out is None else out
    _hip.check(_hip.lib().pnmn_lstm_dropout(x.data_ptr(), y.data_ptr(), B, T, H, p, seed, row_offset, _hip.stream_ptr(torch.device(DEV))),
               "lstm_dropout")
    return y


# ---- 1. the standalone kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("rows,T,H,row_offset", [(37, 1, 256, 0), (50, 7, 128, 1000), (3, 11, 256, 2 ** 33 + 5)])
def test_kernel_equals_host_mask(p, rows, T, H, row_offset):
    x = torch.randn(rows, T, H, device=DEV)
    y = _drop(x, p, SEED, row_offset)
    torch.cuda.synchronize()
    want = apply(x.cpu().numpy(), SEED, p, row_offset)
    assert np.array_equal(y.cpu().numpy(), want)
    z = x.clone()
    _drop(z, p, SEED, row_offset, out=z)  # in place
    assert torch.equal(z, y)


def test_kernel_refuses_bad_arguments():
    lib, st = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    x = torch.zeros(2, 3, 8, device=DEV)
    assert lib.pnmn_lstm_dropout(x.data_ptr(), x.data_ptr(), 2, 3, 8, 1.5, 1, 0, st) == _hip.EINVAL
    assert lib.pnmn_lstm_dropout(x.data_ptr(), x.data_ptr(), 2, 3, 8, -0.1, 1, 0, st) == _hip.EINVAL
    assert lib.pnmn_lstm_dropout(x.data_ptr(), x.data_ptr(), 2, 4, 6, 0.5, 1, 0, st) == _hip.ESHAPE  # H % 4
    assert lib.pnmn_lstm_dropout(x.data_ptr(), x.data_ptr(), 0, 3, 8, 0.5, 1, 0, st) == 0


# ---- 2. the wavefront launch -------------------------------------------------------------------------------------------------
def _reference(enc, B, T, seed, p, dseed, roff):
    """Per-layer path with dropout: layer 1, mask, projection, layer 2; backward masks layer 1's output gradient."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    V = 40
    table = (torch.rand(V, 1024, device=DEV, generator=g) - 0.5)
    tokens = torch.randint(0, V, (B, T), device=DEV, generator=g)
    l1, l2 = enc
    hs1, cs1, act1 = _seq_fwd(table, tokens, l1["w_hh"], B, T)
    hsd = _drop(hs1, p, dseed, roff) if p > 0 else hs1
    xp2 = (hsd.double() @ l2["w_ih"].double().t() + l2["b"].double()).float().contiguous()
    hs2, cs2, act2 = _seq_fwd(xp2, None, l2["w_hh"], B, T)
    dhs2 = torch.randn(B, T, 256, device=DEV, generator=g)
    dg2 = _seq_bwd(dhs2, act2, cs2, l2["w_hh"], B, T)
    dhs1 = (dg2.double() @ l2["w_ih"].double()).float().contiguous()
    if p > 0:
        dhs1 = _drop(dhs1, p, dseed, roff)
    dg1 = _seq_bwd(dhs1, act1, cs1, l1["w_hh"], B, T)
    return dict(table=table, tokens=tokens, hs1=hs1, hsd=hsd, cs1=cs1, act1=act1, hs2=hs2, cs2=cs2, act2=act2, dhs2=dhs2, dg2=dg2, dg1=dg1)


def _stack(encs, refs, shapes, drops_in):
    lib, st = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    n = 2 * len(encs)
    fj, bj = np.zeros(n, _hip.LSTM_STACK_JOB), np.zeros(n, _hip.LSTM_STACK_JOB)
    fd, bd = np.zeros(n, _hip.LSTM_DROPOUT_DESC), np.zeros(n, _hip.LSTM_DROPOUT_DESC)
    outs, keep = [], []
    for k, ((l1, l2), ref, (B, T), (p, dseed, roff)) in enumerate(zip(encs, refs, shapes, drops_in)):
        o = {name: torch.full((B, T, w), float("nan"), device=DEV) for name, w in (("hs1", 256), ("hsd", 256), ("cs1", 256), ("act1", 1024),
                                                                                  ("hs2", 256), ("cs2", 256), ("act2", 1024), ("dg1", 1024),
                                                                                  ("dg2", 1024))}
        packs = [pack_fragments(l1["w_hh"]), pack_fragments(l2["w_hh"]), pack_fragments(l2["w_ih"]), pack_fragments(l1["w_hh"].t()),
                 pack_fragments(l2["w_hh"].t()), pack_fragments(l2["w_ih"].t())]
        keep.append(packs)
        a, b = fj[2 * k], fj[2 * k + 1]
        a["xp"], a["tokens"], a["token_stride"], a["w_hh"] = ref["table"].data_ptr(), ref["tokens"].data_ptr(), T, packs[0].data_ptr()
        a["hs"], a["cs"], a["act"], a["B"], a["T"], a["dep"] = o["hs1"].data_ptr(), o["cs1"].data_ptr(), o["act1"].data_ptr(), B, T, -1
        b["w_hh"], b["w_ih"], b["bias"] = packs[1].data_ptr(), packs[2].data_ptr(), l2["b"].data_ptr()
        b["hs"], b["cs"], b["act"], b["B"], b["T"], b["dep"] = o["hs2"].data_ptr(), o["cs2"].data_ptr(), o["act2"].data_ptr(), B, T, 2 * k
        a, b = bj[2 * k], bj[2 * k + 1]
        a["dhs"], a["act"], a["cs"], a["w_hh"], a["dgates"] = ref["dhs2"].data_ptr(), ref["act2"].data_ptr(), ref["cs2"].data_ptr(), packs[4].data_ptr(), o["dg2"].data_ptr()
        a["B"], a["T"], a["dep"] = B, T, -1
        b["act"], b["cs"], b["w_hh"], b["w_ih"], b["dgates"] = ref["act1"].data_ptr(), ref["cs1"].data_ptr(), packs[3].data_ptr(), packs[5].data_ptr(), o["dg1"].data_ptr()
        b["B"], b["T"], b["dep"] = B, T, 2 * k
        # dropout on layer 1's job: the FIRST job forward, the BELOW job backward
        fd[2 * k]["p"], fd[2 * k]["seed"], fd[2 * k]["row_offset"], fd[2 * k]["hsd"] = p, dseed, roff, o["hsd"].data_ptr()
        bd[2 * k + 1]["p"], bd[2 * k + 1]["seed"], bd[2 * k + 1]["row_offset"] = p, dseed, roff
        outs.append(o)
    for jobs, drops, fn, backward in ((fj, fd, lib.pnmn_lstm_stack_fwd_dropout, 0), (bj, bd, lib.pnmn_lstm_stack_bwd_dropout, 1)):
        nbytes = int(lib.pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, n, backward))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        for _ in range(2):  # (twice: the counters must come back to zero)
            _hip.check(fn(jobs.ctypes.data, drops.ctypes.data, n, ws.data_ptr(), st), "lstm_stack_dropout")
        torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("shapes,drops", [
    ([(64, 9), (40, 6)], [(0.3, SEED, 7), (0.0, 0, 0)]),
    ([(128, 20)], [(0.5, SEED + 1, 0)]),
    ([(33, 1), (20, 5)], [(0.2, 11, 0), (1.0, 12, 3)]),
])
def test_stack_with_dropout_equals_separate_layers(shapes, drops):
    encs = [(_layer(10 * k + 1), _layer(10 * k + 2)) for k in range(len(shapes))]
    refs = [_reference(enc, B, T, 100 + k, *d) for k, (enc, (B, T), d) in enumerate(zip(encs, shapes, drops))]
    outs = _stack(encs, refs, shapes, drops)
    for o, ref, (p, _, _) in zip(outs, refs, drops):
        for name in ("hs1", "cs1", "act1", "dg2") + (("hsd",) if p > 0 else ()):  # FIRST / TOP jobs: bit for bit
            assert torch.equal(o[name], ref[name]), name
        if p == 0:
            assert torch.isnan(o["hsd"]).all()  # (p = 0: nothing written)
        for name in ("hs2", "cs2", "act2", "dg1"):
            assert _close(o[name], ref[name]), name


def test_stack_refuses_misplaced_descriptors():
    lib, st = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    B, T = 16, 2
    jobs = np.zeros(2, _hip.LSTM_STACK_JOB)
    jobs["B"], jobs["T"] = B, T
    jobs[0]["dep"], jobs[1]["dep"] = -1, 0
    # (real buffers of the right sizes, although every call below is refused before a launch)
    bufs = dict(xp=torch.zeros(B, T, 1024, device=DEV), w_hh=torch.zeros(1024, 256, device=DEV), w_ih=torch.zeros(1024, 256, device=DEV),
                bias=torch.zeros(1024, device=DEV), hs=torch.zeros(B, T, 256, device=DEV), cs=torch.zeros(B, T, 256, device=DEV))
    hsd = torch.zeros(B, T, 256, device=DEV)
    for f, t in bufs.items():
        jobs[f] = t.data_ptr()
    ws = torch.empty(int(lib.pnmn_lstm_stack_workspace_bytes(jobs.ctypes.data, 2, 0)), dtype=torch.uint8, device=DEV)
    d = np.zeros(2, _hip.LSTM_DROPOUT_DESC)
    d[1]["p"], d[1]["hsd"] = 0.5, hsd.data_ptr()  # forward: on the SECOND job
    assert lib.pnmn_lstm_stack_fwd_dropout(jobs.ctypes.data, d.ctypes.data, 2, ws.data_ptr(), st) == _hip.EINVAL
    d[:] = 0
    d[0]["p"] = 0.5  # forward: no hsd
    assert lib.pnmn_lstm_stack_fwd_dropout(jobs.ctypes.data, d.ctypes.data, 2, ws.data_ptr(), st) == _hip.EINVAL
    d[0]["p"], d[0]["hsd"] = 1.5, hsd.data_ptr()
    assert lib.pnmn_lstm_stack_fwd_dropout(jobs.ctypes.data, d.ctypes.data, 2, ws.data_ptr(), st) == _hip.EINVAL
    torch.cuda.synchronize()


# ---- 3. / 4. / 7. the eager encoder -----------------------------------------------------------------------------------------
def _tokens(B, W, V, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(B, W, dtype=torch.long)
    lens = torch.randint(2, W + 1, (B,), generator=g)
    lens[0] = W
    for i in range(B):
        out[i, : lens[i]] = torch.randint(4, V, (int(lens[i]),), generator=g)
    return out


def _lstm_ref(sd, prefix, x, valid, mult):
    """Two-layer LSTM in float64 with ``mult`` [B,T,H] between the layers (oracle.seq2seq_oracle.packed_lstm + the mask)."""
    from oracle.seq2seq_oracle import lstm_cell

    B, T, _ = x.shape
    inp = x
    for layer in range(2):
        w_ih, w_hh = sd[prefix + "weight_ih_l%d" % layer], sd[prefix + "weight_hh_l%d" % layer]
        b_ih, b_hh = sd[prefix + "bias_ih_l%d" % layer], sd[prefix + "bias_hh_l%d" % layer]
        h = x.new_zeros(B, w_hh.shape[1])
        c = x.new_zeros(B, w_hh.shape[1])
        outs = []
        for t in range(T):
            h, c = lstm_cell(inp[:, t], h, c, w_ih, w_hh, b_ih, b_hh)
            outs.append(h)
        inp = torch.stack(outs, 1)
        if layer == 0:
            inp = inp * mult
    return inp * valid.unsqueeze(-1).to(inp.dtype)


def _generator(p, seed=0):
    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    torch.manual_seed(seed)
    return ProgramGenerator(Vocabulary.clevr(), dropout=p)


def test_eager_encoder_matches_float64_reference_with_host_mask():
    from oracle.seq2seq_oracle import END, PAD, START, add_sentence_boundary_token_ids

    p, B, W = 0.3, 12, 17
    pg = _generator(p)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in pg.state_dict().items()}
    pg.to(DEV).train()
    pg.sample_row_offset = 5
    toks = _tokens(B, W, 90, 3)
    torch.manual_seed(21)
    dseed = int(torch.randint(0, 2 ** 62, (1,)).item())  # what encode() draws first
    torch.manual_seed(21)
    state = pg.encode(toks.to(DEV))
    g = torch.Generator().manual_seed(4)
    r_enc, r_h = torch.randn(B, W + 1, 256, generator=g, dtype=torch.float64), torch.randn(B, 256, generator=g, dtype=torch.float64)
    ((state["enc"] * r_enc.float().to(DEV)).sum() + (state["h"] * r_h.float().to(DEV)).sum()).backward()

    src, _ = add_sentence_boundary_token_ids(toks, toks != PAD, START, END)
    src = src[:, 1:]
    valid = src != PAD
    emb = F.embedding(src, sd["_source_embedder.token_embedder_tokens.weight"], padding_idx=PAD)
    mult = torch.from_numpy(multiplier(dseed, B, W + 1, 256, p, row_offset=5)).double()
    enc = _lstm_ref(sd, "_encoder._module.", emb, valid, mult)
    h = enc[torch.arange(B), valid.sum(1) - 1]
    ((enc * r_enc).sum() + (h * r_h).sum()).backward()
    torch.testing.assert_close(state["enc"].detach().cpu().double(), enc.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(state["h"].detach().cpu().double(), h.detach(), rtol=1e-4, atol=1e-5)
    names = [n for n in sd if n.startswith("_encoder.") or n.startswith("_source_embedder.")]
    assert len(names) == 9
    params = dict(pg.named_parameters())
    for name in names:
        want = sd[name].grad
        got = params[name].grad.cpu().double()
        assert float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12) < 2e-3, name
    # the mask matters: without it the reference is far off
    enc0 = _lstm_ref({k: v.detach() for k, v in sd.items()}, "_encoder._module.", emb.detach(), valid, torch.ones_like(mult))
    assert float((enc0 - enc.detach()).abs().max()) > 1e-2


def test_eval_mode_and_zero_p_are_the_identity_and_draw_nothing():
    a, b = _generator(0.3), _generator(0.0)
    b.load_state_dict(a.state_dict())
    a.to(DEV).eval()
    b.to(DEV).train()
    toks = _tokens(20, 15, 90, 5).to(DEV)
    torch.manual_seed(3)
    rng = torch.random.get_rng_state()
    with torch.no_grad():
        sa = a.encode(toks)
        assert torch.equal(torch.random.get_rng_state(), rng)
        sb = b.encode(toks)
        assert torch.equal(torch.random.get_rng_state(), rng)
    assert torch.equal(sa["enc"], sb["enc"]) and torch.equal(sa["h"], sb["h"])
    a.train()  # training mode with p > 0: one seed drawn, another result
    with torch.no_grad():
        sc = a.encode(toks)
    assert not torch.equal(torch.random.get_rng_state(), rng)
    assert not torch.equal(sc["enc"], sa["enc"])


def test_masks_differ_per_pass_and_reproduce_from_the_torch_seed():
    pg = _generator(0.3)
    pg.to(DEV).train()
    toks = _tokens(24, 15, 90, 6).to(DEV)
    with torch.no_grad():
        torch.manual_seed(9)
        first, second = pg.encode(toks)["enc"], pg.encode(toks)["enc"]
        torch.manual_seed(9)
        again = pg.encode(toks)["enc"]
    assert not torch.equal(first, second)
    assert torch.equal(first, again)


# ---- 5. the launch plan against the eager passes -----------------------------------------------------------------------------
def _models(seed, p, nmn=False):
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    ms = [ProgramGenerator(vocab, dropout=p), QuestionReconstructor(vocab, dropout=p), ProgramPrior(vocab, hidden_size=256, dropout=p)]
    if nmn:
        ms.append(NeuralModuleNetwork(vocab))
    return vocab, ms


def _grads(models):
    return {"%d.%s" % (i, n): p.grad.detach().clone() for i, m in enumerate(models) for n, p in m.named_parameters()
            if p.grad is not None}


def _compare(outs, grads):
    assert torch.equal(outs[0]["programs"], outs[1]["programs"])
    assert float(outs[0]["objective"]) == pytest.approx(float(outs[1]["objective"]), rel=2e-5, abs=1e-4)
    assert sorted(grads[0]) == sorted(grads[1])
    bad = {}
    for name in grads[0]:
        scale = float(grads[1][name].abs().max()) + 1e-12
        err = float((grads[0][name] - grads[1][name]).abs().max()) / scale
        if err > 2e-4:
            bad[name] = err
    assert not bad, bad


@pytest.mark.parametrize("n,sup,stack", [(24, 7, True), (130, 64, True), (24, 7, False)])
def test_question_coding_plan_equals_eager_with_dropout(n, sup, stack, monkeypatch):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.runtime import seq_plan
    from probnmn.trainers.joint_training import QuestionCodingStep

    monkeypatch.setattr(seq_plan, "USE_STACK", stack)
    dev = torch.device(DEV)
    vocab, a = _models(1, 0.2)
    _, b = _models(2, 0.2)
    for d, s in zip(b, a):
        d.load_state_dict(s.state_dict())
    batch = synthetic_batch(vocab, n, seed=n, with_image=False)
    batch["supervision"][:] = 0
    batch["supervision"][:sup] = 1
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    dbatch["supervision"] = batch["supervision"]
    outs, grads, steps = [], [], []
    for models, plan in ((a, True), (b, False)):
        for m in models:
            m.to(dev)
        step = QuestionCodingStep(*models, objective="ours", alpha=100.0, beta=0.1, delta=0.99, lr=0.0)
        step.use_plan = plan
        torch.manual_seed(77)
        outs.append(step.step(dbatch))
        grads.append(_grads(models[:2]))
        steps.append(step)
    plans = [p for p in steps[0].__dict__.get("_plans", {}).values()]
    assert plans and all(p is not False for p in plans)  # (the plan DID run)
    names = [nm for p in plans for calls in (p.fwd_pg_enc, p.fwd_qr, p.bwd_a, p.bwd_b) for _, _, nm in calls]
    assert any("dropout" in nm for nm in names)
    if stack:
        assert "pnmn_lstm_stack_fwd_dropout" in names
    else:
        assert "pnmn_lstm_dropout" in names and not any(nm.startswith("pnmn_lstm_stack") for nm in names)
    _compare(outs, grads)
    second = []
    for step, models in zip(steps, (a, b)):
        torch.manual_seed(78)
        second.append((step.step(dbatch), _grads(models[:2])))
    torch.cuda.synchronize()
    _compare([s[0] for s in second], [s[1] for s in second])


def test_joint_plan_equals_eager_with_dropout():
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.trainers.joint_training import JointTrainingStep

    dev = torch.device(DEV)
    vocab, a = _models(3, 0.2, nmn=True)
    _, b = _models(4, 0.2, nmn=True)
    for d, s in zip(b, a):
        d.load_state_dict(s.state_dict())
    batch = synthetic_batch(vocab, 20, seed=5)
    batch["supervision"][:] = 0
    batch["supervision"][:9] = 1
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    dbatch["supervision"] = batch["supervision"]
    outs, grads, plans = [], [], []
    for models, plan in ((a, True), (b, False)):
        for m in models:
            m.to(dev)
        step = JointTrainingStep(*models, objective="ours", alpha=100.0, beta=0.1, gamma=1.0, delta=0.99, lr=1e-5)
        step.use_plan = plan
        torch.manual_seed(5)
        outs.append(step.step(dbatch))
        torch.cuda.synchronize()
        grads.append(_grads(models[:2]))
        plans.append(step.__dict__.get("_plans", {}))
        step.close()
    assert plans[0] and all(p is not False for p in plans[0].values())
    assert float(outs[0]["loss"]["nmn"]) == pytest.approx(float(outs[1]["loss"]["nmn"]), rel=1e-5, abs=1e-5)
    _compare(outs, grads)


# ---- 6. the program prior phase -----------------------------------------------------------------------------------------------
def test_program_prior_step_with_dropout_matches_float64_reference():
    from oracle.seq2seq_oracle import END, PAD, START, add_sentence_boundary_token_ids, sequence_cross_entropy_with_logits
    from probnmn.models import ProgramPrior
    from probnmn.trainers.module_training import ProgramPriorStep
    from probnmn.vocabulary import Vocabulary

    p = 0.3
    torch.manual_seed(4)
    prior = ProgramPrior(Vocabulary.clevr(), hidden_size=256, dropout=p)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in prior.state_dict().items() if k != "_output_layer.weight"}
    prior.to(DEV)
    progs = _tokens(16, 26, 44, 13)
    step = ProgramPriorStep(prior, lr=1e-2)
    torch.manual_seed(31)
    dseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(31)
    out = step.step({"program": progs.to(DEV)})

    toks, _ = add_sentence_boundary_token_ids(progs, progs != PAD, START, END)
    valid = toks != PAD
    w = sd["_embedder.token_embedder_programs.weight"]
    B, T = toks.shape
    mult = torch.from_numpy(multiplier(dseed, B, T, 256, p)).double()
    enc = _lstm_ref(sd, "_encoder._module.", F.embedding(toks, w, padding_idx=PAD), valid, mult)
    logits = F.linear(F.linear(enc, sd["_projection_layer.weight"]), w)
    ref = sequence_cross_entropy_with_logits(logits[:, :-1], toks[:, 1:], valid[:, 1:].long()).mean()
    ref.backward()
    assert float(out["loss"].detach()) == pytest.approx(float(ref.detach()), rel=1e-4)
    for name, prm in prior.named_parameters():
        want = sd[name].grad
        assert float((prm.grad.cpu().double() - want).abs().max()) / (float(want.abs().max()) + 1e-12) < 2e-3, name
