"""Free-running decoder tiles that stop once all their rows have emitted @end@ (pnmn_attn_lstm_fwd_group_stop), and the
backward of such a pass with its rows grouped by the steps the forward counted (pnmn_length_order_steps,
pnmn_attn_lstm_bwd_group_ordered): against the call with ``steps_out`` null -- bit for bit up to every row's first @end@,
@end@ in the tokens and finite values behind it, every output pre-filled with NaN so that an element that must be defined and is
not shows -- a pass cut into two row ranges, the argument checks, the ordered backward against the unordered one over the same
saved tensors, and one 260-question seq2seq plan with the switch on against off.

Shapes: hidden 256 (fixed by the kernels), S = 5, V = 12, T = 8; B = 40 is two full tiles and one of 8 rows.

How the rows come to end where the tests need them: the cell's candidate gate follows the row's context, the context is the row's
encoder level ``s`` (all its source positions hold about the same vector), and the end token's logit is A mean(h_t) - M -- so a
row's hidden state climbs by its level every step and crosses the bar at a step its level picks; a negative level never does.
Which level gives which step is READ from a run of the plain call over a sweep of 512 levels (``_pool``), the 40 rows are
copies of sweep rows (a row's arithmetic does not depend on its neighbours), and every test asserts the lengths it needs on
the plain run of the rows it uses -- nothing rests on the sweep having been read right."""
import functools

import numpy as np
import pytest
import torch

from probnmn import _hip
from probnmn.modules.seq2seq_base import pack_fragments
from test_gemm_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, S, V, T = 256, 5, 12, 8
PAD, UNK, START, END = 0, 1, 2, 3
SEED = 1234
FWD_OUT = ("hs", "cs", "act", "ctx", "probs")
BWD_OUT = ("dgates", "dctx", "dscore", "weights", "dh0")
NEVER = T + 1  # (a length of the layouts below: a row without an @end@)
# lengths (steps: 1 + the step of the first @end@) of the 40 rows: a tile that has ended by step 2; a tile with rows that never
# end; the ragged tile, whose last row ends at step T - 1 exactly
LAYOUT = [1, 2, 3, 3, 2, 1, 1, 3, 2, 2, 3, 1, 3, 3, 1, 2] + [NEVER, 8, 1, 5, 2, 7, 3, 6, 4, NEVER, 1, 1, 2, 2, 3, 3] + [2, 4, 6, 8, 1, 3, 5, 7]


def _stream():
    return _hip.stream_ptr(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(11)
    r = lambda *shape, scale: torch.randn(*shape, generator=g) * scale  # noqa: E731
    w_c, w_hh, etable = r(4 * H, H, scale=0.02), r(4 * H, H, scale=0.02), r(V, 4 * H, scale=0.02)
    w_c[2 * H:3 * H] += torch.eye(H)              # the candidate gate follows the context
    etable[:, :H] += 3.0                           # input, forget and output gates open
    etable[:, H:2 * H] += 4.0
    etable[:, 3 * H:] += 3.0
    w_p, b_p = r(V, H, scale=0.05), r(V, scale=0.1)
    w_p[END] = 1000.0 / H                          # logit of @end@ = 1000 mean(h_t) - 300
    b_p[END] = -300.0
    w = dict(w_c=pack_fragments(w_c.to(DEV)), w_hh=pack_fragments(w_hh.to(DEV)), w_c_t=pack_fragments(w_c.t().contiguous().to(DEV)),
             w_hh_t=pack_fragments(w_hh.t().contiguous().to(DEV)), etable=etable.to(DEV), w_p=w_p.to(DEV), b_p=b_p.to(DEV))
    return w


def _rows(levels, seed):
    """Per-row inputs of rows whose encoder level is ``levels``."""
    B = len(levels)
    g = torch.Generator().manual_seed(seed)
    enc = torch.as_tensor(levels, dtype=torch.float32)[:, None, None] + 0.01 * torch.randn(B, S, H, generator=g)
    mask = torch.ones(B, S)
    mask[torch.arange(B) % 3 == 0, S - 2:] = 0.0
    return dict(enc=enc.to(DEV), mask=mask.to(DEV), h0=(0.05 * torch.randn(B, H, generator=g)).to(DEV))


def _workspace(B, backward):
    n = _hip.decoder_workspace_bytes([B], backward)
    assert n > 0  # (the multi-CU kernels do take this pass)
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _forward(rows, mode, stop, end=END, teacher=None):
    """One free-running pass (``mode`` 1 sampling, 2 greedy); ``stop``: through the new entry point with steps_out.  Outputs NaN /
    -7 pre-filled.  Returns (rc, outputs)."""
    B, w = rows["enc"].size(0), _weights()
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out = dict(hs=nan(B, T, H), cs=nan(B, T, H), act=nan(B, T, 4 * H), ctx=nan(B, T, H), probs=nan(B, T, S),
               tokens=torch.full((B, T), -7, dtype=torch.long, device=DEV), steps=torch.full((B,), -7, dtype=torch.int32, device=DEV))
    job = np.zeros(1, _hip.DECODER_FWD_JOB)
    j = job[0]
    for k in ("enc", "mask", "h0"):
        j[k] = rows[k].data_ptr()
    for k in ("w_c", "w_hh", "etable", "w_p", "b_p"):
        j[k] = w[k].data_ptr()
    for k in FWD_OUT + ("tokens",):
        j[k] = out[k].data_ptr()
    j["B"], j["T"], j["S"], j["V"], j["sample"] = B, T, S, V, mode
    j["pad_index"], j["unk_index"], j["start_index"], j["seed"], j["row_offset"] = PAD, UNK, START, SEED, 5
    if teacher is not None:
        j["sample"], j["in_tokens"], j["in_token_stride"] = 0, teacher.data_ptr(), teacher.stride(0)
    ws, lib = _workspace(B, False), _hip.lib()
    if stop:
        outs = np.array([out["steps"].data_ptr()], np.uint64)
        rc = lib.pnmn_attn_lstm_fwd_group_stop(job.ctypes.data, None, end, None, None, None, 0, 0, 1, H, None, None, outs.ctypes.data,
                                               ws.data_ptr(), _stream())
    else:
        rc = lib.pnmn_attn_lstm_fwd_group_stop(job.ctypes.data, None, 0, None, None, None, 0, 0, 1, H, None, None, None,
                                               ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out


def _lengths(tokens):
    """1 + the step of every row's first @end@; NEVER without one."""
    is_end = tokens == END
    first = torch.where(is_end.any(1), is_end.float().argmax(1), torch.full_like(tokens[:, 0], NEVER - 1))
    return first + 1


@functools.lru_cache(maxsize=None)
def _pool(mode):
    """512 rows of levels -0.05 .. 0.6 through the plain call: (levels, the length each realised).  The positive levels are
    spaced geometrically: a length's range of levels narrows as the length grows."""
    levels = np.concatenate([np.linspace(-0.05, 0.0, 32), np.geomspace(0.03, 0.6, 480)])
    rc, out = _forward(_rows(levels, seed=21), mode, stop=False)
    assert rc == 0
    return levels, _lengths(out["tokens"]).cpu().numpy()


def _levels_for(mode, lengths):
    """A sweep level for every wanted length: the middle one of those that realised it."""
    levels, got = _pool(mode)
    pick = {}
    for n in sorted(set(lengths)):
        hits = np.flatnonzero(got == n)
        assert len(hits) >= 3, (n, np.bincount(got))  # (the sweep reaches every length, with room either side)
        pick[n] = levels[hits[len(hits) // 2]]
    return [pick[n] for n in lengths]


@functools.lru_cache(maxsize=None)
def _case(mode):
    rows = _rows(_levels_for(mode, LAYOUT), seed=22)
    rc0, plain = _forward(rows, mode, stop=False)
    rc1, got = _forward(rows, mode, stop=True)
    assert rc0 == 0 and rc1 == 0
    return rows, plain, got, _lengths(plain["tokens"])


def _check_against_plain(plain, got, B):
    """What the issue asks of a stopped pass against the plain one; returns (steps, ran): every row's steps and its tile's."""
    length = _lengths(plain["tokens"])
    steps = length.clamp(max=T)
    assert torch.equal(got["steps"].long(), steps)
    ran = torch.stack([steps[k:k + 16].max() for k in range(0, B, 16)]).repeat_interleave(16)[:B]
    t = torch.arange(T, device=DEV)[None, :]
    own, tile = t < steps[:, None], t < ran[:, None]
    assert torch.equal(got["tokens"][own], plain["tokens"][own])
    assert bool((got["tokens"][~own] == END).all())
    for k in FWD_OUT:
        assert not bool(torch.isnan(plain[k]).any()), k
        assert torch.equal(got[k][own], plain[k][own]), k       # bit for bit up to and including the first @end@
        assert bool(torch.isfinite(got[k]).all()), k            # what a later call or a regrouped backward may read
        if bool((~tile).any()):
            assert float(got[k][~tile].abs().max()) == 0.0, k   # zeros from the tile's last step on
    return steps, ran


@pytest.mark.parametrize("mode", [1, 2])
def test_stopped_pass_against_the_plain_call(mode):
    rows, plain, got, length = _case(mode)
    # the preconditions, on the run without steps_out: a tile that has ended by step 2, a tile with a row that never ends, a
    # tile whose last row ends at step T - 1 exactly
    assert int(length[:16].max()) <= 3
    assert int(length[16:32].max()) == NEVER
    assert int(length[32:].max()) == T
    assert len(set(length.tolist())) >= 8  # (scattered)
    steps, ran = _check_against_plain(plain, got, 40)
    assert ran[0] <= 3 and ran[16] == T and ran[32] == T


@pytest.mark.parametrize("mode", [1, 2])
def test_two_row_ranges(mode):
    """B = 520 runs as two launches (512 rows + 8): the second takes steps_out + 512."""
    rng = np.random.Generator(np.random.Philox(8))
    lengths = np.concatenate([rng.integers(1, 5, 256), rng.choice(np.arange(1, NEVER + 1), 256), rng.integers(1, 4, 8)])
    rows = _rows(_levels_for(mode, lengths.tolist()), seed=23)
    rc0, plain = _forward(rows, mode, stop=False)
    rc1, got = _forward(rows, mode, stop=True)
    assert rc0 == 0 and rc1 == 0
    steps, ran = _check_against_plain(plain, got, 520)
    assert int(ran[512:].max()) < T and int(ran[:256].min()) < T and int(ran.max()) == T  # short tiles in both ranges, and a full one


def test_rejected_jobs():
    einval = _hip.CONSTANTS["PNMN_EINVAL"]
    rows = _rows([0.1] * 16, seed=24)
    teacher = torch.randint(4, V, (16, T), device=DEV)
    assert _forward(rows, 0, stop=True, teacher=teacher)[0] == einval   # a teacher-forced job with steps_out
    assert _forward(rows, 0, stop=False, teacher=teacher)[0] == 0       # (the same job without: the call as it was)
    for mode in (1, 2):
        assert _forward(rows, mode, stop=True, end=-1)[0] == einval     # end_index outside [0, V)
        assert _forward(rows, mode, stop=True, end=V)[0] == einval


def _order_of(steps):
    B = steps.numel()
    order = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tile_steps = torch.full(((B + 15) // 16,), -1, dtype=torch.int32, device=DEV)
    _hip.check(_hip.lib().pnmn_length_order_steps(steps.data_ptr(), B, T, order.data_ptr(), tile_steps.data_ptr(), _stream()), "length_order_steps")
    return order, tile_steps


def _backward(rows, fwd, dhs, lists):
    B, w = dhs.size(0), _weights()
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out = dict(dgates=nan(B, T, 4 * H), dctx=nan(B, T, H), dscore=nan(B, T, S), weights=nan(B, T, S), dh0=nan(B, H))
    job = np.zeros(1, _hip.DECODER_BWD_JOB)
    j = job[0]
    j["dhs"] = dhs.data_ptr()
    for k in ("enc", "mask", "h0"):
        j[k] = rows[k].data_ptr()
    j["w_c_t"], j["w_hh_t"] = w["w_c_t"].data_ptr(), w["w_hh_t"].data_ptr()
    for k in ("act", "cs", "hs", "probs"):
        j[k] = fwd[k].data_ptr()
    for k in BWD_OUT:
        j[k] = out[k].data_ptr()
    j["B"], j["T"], j["S"] = B, T, S
    ws, lib = _workspace(B, True), _hip.lib()
    if lists is None:
        rc = lib.pnmn_attn_lstm_bwd_group(job.ctypes.data, 1, H, ws.data_ptr(), _stream())
    else:
        arr = np.array([[lists[0].data_ptr()], [lists[1].data_ptr()]], np.uint64)
        rc = lib.pnmn_attn_lstm_bwd_group_ordered(job.ctypes.data, 1, H, arr[0].ctypes.data, arr[1].ctypes.data, ws.data_ptr(), _stream())
    _hip.check(rc, "attn_lstm_bwd_group")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", [1, 2])
def test_backward_grouped_by_the_counted_steps(mode):
    """The lists are built from steps_out; the backward then groups rows differently from the forward that saved their tensors: a
    short row of the forward's first tile (3 steps, zeros behind) sits in a backward tile of up to T steps."""
    rows, _, fwd, _ = _case(mode)
    steps = fwd["steps"]
    order, tile_steps = _order_of(steps)
    assert np.array_equal(order.cpu().numpy(), np.argsort(-steps.cpu().numpy(), kind="stable"))
    slot = torch.empty(40, dtype=torch.long, device=DEV)
    slot[order.long()] = torch.arange(40, device=DEV)
    row_ts = tile_steps.long()[slot // 16]
    fwd_ran = torch.stack([steps[k:k + 16].max() for k in range(0, 40, 16)]).repeat_interleave(16)[:40].long()
    assert bool((row_ts > fwd_ran).any())  # (the mismatch is there: a row whose backward tile outlasts its forward tile)
    valid = torch.arange(T, device=DEV)[None, :] < steps.long()[:, None]
    g = torch.Generator(device=DEV).manual_seed(4)
    dhs = torch.randn(40, T, H, device=DEV, generator=g) * valid[:, :, None]
    plain = _backward(rows, fwd, dhs, None)
    got = _backward(rows, fwd, dhs, (order, tile_steps))
    for k in BWD_OUT:
        assert not bool(torch.isnan(plain[k]).any()), k
        assert not bool(torch.isnan(got[k]).any()), k
    assert torch.equal(got["dh0"], plain["dh0"])
    for k in ("dgates", "dctx", "dscore", "weights"):
        assert torch.equal(got[k][valid], plain[k][valid]), k
    for k in ("dgates", "dctx", "dscore"):
        assert float(got[k][~valid].abs().max()) == 0.0, k
    ran = torch.arange(T, device=DEV)[None, :] < row_ts[:, None]
    assert float(got["weights"][~ran].abs().max()) == 0.0


N_NOSUP, N_SUP, TQ, TP = 258, 2, 20, 12  # 260 questions: the sampling pass is above the 256-row threshold


def _plan(monkeypatch, switch):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.runtime.seq_plan import Seq2SeqPlan
    from probnmn.vocabulary import Vocabulary

    dev = torch.device(DEV)
    vocab = Vocabulary.clevr()
    torch.manual_seed(1)
    models = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256)]
    with torch.no_grad():  # (a fresh generator rarely ends a program: make @end@ likely enough that rows end at scattered steps)
        models[0]._output_projection_layer.bias[models[0]._end_index] += 2.5
    for m in models:
        m.to(dev)
    models[2].eval()
    B = N_NOSUP + N_SUP
    batch = synthetic_batch(vocab, B, seed=4, with_image=False)
    question, program = batch["question"][:, :TQ].contiguous().to(dev), batch["program"][:, :TP].contiguous().to(dev)
    monkeypatch.setenv("PNMN_SAMPLED_PASS_STOP", switch)
    plan = Seq2SeqPlan(*models, dev, N_NOSUP, N_SUP, TQ, TP)
    names = [name for calls in (plan.fwd_pg, plan.bwd_a) for _, _, name in calls]
    assert ("pnmn_attn_lstm_fwd_group_stop" in names) == (switch == "1")
    assert ("pnmn_length_order_steps" in names) == (switch == "1")
    for name in ["pg.d." + k for k in ("hs", "cs", "cx", "act", "dg", "dctx")] + ["pg.s." + k for k in ("probs", "dscore", "weights")]:
        plan[name].fill_(float("nan"))
    torch.manual_seed(9)
    plan.run_encoder(question, program, torch.arange(N_NOSUP, device=dev), torch.arange(N_NOSUP, B, device=dev))
    plan.run_decoders()
    plan.run_generator_finish()
    plan.run_reconstructor()
    plan.run_prior()
    g = torch.Generator(device=dev).manual_seed(2)
    plan.backward(*(torch.randn(r, device=dev, generator=g) for r in (N_NOSUP, N_SUP, B)))
    torch.cuda.synchronize()
    return plan


def test_plan_with_the_switch_on_against_off(monkeypatch):
    on, off = _plan(monkeypatch, "1"), _plan(monkeypatch, "0")
    steps = on["pg.s.steps"].long()
    tiles = torch.stack([steps[k:k + 16].max() for k in range(0, N_NOSUP, 16)])
    assert int(tiles.min()) < on.D and len(set(steps.tolist())) > 3  # (tiles did stop, at scattered steps)
    assert torch.equal(on.out["z"], off.out["z"])                    # the trimmed programs
    for key in ("loss_s", "loss_t", "loss_q", "loss_p"):
        assert bool(torch.isfinite(on.out[key]).all()) and torch.equal(on.out[key], off.out[key]), key  # per-row losses: bit-equal
    K = (N_NOSUP + N_SUP) * max(on.e_pg["T"], on.e_qr["T"], on.D)  # (the bar of tests/test_seq_plan_pairs_gpu.py)
    for mm, ref in ((on.pg, off.pg), (on.qr, off.qr)):
        for got, want in zip(mm.grads, ref.grads):
            assert bool(torch.isfinite(got).all())
            if float(want.abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0
            else:
                _close(got, want.double(), K)
