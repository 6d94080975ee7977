"""The seq2seq plan's weight gradients over the valid (row, step) pairs only (PNMN_GEMM_VALID_PAIRS, seq_plan.py) against the
same plan with every product whole: one forward and backward from the same weights, inputs and seed.  Every parameter
gradient agrees within test_gemm_gpu's ``_close`` at K = rows x T of the largest pass, and -- the premise the lists rest on,
asserted on the plan's own buffers -- every row of a dy operand that a list drops is exactly zero."""
import pytest
import torch

from test_gemm_gpu import _close

pytestmark = pytest.mark.gpu
N_NOSUP, N_SUP, TQ, TP = 272, 264, 20, 12  # (each pass just above the 256-row threshold)


def _run(monkeypatch, switch, state=None):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.runtime.seq_plan import Seq2SeqPlan
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(1)
    models = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256)]
    for m in models:
        m.to(dev)
    models[2].eval()
    B = N_NOSUP + N_SUP
    batch = synthetic_batch(vocab, B, seed=4, with_image=False)
    question, program = batch["question"][:, :TQ].contiguous().to(dev), batch["program"][:, :TP].contiguous().to(dev)
    monkeypatch.setenv("PNMN_GEMM_VALID_PAIRS", switch)
    plan = Seq2SeqPlan(*models, dev, N_NOSUP, N_SUP, TQ, TP)
    rows_entry = [name for calls in (plan.bwd_a, plan.bwd_b) for _, _, name in calls if name in ("pnmn_gemm_rows", "pnmn_valid_rows")]
    assert bool(rows_entry) == (switch == "1")
    torch.manual_seed(9)
    plan.run_encoder(question, program, torch.arange(N_NOSUP, device=dev), torch.arange(N_NOSUP, B, device=dev))
    plan.run_decoders()
    plan.run_generator_finish()
    plan.run_reconstructor()
    plan.run_prior()
    g = torch.Generator(device=dev).manual_seed(2)
    plan.backward(*(torch.randn(r, device=dev, generator=g) for r in (N_NOSUP, N_SUP, B)))
    torch.cuda.synchronize()
    return plan, models


def _steps_of_mask(tokens, T, pad):
    """1 + the last step whose token is not padding (0: none)."""
    w = tokens[:, :T] != pad
    return (w * torch.arange(1, T + 1, device=tokens.device)[None, :]).amax(1)


def test_plan_gradients_over_valid_pairs(monkeypatch):
    plan, models = _run(monkeypatch, "1")
    whole, _ = _run(monkeypatch, "0")
    assert torch.equal(plan.out["z"], whole.out["z"])
    K = (N_NOSUP + N_SUP) * max(plan.e_pg["T"], plan.e_qr["T"], plan.D)
    for mm, ref in ((plan.pg, whole.pg), (plan.qr, whole.qr)):
        for p, got, want in zip(mm.params, mm.grads, ref.grads):
            assert bool(torch.isfinite(got).all())
            if float(want.abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0
            else:
                _close(got, want.double(), K)
    # the premise: what a list drops is zero.  Encoders: steps = clamp(last + 1, 1, T)
    checked = 0
    for e in (plan.e_pg, plan.e_qr):
        T = e["T"]
        steps = (e["last"] + 1).clamp(1, T)
        dropped = torch.arange(T, device=steps.device)[None, :] >= steps[:, None]
        assert bool(dropped.any())
        for name in ("dg1", "dg2"):
            assert float(e[name][dropped].abs().max()) == 0.0, (e["tag"], name)
            checked += 1
    # decoders: steps = 1 + the last weighted step of the pass's loss; the flat buffers hold a model's passes one behind the other
    pad = models[0]._pad_index
    passes = {"pg": [(plan.out["z"], N_NOSUP, plan.D), (plan["pg.tgt"][:, 1:], N_SUP, TP + 1)],
              "qr": [(plan["qr.tgt"][:, 1:], N_NOSUP + N_SUP, TQ + 1)]}
    for tag, ps in passes.items():
        row0 = 0
        for tokens, rows, T in ps:
            steps = _steps_of_mask(tokens, T, pad)
            dropped = (torch.arange(T, device=steps.device)[None, :] >= steps[:, None]).reshape(-1)
            assert bool(dropped.any())
            for name in (tag + ".d.dg", tag + ".dlogits"):
                assert float(plan[name][row0:row0 + rows * T][dropped].abs().max()) == 0.0, (tag, name)
                checked += 1
            row0 += rows * T
        assert row0 == plan[tag + ".d.dg"].size(0)
    assert checked == 10
