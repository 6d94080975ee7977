"""Parity hygiene asked for by the round-5 review:
  * the joint iteration with ``objective="baseline"`` (reference probnmn/modules/elbo.py:241-250,
    configs/joint_training_baseline.yml) ON THE DEVICE against the oracle -- the fused step only had CPU tests for it;
  * the gradient-noise control of scripts/r05_grad_noise.py as an ASSERTION: per example, the device's NMN gradients are as
    close to the oracle's as the oracle's own are when its weights move by one part in 1e6 (what the wide whole-network
    tolerances of tests/test_nmn_gpu.py rest on);
  * one longer trajectory (100 module-training iterations at 32 questions; ``slow``: set PNMN_RUN_SLOW=1)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _baseline_step_errors(model_seed):
    """One joint iteration with objective="baseline" on the device and on the oracle (which replays the device's sampled
    programs) from the same weights: the scalar outputs are asserted here; returns {(model, tensor): relative error of the
    clamped gradient}."""
    from oracle.train_oracle import OracleJointTrainer
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.trainers.joint_training import JointTrainingStep
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(model_seed)
    pg, qr = ProgramGenerator(vocab), QuestionReconstructor(vocab)
    prior, nmn = ProgramPrior(vocab, hidden_size=256), NeuralModuleNetwork(vocab)
    batch = synthetic_batch(vocab, 12, seed=8)
    batch["supervision"][:] = 0
    batch["supervision"][:5] = 1
    for m in (pg, qr, prior, nmn):
        m.to(dev)
    # an untrained generator samples invalid programs, which reach no NMN parameter: fit it on the batch's programs first
    # (as bench.py does), so that the comparison covers the NMN's gradients under this objective too
    import bench

    fit = {k: v.to(dev) for k, v in batch.items()}
    valid_fraction, _ = bench.fit_program_generator(pg, vocab, fit, dev, 400, 0.9)
    assert valid_fraction > 0.5, valid_fraction
    sds = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in (pg, qr, prior, nmn)]
    sds[2].pop("_output_layer.weight")
    kw = dict(objective="baseline", alpha=100.0, beta=0.1, gamma=1.0, delta=0.99, lr=1e-4)
    step = JointTrainingStep(pg, qr, prior, nmn, **kw)
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    dbatch["supervision"] = batch["supervision"]
    out = step.step(dbatch)
    z = out["programs"].detach().cpu()
    torch.cuda.synchronize()
    ref = OracleJointTrainer(*sds, vocab.get_index_to_token_vocabulary("programs"), **kw)
    ref_out = ref.step(batch, forced_programs=z)
    assert torch.equal(ref_out["programs"], z)
    assert float(out["loss"]["nmn"]) == pytest.approx(float(ref_out["nmn_loss"]), rel=1e-4, abs=1e-4)
    for k in ("elbo", "reinforce_reward"):  # (the baseline objective reports these two: reference elbo.py:241-250)
        assert float(out["elbo"][k]) == pytest.approx(float(ref_out["elbo"][k]), rel=1e-4, abs=1e-4), k
    assert float(out["objective"]) == pytest.approx(float(ref_out["objective"]), rel=1e-4, abs=1e-3)
    assert step.elbo._reinforce._reinforce_baseline == pytest.approx(ref_out["baseline"], rel=1e-4, abs=1e-4)
    errs = {}
    for key, model in (("pg", pg), ("qr", qr), ("nmn", nmn)):
        for name, p in model.named_parameters():
            g_ref = ref_out["grads"][key][name]
            if g_ref is None or float(g_ref.abs().max()) == 0.0:
                # (the reconstruction is evaluated and discarded under this objective: no gradient reaches the reconstructor)
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (key, name)
                continue
            assert p.grad is not None, (key, name)
            got = p.grad.detach().cpu().clamp(-5, 5)
            errs[(key, name)] = float((got - g_ref).abs().max()) / (float(g_ref.abs().max()) + 1e-12)
    return errs


def test_joint_baseline_objective_matches_oracle():
    errs = _baseline_step_errors(11)
    assert len(errs) > 60, len(errs)  # (the generator's 15 tensors and the NMN modules the sampled programs use)
    # Every clamped gradient within 5e-3 of the oracle's.  The network has hard gates (ReLU, max-pool arg-max, min / max):
    # an element within fp32 round-off of a gate takes the other side on one of the two machines and moves a tensor that
    # few examples reach by a few 1e-3 (test_gradient_noise_control holds the rate of such flips to the oracle's own).  A
    # flipped gate touches a few tensors and does not repeat on other weights; an indexing or arithmetic error moves most
    # tensors on every input.  So, as smoke() does: at most three tensors beyond the bar, each within it on a second,
    # independently initialised run.
    loose = sorted(k for k, e in errs.items() if e >= 5e-3)
    assert len(loose) <= 3, [(k, errs[k]) for k in loose]
    if loose:
        errs2 = _baseline_step_errors(12)
        assert len(errs2) > 60, len(errs2)
        still = [(k, errs[k], errs2[k]) for k in loose if errs2.get(k, 0.0) >= 5e-3]
        assert not still, still


def test_gradient_noise_control():
    """Per example (batch of one, ground-truth program): relative error of every gradient tensor, device vs oracle, next to
    oracles whose weights are perturbed by 1e-6 and 1e-5.  A flipped hard gate shows as FEW tensors far off (> 1e-3), an
    arithmetic or indexing error as most tensors off on every example."""
    from oracle import nmn_oracle
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models.nmn import NeuralModuleNetwork
    from probnmn.vocabulary import Vocabulary

    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 16))
    try:
        dev = torch.device("cuda:0")
        vocab = Vocabulary.clevr()
        itos = vocab.get_index_to_token_vocabulary("programs")
        torch.manual_seed(0)
        net = NeuralModuleNetwork(vocab)
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        net.to(dev).train()

        def oracle_grads(state, b):
            params = {k: v.detach().clone().requires_grad_(True) for k, v in state.items()}
            nmn_oracle.nmn_forward(params, itos, b["image"], b["program"], b["answer"])["loss"].mean().backward()
            return {k: p.grad for k, p in params.items() if p.grad is not None}

        def errors(a, b):
            return np.array(sorted(float((a[k] - b[k]).abs().max()) / (float(b[k].abs().max()) + 1e-20)
                                   for k in b if k in a and float(b[k].abs().max()) > 0))

        def perturbed(state, seed, scale):
            g = torch.Generator().manual_seed(seed)
            return {k: v * (1.0 + scale * torch.randn(v.shape, generator=g)) for k, v in state.items()}

        n = 8
        big = synthetic_batch(vocab, n, seed=1000)
        med = {"device": [], "1e-06": [], "1e-05": []}
        flips = {"device": 0, "1e-06": 0, "1e-05": 0}
        for i in range(n):
            b = {k: v[i:i + 1] for k, v in big.items()}
            ref = oracle_grads(sd, b)
            net.zero_grad(set_to_none=True)
            net(b["image"].to(dev), b["program"].to(dev), b["answer"].to(dev))["loss"].mean().backward()
            torch.cuda.synchronize()
            got = {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}
            # the same parameters receive a gradient (the arena hands autograd a zero slice for the modules a program does not
            # use, where the reference's autograd leaves None: the optimiser tells the two apart by ParamArena.touched)
            assert set(ref) <= set(got), set(ref) - set(got)
            assert all(float(got[k].abs().max()) == 0.0 for k in set(got) - set(ref))
            for name, g in (("device", got), ("1e-06", oracle_grads(perturbed(sd, 7, 1e-6), b)), ("1e-05", oracle_grads(perturbed(sd, 7, 1e-5), b))):
                e = errors(g, ref)
                med[name].append(float(np.median(e)))
                flips[name] += int(e[-1] > 1e-3)
        m = {k: float(np.median(v)) for k, v in med.items()}
        print("median tensor error: device %.1e, weights * (1 + 1e-6 N) %.1e, * (1 + 1e-5 N) %.1e; examples with a tensor beyond 1e-3: "
              "%d / %d / %d of %d" % (m["device"], m["1e-06"], m["1e-05"], flips["device"], flips["1e-06"], flips["1e-05"], n))
        # rounding: the typical tensor is as close as under a 1e-6 weight perturbation (measured 1.4e-6 .. 2.8e-6 against 2.3e-6 .. 4.3e-6)
        assert m["device"] <= 3.0 * m["1e-06"] + 2e-6, m
        # gates: no more examples with a far-off tensor than a 1e-5 perturbation produces, and never most of them
        assert flips["device"] <= max(flips["1e-05"], flips["1e-06"] + 2) and flips["device"] <= n // 2, flips
    finally:
        torch.set_num_threads(threads)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("PNMN_RUN_SLOW") != "1", reason="100 oracle iterations at 32 questions x 3 models: set PNMN_RUN_SLOW=1")
def test_long_module_training_trajectory():
    """100 module-training iterations at 32 questions: device, oracle and two controls (see tests/test_trajectory_gpu.py for
    what "the same trajectory" can mean in fp32 and for the tolerances' form)."""
    import test_trajectory_gpu as tj
    from oracle import nmn_oracle
    from oracle.train_oracle import OracleModuleTrainer
    from probnmn.models.nmn import NeuralModuleNetwork
    from probnmn.trainers.module_training import ModuleTrainingStep
    from probnmn.vocabulary import Vocabulary

    torch.set_num_threads(min(torch.get_num_threads(), 16))
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    itos = vocab.get_index_to_token_vocabulary("programs")
    torch.manual_seed(0)
    net = NeuralModuleNetwork(vocab)
    cpu_sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.to(dev)
    lr, iters, B = 3e-4, 100, 32
    trainer = ModuleTrainingStep(net, lr=lr)
    ref = OracleModuleTrainer(cpu_sd, itos, lr=lr)
    controls = [OracleModuleTrainer(tj.perturbed(cpu_sd, s, tj.CONTROL_SCALE), itos, lr=lr) for s in (1, 2)]
    got, want, ctl = [], [], []
    for it in range(iters):
        batch = tj.learnable_batch(vocab, B, seed=5000 + it)
        got.append(float(trainer.step(tj.to_dev(batch, dev))["loss"]))
        want.append(float(ref.step(batch)["loss"]))
        ctl.append(float(controls[0].step(batch)["loss"]))
        controls[1].step(batch)
    gap, chaos = tj.rel_gap(got, want), tj.rel_gap(ctl, want)
    print("loss, every 10th iteration (device / oracle / control):")
    for it in range(0, iters, 10):
        print("  %3d  %.4f  %.4f  %.4f" % (it, got[it], want[it], ctl[it]))
    print("RMS relative gap device-oracle %.2e (worst %.2e), control-oracle %.2e (worst %.2e)" % (tj.rms(gap), gap.max(), tj.rms(chaos), chaos.max()))
    assert gap[:2].max() <= 1e-5
    assert tj.rms(gap) <= tj.CHAOS_FACTOR * tj.rms(chaos) + 1e-3
    assert np.mean(got[-10:]) < 0.5 * np.mean(got[:5]) and np.mean(want[-10:]) < 0.5 * np.mean(want[:5])
    held = tj.learnable_batch(vocab, 128, seed=99)
    net.eval()
    with torch.no_grad():
        d = tj.to_dev(held, dev)
        pred = net(d["image"], d["program"], d["answer"])["predictions"].cpu()
        preds = [nmn_oracle.nmn_forward(t.params, itos, held["image"], held["program"], held["answer"])["predictions"] for t in [ref] + controls]
    acc = [int((p == held["answer"]).sum()) for p in [pred] + preds]
    agree = float((pred == preds[0]).float().mean())
    ctl_agree = min(float((p == preds[0]).float().mean()) for p in preds[1:])
    print("held-out 128: device %d correct, oracle %d, controls %d / %d; agreement with the oracle %.3f (controls at least %.3f)"
          % (acc[0], acc[1], acc[2], acc[3], agree, ctl_agree))
    # Three runs of this test on three boxes: device 120 / 123 / 128 correct of 128 against the oracle's 128 and the controls'
    # 126-128 -- the device's OWN run-to-run spread (its weight gradients are summed with atomics; Adam amplifies the last
    # bit over 100 iterations) is as wide as the distance to the oracle.  scripts/r06_long_traj_diag.py shows what is NOT behind
    # it: the oracle's forward pass on the device's final weights gives the device's predictions on all 128 examples (loss
    # within 9e-7), and every module's Adam step count equals the reference's (first appearance .. end).
    spread = max(abs(acc[1] - acc[2]), abs(acc[1] - acc[3]), abs(acc[2] - acc[3]))
    assert abs(acc[0] - acc[1]) <= spread + 10
    assert agree >= ctl_agree - 0.10 and agree >= 0.88


def test_touched_parameters_are_the_ones_the_reference_gives_a_gradient():
    """the parameters counted as "received a gradient" (torch.optim.Adam starts a parameter's state at its first
    gradient) must be the ones autograd reaches in the reference's interpreter -- not every token of a valid program: a chain
    saved by ``scene`` and never read by a binary module is executed but not part of the loss graph (its modules keep
    ``grad = None``), an invalid program's modules get none, the classifier conv always gets one."""
    from oracle import nmn_oracle
    from probnmn.models.nmn import NeuralModuleNetwork
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    itos = vocab.get_index_to_token_vocabulary("programs")
    stoi = vocab.get_token_to_index_vocabulary("programs")
    torch.manual_seed(0)
    net = NeuralModuleNetwork(vocab)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.to(dev)
    engine = net.engine
    arena = engine.ensure_arena()

    def row(*tokens):
        r = [stoi[t] for t in tokens]
        return r + [0] * (12 - len(r))

    programs = torch.tensor([
        row("query_color", "filter_shape[cube]", "scene", "filter_color[red]", "scene"),     # filter_color[red]: dead chain
        row("count", "filter_size[large]", "scene"),                                           # plain chain
        row("filter_material[metal]", "scene"),                                                # invalid: ends on an attention
        row("equal_color", "query_color", "filter_shape[sphere]", "scene", "query_color", "filter_color[blue]", "scene"),
    ])
    g = torch.Generator().manual_seed(1)
    image = torch.randn(4, 1024, 14, 14, generator=g).relu_()
    answers = torch.tensor([1, 2, 3, 4])
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out = nmn_oracle.nmn_forward(params, itos, image, programs, answers)
    out["loss"].mean().backward()
    want = {k for k, p in params.items() if p.grad is not None and k in arena.offsets}
    compiled = engine.compiler.compile_batch(programs.numpy())
    valid = np.array([c.valid for c in compiled])
    assert valid.tolist() == [True, True, False, True]
    mask = engine._touched_by(programs.numpy(), valid)
    got = {n for n, m in zip(arena.names, mask) if m}
    assert got == want, (sorted(got - want), sorted(want - got))
    # the shipped path: the library's planner reports the reachable tokens of the batch it compiled
    net.train()
    out = net(image.to(dev), programs.to(dev), answers.to(dev))
    out["loss"].mean().backward()
    shipped = {n for n, m in zip(arena.names, engine.last_touched) if m}
    assert shipped == want, (sorted(shipped - want), sorted(want - shipped))
    assert not any(n.startswith("filter_color[red].") for n in got) and not any(n.startswith("filter_material[metal].") for n in got)
    # every program invalid: the classifier conv's gradient is still a tensor (zeros), nothing else is reached
    none_valid = engine._touched_by(programs.numpy()[2:3], np.array([False]))
    assert {n for n, m in zip(arena.names, none_valid) if m} == {n for n in arena.names if n.startswith("classifier.")}
