"""What training the program generator and the modules together on the marginal likelihood costs: (a) the gradient-mode launch
of pnmn_hypothesis_posterior (csrc/hypothesis_posterior.hip) against the plain launch and against the composition it replaces,
and (b) a ``MarginalJointStep`` against ``ModuleTrainingStep(objective="marginal")`` on the same candidates, of this tree and of
a checkout of the parent commit.

usage: python scripts/joint_marginal_rate.py [--groups 256] [--rows-per-group 8] [--steps-x 28] [--vocab-x 44] [--launches 20]
                                             [--rounds 5] [--questions 256] [--steps 10] [--parent scripts/_ab/old] [--skip-steps]

``kernel`` (a): ``--groups`` groups of ``--rows-per-group`` candidate rows whose x term has the generator's shapes
(``--steps-x`` teacher-forced steps over ``--vocab-x`` program tokens, a quarter of the steps padding), a random log_q per
row, weights (1, 0, 1).  ``gradient_mode`` is ONE launch: the loss (-log_evidence), the posterior and d loss / d logits.
``plain`` is the launch without the gradient.  ``composition`` is what a caller had to queue before, all from this tree: the
plain launch (the posterior shares), ``pnmn_seq_nll_fwd`` / ``pnmn_seq_nll_bwd`` on the term with dloss = the scored tokens
(each step's cross-entropy gradient of the SUM), and the multiply of that gradient by ``exp(log_posterior)``.  Device events
around ``--launches`` back-to-back runs of each, the three alternating, ``--rounds`` rounds after a warm-up, the median and
the spread; the gradients are compared once.

``step`` (b): ms per step at ``--questions`` questions of full-size feature maps on the full-size models, ``--steps`` steps per
turn after a warm-up turn, a host clock around steps that end in a device synchronise.  Each variant is a child process of
its own (``--child``), the variants alternating over ``--rounds`` rounds: ``joint`` (this tree, ``MarginalJointStep`` with a
constrained beam of 4), ``generator_only`` (the same with ``train_modules=False``), ``modules`` (this tree,
``ModuleTrainingStep(objective="marginal")`` on the same beam) and ``parent_modules`` (the same step with the python package of
``--parent``, a checkout of the parent commit made with
    mkdir -p scripts/_ab/old && git archive <parent> probnmn-clevr_amd/probnmn include | tar -x -C scripts/_ab/old
running on this tree's library: the ABI is the same).  Without that directory the parent's step is reported as not measured.
Freshly initialised models; each variant reports the rows per question of its steps.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(variant: str, questions: int, steps: int) -> None:
    """One turn of ``steps`` steps after a warm-up turn; prints {"ms_per_step", "rows_per_question"}."""
    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg, nmn = ProgramGenerator(vocab).to(dev), NeuralModuleNetwork(vocab).to(dev)
    batch = synthetic_batch(vocab, questions, seed=0)
    batch = {k: batch[k].to(dev) for k in ("question", "image", "answer")}
    if variant == "modules":
        from probnmn.trainers.module_training import ModuleTrainingStep

        step = ModuleTrainingStep(nmn, program_generator=pg, objective="marginal", beam_size=4, constrained=True)
    else:
        from probnmn.trainers import MarginalJointStep

        step = MarginalJointStep(pg, nmn, beam_size=4, constrained=True, train_modules=variant == "joint")
    rows = []

    def turn() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            rows.append(step.step(batch)["rows"])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    turn()
    del rows[:]
    print(json.dumps({"ms_per_step": turn(), "rows_per_question": statistics.mean(rows) / questions}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--rows-per-group", type=int, default=8)
    ap.add_argument("--steps-x", type=int, default=28)
    ap.add_argument("--vocab-x", type=int, default=44)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed turn of a trainer")
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "_ab", "old"), help="a checkout of the parent commit")
    ap.add_argument("--skip-steps", action="store_true", help="the kernel measurement only")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", choices=("joint", "generator_only", "modules"), help=argparse.SUPPRESS)
    ap.add_argument("--package", default=os.path.join(ROOT, "probnmn-clevr_amd"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path[:0] = [ROOT, args.package]

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("joint_marginal_rate.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.questions, args.steps)

    from probnmn import _hip

    dev = torch.device("cuda:0")
    G, K, T, V = args.groups, args.rows_per_group, args.steps_x, args.vocab_x
    R = G * K
    gen = torch.Generator().manual_seed(0)
    logits = (torch.randn(R, T, V, generator=gen) * 3).to(dev)
    tokens = torch.randint(1, V, (R, T), generator=gen)
    tokens[torch.rand(R, T, generator=gen) < 0.25] = 0  # (0 is the padding)
    tokens = tokens.to(dev)
    log_q = (torch.randn(R, generator=gen) * 2 - 3).to(dev)
    group_start = (torch.arange(G + 1, dtype=torch.int32) * K).to(dev)
    scored = (tokens != 0).sum(1).float()
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    make = lambda: {"d": torch.empty(R, T, V, **f), "lp": torch.empty(R, **f), "log_posterior": torch.empty(R, **f),  # noqa: E731
                    "log_evidence": torch.empty(G, **f), "best_row": torch.empty(G, **i), "support": torch.empty(G, **i),
                    "loss": torch.empty(R, **f), "lse": torch.empty(R, T, **f)}
    one, two, three = make(), make(), make()
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def posterior(out, slot, best_row):
        _hip.check(lib.pnmn_hypothesis_posterior(
            logits.data_ptr(), tokens.data_ptr(), T, 0, 0, 0, log_q.data_ptr(), group_start.data_ptr(), 1.0, 0.0, 1.0, 0, 0, slot, 0,
            out["log_posterior"].data_ptr(), out["log_evidence"].data_ptr(), best_row, out["support"].data_ptr(), G, R, T, V, 1, 1,
            stream), "hypothesis_posterior")

    def gradient_mode():
        posterior(one, one["d"].data_ptr(), 0)
        return one["d"]

    def plain():
        posterior(three, three["lp"].data_ptr(), three["best_row"].data_ptr())

    def composition():
        posterior(two, two["lp"].data_ptr(), two["best_row"].data_ptr())
        _hip.check(lib.pnmn_seq_nll_fwd(logits.data_ptr(), T * V, tokens.data_ptr(), T, tokens.data_ptr(), T, 0, two["loss"].data_ptr(),
                                        two["lse"].data_ptr(), R, T, V, 1e-13, stream), "seq_nll_fwd")
        _hip.check(lib.pnmn_seq_nll_bwd(logits.data_ptr(), T * V, tokens.data_ptr(), T, tokens.data_ptr(), T, 0, two["lse"].data_ptr(),
                                        scored.data_ptr(), two["d"].data_ptr(), T * V, R, T, V, 1e-13, stream), "seq_nll_bwd")
        return two["d"] * two["log_posterior"].exp().view(R, 1, 1)

    def events(fn, calls: int) -> float:
        """ms per call: device events around ``calls`` calls."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    plain()
    agree = bool(torch.allclose(gradient_mode(), composition(), rtol=1e-4, atol=1e-6)
                 and torch.equal(one["log_evidence"], two["log_evidence"]) and torch.equal(one["log_posterior"], three["log_posterior"]))
    fns = {"gradient_mode": gradient_mode, "plain": plain, "composition": composition}
    for fn in fns.values():
        events(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(events(fn, args.launches))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "measurement": "kernel", "groups": G, "rows_per_group": K, "steps_x": T, "vocab_x": V, "launches": args.launches,
        "rounds": args.rounds, "gradient_megabytes": round(R * T * V * 4 / 1e6, 2), "results_agree": agree,
        "us_per_call": {k: round(1e3 * v, 2) for k, v in med.items()},
        "spread_us": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
        "gradient_mode_over_plain_time": round(med["gradient_mode"] / med["plain"], 4),
        "gradient_mode_over_composition_time": round(med["gradient_mode"] / med["composition"], 4)}), flush=True)
    if args.skip_steps:
        return

    # ---- the training steps, each variant in child processes of its own, alternating
    here = os.path.join(ROOT, "probnmn-clevr_amd")
    variants = [("joint", "joint", here), ("generator_only", "generator_only", here), ("modules", "modules", here)]
    parent = os.path.join(args.parent, "probnmn-clevr_amd")
    if os.path.isdir(os.path.join(parent, "probnmn")):
        variants.append(("parent_modules", "modules", parent))
    env = dict(os.environ, PNMN_LIB=_hip.LIB_PATH)
    took = {name: [] for name, _, _ in variants}
    rows = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, variant, package in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--package", package,
                   "--questions", str(args.questions), "--steps", str(args.steps)]
            got = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            if got.returncode != 0:  # (nothing more is started on the device after a child that failed)
                raise SystemExit("%s: the child process ended with status %d" % (name, got.returncode))
            result = json.loads(got.stdout.strip().splitlines()[-1])
            took[name].append(result["ms_per_step"]), rows[name].append(result["rows_per_question"])
    med = {name: statistics.median(v) for name, v in took.items()}
    print(json.dumps({
        "measurement": "step", "questions": args.questions, "steps_per_turn": args.steps, "rounds": args.rounds,
        "ms_per_step": {name: round(v, 2) for name, v in med.items()},
        "spread_ms": {name: [round(min(v), 2), round(max(v), 2)] for name, v in took.items()},
        "rows_per_question": {name: round(statistics.mean(v), 2) for name, v in rows.items()},
        "joint_over_modules_time": round(med["joint"] / med["modules"], 3),
        "joint_over_parent_modules_time": round(med["joint"] / med["parent_modules"], 3) if "parent_modules" in med else "not measured"}),
        flush=True)


if __name__ == "__main__":
    main()
