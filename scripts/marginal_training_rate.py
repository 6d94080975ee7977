"""What training the modules on the marginal likelihood over K programs costs: (a) the gradient-mode launch of
pnmn_answer_posterior (csrc/answer_posterior.hip) against the composition it replaces, and (b) a ``ModuleTrainingStep`` with
``objective="marginal", beam_size=4`` against the default sampled step, of this tree and of a checkout of the parent commit.

usage: python scripts/marginal_training_rate.py [--groups 256] [--rows-per-group 8] [--answers 28] [--launches 20] [--rounds 5]
                                                [--questions 256] [--steps 10] [--parent scripts/_ab/old] [--skip-steps]

``kernel`` (a): ``--groups`` groups of ``--rows-per-group`` hypothesis rows of ``--answers`` answer logits, random log-weights,
one random given answer per group, ``w_a`` = 1.  ``gradient_mode`` is ONE launch: the loss (-log_evidence), the posterior and
d loss / d logits.  ``composition`` is what a caller had to queue before, all from this tree: a plain ``pnmn_answer_posterior``
launch (the posterior shares), ``pnmn_answer_loss`` on the rows with ``answers[question_rows]`` (each row's cross-entropy
gradient), and the multiply of that gradient by ``exp(log_posterior)``.  Device events around ``--launches`` back-to-back
runs of each, the two alternating, ``--rounds`` rounds after a warm-up, the median and the spread; the gradients are
compared once.

``step`` (b): ms per step at ``--questions`` questions of full-size feature maps on the full-size NMN, ``--steps`` steps per
turn after a warm-up turn, a host clock around steps that end in a device synchronise.  Each variant is a child process of
its own (``--child``), the variants alternating over ``--rounds`` rounds: ``marginal`` (this tree, a constrained beam of 4),
``sampled`` (this tree, the default step with the generator's one sample), ``annotated`` (this tree, the default step on the
batch's own annotated programs, all valid: what a step over ``--questions`` VALID rows costs -- an untrained generator's
samples are mostly invalid programs, which the NMN does not run) and ``parent_sampled`` (the same default step as ``sampled``
with the python package of ``--parent``, a checkout of the parent commit made with
    mkdir -p scripts/_ab/old && git archive <parent> probnmn-clevr_amd/probnmn include | tar -x -C scripts/_ab/old
running on this tree's library: the ABI is the same).  Without that directory the parent's step is reported as not measured.
Random weights: the kernels' time does not depend on the values; the rows per question, the share of valid programs and their
length do, so each variant also reports ``valid_programs`` and ``tokens_per_program`` of one decode.

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
    """One turn of ``steps`` steps after a warm-up turn; prints {"ms_per_step", "rows_per_question", "valid_programs",
    "tokens_per_program"}."""
    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.trainers.module_training import ModuleTrainingStep
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg, nmn = ProgramGenerator(vocab).to(dev), NeuralModuleNetwork(vocab).to(dev)
    batch = synthetic_batch(vocab, questions, seed=0)
    batch = {k: batch[k].to(dev) if k != "program" else batch[k] for k in ("question", "image", "answer", "program")}
    options = dict(objective="marginal", beam_size=4, constrained=True) if variant == "marginal" else {}
    step = ModuleTrainingStep(nmn, program_generator=None if variant == "annotated" else pg, **options)
    pad = pg._pad_index
    # what the NMN is given: the programs of one decode, how many are valid and how long they are (not timed)
    if variant == "marginal":
        programs = step._hypotheses(batch)[0].numpy()
    elif variant == "annotated":
        programs = batch["program"].numpy()
    else:
        with torch.no_grad():
            programs = pg(batch["question"], decoding_strategy="sampling")["predictions"].cpu().numpy()
    valid = [c.valid for c in nmn.engine.compiler.compile_batch(programs)]
    rows = []

    def turn() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            rows.append(step.step(batch).get("rows", questions))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    turn()
    del rows[:]
    print(json.dumps({"ms_per_step": turn(), "rows_per_question": statistics.mean(rows) / questions,
                      "valid_programs": sum(valid) / len(valid), "tokens_per_program": float((programs != pad).sum(1).mean())}),
          flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--rows-per-group", type=int, default=8)
    ap.add_argument("--answers", type=int, default=28)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed turn of a trainer")
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "_ab", "old"), help="a checkout of the parent commit")
    ap.add_argument("--skip-steps", action="store_true", help="the kernel measurement only")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", choices=("marginal", "sampled", "annotated"), help=argparse.SUPPRESS)
    ap.add_argument("--package", default=os.path.join(ROOT, "probnmn-clevr_amd"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path[:0] = [ROOT, args.package]

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("marginal_training_rate.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.questions, args.steps)

    from probnmn import _hip

    dev = torch.device("cuda:0")
    G, K, A = args.groups, args.rows_per_group, args.answers
    R = G * K
    gen = torch.Generator().manual_seed(0)
    logits = (torch.randn(R, A, generator=gen) * 3).to(dev)
    log_weight = (torch.randn(R, generator=gen) * 4 - 20).to(dev)
    answers = torch.randint(0, A, (G,), generator=gen).to(dev)
    question_rows = torch.arange(G, device=dev).repeat_interleave(K)
    valid = torch.ones(R, dtype=torch.int32, device=dev)
    group_start = (torch.arange(G + 1, dtype=torch.int32) * K).to(dev)
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    make = lambda: {"d_logits": torch.empty(R, A, **f), "row_predictions": torch.empty(R, dtype=torch.long, device=dev),  # noqa: E731
                    "log_posterior": torch.empty(R, **f), "log_evidence": torch.empty(G, **f), "best_row": torch.empty(G, **i),
                    "support": torch.empty(G, **i), "consistent_count": torch.empty(G, **i), "loss": torch.empty(R, **f)}
    one, two = make(), make()
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def posterior(out, d_logits, best_row):
        _hip.check(lib.pnmn_answer_posterior(
            logits.data_ptr(), valid.data_ptr(), log_weight.data_ptr(), answers.data_ptr(), group_start.data_ptr(), 1.0, d_logits,
            out["row_predictions"].data_ptr(), out["log_posterior"].data_ptr(), out["log_evidence"].data_ptr(), best_row,
            out["support"].data_ptr(), out["consistent_count"].data_ptr(), 0, G, R, A, A, stream), "answer_posterior")

    def gradient_mode():
        posterior(one, one["d_logits"].data_ptr(), 0)
        return one["d_logits"]

    def composition():
        posterior(two, 0, two["best_row"].data_ptr())
        row_answers = answers[question_rows]
        _hip.check(lib.pnmn_answer_loss(logits.data_ptr(), row_answers.data_ptr(), valid.data_ptr(), two["row_predictions"].data_ptr(),
                                        two["loss"].data_ptr(), two["d_logits"].data_ptr(), R, A, A, 1.0, stream), "answer_loss")
        return two["d_logits"] * two["log_posterior"].exp().unsqueeze(1)

    def events(fn, calls: int) -> float:
        """ms per call: device events around ``calls`` calls."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    agree = bool(torch.allclose(gradient_mode(), composition(), rtol=1e-4, atol=1e-6)
                 and torch.equal(one["log_evidence"], two["log_evidence"]))
    events(gradient_mode, 3), events(composition, 3)
    ms = {"gradient_mode": [], "composition": []}
    for _ in range(args.rounds):
        ms["gradient_mode"].append(events(gradient_mode, args.launches))
        ms["composition"].append(events(composition, args.launches))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "measurement": "kernel", "groups": G, "rows_per_group": K, "answers": A, "launches": args.launches, "rounds": args.rounds,
        "results_agree": agree, "us_per_call": {k: round(1e3 * v, 2) for k, v in med.items()},
        "spread_us": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
        "gradient_mode_over_composition_time": round(med["gradient_mode"] / med["composition"], 4)}), flush=True)
    if args.skip_steps:
        return

    # ---- the training steps, each variant in child processes of its own, alternating
    here = os.path.join(ROOT, "probnmn-clevr_amd")
    variants = [("marginal", "marginal", here), ("sampled", "sampled", here), ("annotated", "annotated", here)]
    parent = os.path.join(args.parent, "probnmn-clevr_amd")
    if os.path.isdir(os.path.join(parent, "probnmn")):
        variants.append(("parent_sampled", "sampled", parent))
    env = dict(os.environ, PNMN_LIB=_hip.LIB_PATH)
    took = {name: [] for name, _, _ in variants}
    rows = {name: [] for name, _, _ in variants}
    given = {}
    for _ in range(args.rounds):
        for name, variant, package in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--package", package,
                   "--questions", str(args.questions), "--steps", str(args.steps)]
            got = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            if got.returncode != 0:  # (nothing more is started on the device after a child that failed)
                raise SystemExit("%s: the child process ended with status %d" % (name, got.returncode))
            result = json.loads(got.stdout.strip().splitlines()[-1])
            took[name].append(result["ms_per_step"]), rows[name].append(result["rows_per_question"])
            given[name] = {k: round(result[k], 3) for k in ("valid_programs", "tokens_per_program")}
    med = {name: statistics.median(v) for name, v in took.items()}
    yardstick = "parent_sampled" if "parent_sampled" in med else None
    print(json.dumps({
        "measurement": "step", "questions": args.questions, "steps_per_turn": args.steps, "rounds": args.rounds,
        "ms_per_step": {name: round(v, 2) for name, v in med.items()},
        "spread_ms": {name: [round(min(v), 2), round(max(v), 2)] for name, v in took.items()},
        "rows_per_question": {name: round(statistics.mean(v), 2) for name, v in rows.items()}, "programs": given,
        "marginal_over_parent_sampled_time": round(med["marginal"] / med[yardstick], 3) if yardstick else "not measured",
        "marginal_over_sampled_time": round(med["marginal"] / med["sampled"], 3)}), flush=True)


if __name__ == "__main__":
    main()
