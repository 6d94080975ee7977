"""What decoding under the grammar automaton costs against the unconstrained decodes of the same build.

usage: python scripts/constrained_sampling_rate.py [--questions 256] [--steps 30] [--rounds 5] [--window 0.5]
                                                   [--timeout 240] [--out profiles/ab/constrained_sampling.txt]

``ProgramGenerator.decode`` of B questions x T steps, free running: ``"sampling"`` and ``"greedy"`` unconstrained, sampling
under the filter (0.7, 10, 0.9), and the same three under the CLEVR program automaton (``"constrained_sampling"`` with the
identity filter and with (0.7, 10, 0.9), ``"constrained_greedy"``), on both decoder families -- the multi-CU kernels the
library picks by default and the one-workgroup-per-tile kernel (PNMN_DECODER_CLUSTER=0).  The model is untrained and the
questions random; a program may end early, but the kernel runs all T steps either way.  The variants alternate
inside each round; a measurement is the host clock around as many decodes as fill ``--window`` seconds (counted from a
short trial of the variant), ending in a device synchronise, after a warm-up of every variant.  The figure is the whole
``decode`` call -- the per-call token table, the trim and the loss with the kernel -- for every variant alike.

Each family is measured by a child process of its own under ``--timeout`` seconds; the first child that fails or runs
out of time ends the run (nothing more is started on the device).  The parent never touches the device.  It writes, and
prints, one JSON line per family (median ms per decode of each variant over the rounds, the spread (min, max) and the
ratio of every constrained variant to its unconstrained twin) to ``--out``, keeping whatever follows a line starting with
``## headline`` in an existing file (the step benchmark against the parent commit, added by hand)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]
FILTER = (0.7, 10, 0.9)
# variant -> (decoding strategy, filter); a constrained variant is measured against the twin named in TWINS
VARIANTS = {"sampling": ("sampling", None), "greedy": ("greedy", None), "sampling_filtered": ("sampling", FILTER),
            "constrained_sampling": ("constrained_sampling", None), "constrained_greedy": ("constrained_greedy", None),
            "constrained_sampling_filtered": ("constrained_sampling", FILTER)}
TWINS = {"constrained_sampling": "sampling", "constrained_greedy": "greedy", "constrained_sampling_filtered": "sampling_filtered"}
FAMILIES = {"multi_cu": None, "one_workgroup": "0"}  # PNMN_DECODER_CLUSTER of the child


def worker(args) -> None:
    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("constrained_sampling_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab, max_decoding_steps=args.steps).to(dev).eval()
    questions = synthetic_batch(vocab, args.questions, seed=1)["question"].to(dev)
    compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    automaton = compiler.decoding_automaton(exclude=[pg._pad_index, pg._unk_index, pg._start_index, pg._end_index])

    def timed(fn, calls: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    with torch.no_grad():
        state = pg.encode(questions)

        def variant(strategy, filt):
            kw = {} if filt is None else dict(temperature=filt[0], top_k=filt[1], top_p=filt[2])
            if strategy.startswith("constrained"):
                kw["constraint"] = automaton
            return lambda: pg.decode(state, decoding_strategy=strategy, seed=7, **kw)

        variants = tuple((name, variant(*what)) for name, what in VARIANTS.items())
        for _, fn in variants:
            for _ in range(3):
                fn()
        calls = {name: max(10, int(args.window * 1e3 / timed(fn, 10)) + 1) for name, fn in variants}
        ms = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                ms[name].append(timed(fn, calls[name]))
    med = {name: statistics.median(v) for name, v in ms.items()}
    print(json.dumps({
        "family": args.worker, "questions": args.questions, "steps": args.steps, "calls": calls,
        "ms": {name: round(med[name], 4) for name in ms},
        "spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in ms.items()},
        "over_unconstrained": {name: round(med[name] / med[twin], 3) for name, twin in TWINS.items()},
        "us_per_step": {name: round(med[name] / args.steps * 1e3, 2) for name in ms}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of decodes per measurement")
    ap.add_argument("--timeout", type=int, default=240, help="seconds each family's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "constrained_sampling.txt"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker is not None:
        return worker(args)
    lines = ["# scripts/constrained_sampling_rate.py --questions %d --steps %d --rounds %d --window %g"
             % (args.questions, args.steps, args.rounds, args.window),
             "# ms per ProgramGenerator.decode, median over the rounds; over_unconstrained = constrained variant / its unconstrained twin, same build"]
    failed = None
    for family, cluster in FAMILIES.items():
        env = dict(os.environ)
        env.pop("PNMN_DECODER_CLUSTER", None)
        if cluster is not None:
            env["PNMN_DECODER_CLUSTER"] = cluster
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", family,
               "--questions", str(args.questions), "--steps", str(args.steps), "--rounds", str(args.rounds),
               "--window", str(args.window)]
        got = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        if got.returncode != 0:
            failed = "%s: exit status %d -- nothing further was started" % (family, got.returncode)
            lines.append("# " + failed)
            break
        lines += [ln for ln in got.stdout.splitlines() if ln.startswith("{")]
    kept = []
    if os.path.exists(args.out):
        old = open(args.out).read().splitlines()
        at = [i for i, ln in enumerate(old) if ln.startswith("## headline")]
        kept = old[at[0]:] if at else []
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + kept) + "\n")
    print("\n".join(lines), flush=True)
    if failed:
        raise SystemExit(failed)


if __name__ == "__main__":
    main()
