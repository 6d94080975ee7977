"""What ``ProgramPrior.sample`` costs as one persistent HIP launch (``pnmn_prior_sample``) against the step-by-step torch
loop it replaces, and what the filtered, constrained and greedy modes cost against the plain kernel.

usage: python scripts/prior_sample_rate.py [--sizes 64,1024,8192] [--length 28] [--runs 20] [--timeout 300]
                                           [--out profiles/ab/prior_sample.txt]

``sample(n, length)`` of an untrained prior (hidden size 256, the CLEVR program vocabulary) in evaluation mode: the kernel
path (plain, under the filter (0.7, 10, 0.9), under the program grammar's automaton, greedy) and the torch loop
(``_sample_loop``: the code behind ``_forced`` and the fallback shapes).  Every figure is the whole call -- the per-call token
table, the launch, the trim and the sort -- with a device synchronisation before and after each run; the variants alternate
inside each round, after a warm-up of every variant.  Reported per size: the median, the fastest and the slowest of
``--runs`` runs of each variant, the ratio of the loop to the kernel, whether the kernel's slowest run beats the loop's
fastest, and the ratio of every mode to the plain kernel.

The measurement runs in one child process under ``--timeout`` seconds; the parent never touches the device.  One JSON line
per size goes to ``--out`` and to the standard output."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]
FILTER = dict(temperature=0.7, top_k=10, top_p=0.9)


def worker(args) -> None:
    import torch

    from probnmn.models import ProgramPrior
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("prior_sample_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev).eval()
    assert prior._sample_kernel_path()
    comp = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    auto = comp.decoding_automaton(exclude=[prior._pad_index, prior._unk_index, prior._start_index, prior._end_index])

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for n in args.sizes:
        variants = (("kernel", lambda: prior.sample(n, args.length, seed=7)),
                    ("torch_loop", lambda: prior._sample_loop(n, args.length)),
                    ("kernel_filtered", lambda: prior.sample(n, args.length, seed=7, **FILTER)),
                    ("kernel_constrained", lambda: prior.sample(n, args.length, seed=7, constraint=auto)),
                    ("kernel_greedy", lambda: prior.sample(n, args.length, greedy=True)))
        for _, fn in variants:
            for _ in range(3):
                fn()
        ms = {name: [] for name, _ in variants}
        for _ in range(args.runs):
            for name, fn in variants:
                ms[name].append(timed(fn))
        med = {name: statistics.median(v) for name, v in ms.items()}
        print(json.dumps({
            "samples": n, "length": args.length, "runs": args.runs,
            "ms": {name: round(med[name], 4) for name in ms},
            "spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in ms.items()},
            "loop_over_kernel": round(med["torch_loop"] / med["kernel"], 2),
            "kernel_slowest_beats_loop_fastest": max(ms["kernel"]) < min(ms["torch_loop"]),
            "over_plain_kernel": {name: round(med[name] / med["kernel"], 3) for name in ms if name.startswith("kernel_")}}),
            flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[64, 1024, 8192])
    ap.add_argument("--length", type=int, default=28)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "prior_sample.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs: at least 20")
    if args.worker:
        return worker(args)
    lines = ["# scripts/prior_sample_rate.py --sizes %s --length %d --runs %d" % (",".join(map(str, args.sizes)), args.length, args.runs),
             "# ms per ProgramPrior.sample(n, length), median over the runs; spread_ms = (fastest, slowest)"]
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--sizes",
           ",".join(map(str, args.sizes)), "--length", str(args.length), "--runs", str(args.runs)]
    got = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines += [ln for ln in got.stdout.splitlines() if ln.startswith("{")]
    if got.returncode != 0:
        lines.append("# the child ended with exit status %d" % got.returncode)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    if got.returncode != 0:
        raise SystemExit(got.returncode)


if __name__ == "__main__":
    main()
