"""What LSTM dropout between the encoders' layers costs a training step: the question-coding step at 512 questions and the
joint step at 128 and 1024, with PROGRAM_GENERATOR / QUESTION_RECONSTRUCTOR dropout 0.0 against 0.2 from the same seeds.

usage: python scripts/dropout_cost.py [--rounds R] [--steps K] [--warmup W] [--timeout S]
    Alternates the two settings (0.0, 0.2, 0.0, 0.2, ...) per workload, each measurement a fresh child process under its
    own time limit; stops at the first child that fails.  Prints one JSON line per measurement and a summary per
    workload (median ms per step of each setting, the spread of the rounds, the added fraction).
python scripts/dropout_cost.py --child MODE BATCH P [--steps K] [--warmup W]
    One measurement: MODE is qc or joint; prints {"mode", "batch", "p", "ms": [ms per step of each of 3 repeats]}."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = [("qc", 512), ("joint", 128), ("joint", 1024)]


def child(mode: str, n: int, p: float, steps: int, warmup: int) -> None:
    sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]
    import torch

    import bench
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.trainers.joint_training import JointTrainingStep, QuestionCodingStep
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    nmn = NeuralModuleNetwork(vocab).to(dev) if mode == "joint" else None
    pg, qr = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev)
    batch = bench.device_batch(vocab, n, 1000, dev)
    bench.fit_program_generator(pg, vocab, batch, dev, 300, 0.95)  # (at p = 0 in both settings: the same programs)
    for m in (pg, qr):
        m._encoder._module.dropout = p
    if mode == "joint":
        step = JointTrainingStep(pg, qr, prior, nmn, **bench.JOINT)
    else:
        step = QuestionCodingStep(pg, qr, prior, objective="ours", alpha=100.0, beta=0.1, delta=0.99, lr=1e-3)
    torch.manual_seed(1)
    for _ in range(warmup):
        step.step(batch)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step.step(batch)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / steps * 1e3, 3))
    plans = step.__dict__.get("_plans", {})
    planned = bool(plans) and all(v is not False for v in plans.values())
    if hasattr(step, "close"):
        step.close()
    print(json.dumps({"mode": mode, "batch": n, "p": p, "ms": ms, "planned": planned}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("MODE", "BATCH", "P"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=150)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), float(args.child[2]), args.steps, args.warmup)
        return 0
    results = {}
    for mode, n in WORKLOADS:
        for _ in range(args.rounds):
            for p in (0.0, 0.2):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(n), str(p), "--steps", str(args.steps),
                       "--warmup", str(args.warmup)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                except subprocess.TimeoutExpired:
                    print("%s %d p=%.1f: over %d s -- stopping" % (mode, n, p, args.timeout), flush=True)
                    return 124
                if r.returncode != 0:
                    print("%s %d p=%.1f: exit %d -- stopping\n%s" % (mode, n, p, r.returncode, r.stderr[-3000:]), flush=True)
                    return r.returncode if r.returncode > 0 else 128 - r.returncode
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                results.setdefault((mode, n, p), []).append(min(json.loads(line)["ms"]))
    for mode, n in WORKLOADS:
        off, on = results[(mode, n, 0.0)], results[(mode, n, 0.2)]
        m0, m1 = statistics.median(off), statistics.median(on)
        print(json.dumps({"workload": "%s %d" % (mode, n), "p0_ms": m0, "p0_range": [min(off), max(off)], "p02_ms": m1,
                          "p02_range": [min(on), max(on)], "added": round(m1 / m0 - 1.0, 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
