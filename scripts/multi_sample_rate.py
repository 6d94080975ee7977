"""What drawing K programs per unsupervised question costs, and what the leave-one-out baseline buys: the step time of the
question-coding and the joint-training iteration at K = 1, 2, 4, and the variance of the generator's gradient at fixed
parameters under K = 4 leave-one-out against K = 1 with the moving baseline.

usage: python scripts/multi_sample_rate.py [--qc-questions 128] [--joint-questions 256] [--steps 20] [--rounds 5]
                                           [--variance-questions 64] [--seeds 200] [--skip-cost] [--skip-variance]

``cost``: half of the batch carries program supervision; the steps of K = 1, 2, 4 (K = 1: the moving baseline, K > 1:
leave-one-out; each its own models, the same weights) alternate inside a round, ``--steps`` steps per turn after a warm-up
turn, a host clock around the turn with a device synchronisation at both ends; the median over ``--rounds`` rounds and the
spread, and the ratio to K = 1 of the same run.

``variance``: a batch of ``--variance-questions`` questions, none supervised, a question-coding step with a learning rate
of zero, so every step evaluates the estimator at the same parameters with other samples.  The gradient of the generator's
output bias is read after each step; the trace of its covariance over the seeds (unbiased, per element, summed) is the
estimator's variance.  K = 4 leave-one-out over ``--seeds`` seeds; K = 1 over four times as many with the moving baseline
held at its converged value (the mean reward over 50 warm-up steps at these parameters, set again before every step).
A gradient is a mean over its sampled rows, so its variance falls as 1 / rows: both traces are reported times their
sampled rows (64 K), which is the variance per unit of sampled rows, and as the ratio of the two.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--qc-questions", type=int, default=128)
    ap.add_argument("--joint-questions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variance-questions", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-variance", action="store_true")
    args = ap.parse_args()

    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.trainers.joint_training import JointTrainingStep, QuestionCodingStep
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("multi_sample_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()

    def models(joint: bool):
        torch.manual_seed(0)
        ms = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256)]
        if joint:
            ms.append(NeuralModuleNetwork(vocab))
        return [m.to(dev) for m in ms]

    def device_batch(questions: int, joint: bool, supervised: bool):
        b = synthetic_batch(vocab, questions, seed=1, with_image=joint)
        b["supervision"][:] = 0
        if supervised:
            b["supervision"][::2] = 1
        out = {k: v.to(dev) for k, v in b.items()}
        out["supervision"] = b["supervision"]
        return out

    def turn(step, batch, steps: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step.step(batch)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    if not args.skip_cost:
        for name, joint, questions in (("question_coding", False, args.qc_questions), ("joint_training", True, args.joint_questions)):
            batch = device_batch(questions, joint, True)
            steps = {}
            for K in (1, 2, 4):
                ms = models(joint)
                steps[K] = (JointTrainingStep(*ms, lr=1e-6, num_samples=K) if joint else QuestionCodingStep(*ms, lr=1e-6, num_samples=K))
                turn(steps[K], batch, 5)
            took = {K: [] for K in steps}
            for _ in range(args.rounds):
                for K, step in steps.items():
                    took[K].append(turn(step, batch, args.steps))
            med = {K: statistics.median(v) for K, v in took.items()}
            print(json.dumps({
                "measurement": "cost", "step": name, "questions": questions, "supervised": questions - questions // 2,
                "steps_per_turn": args.steps, "rounds": args.rounds,
                "ms_per_step": {"K=%d" % K: round(v, 3) for K, v in med.items()},
                "spread_ms": {"K=%d" % K: [round(min(v), 3), round(max(v), 3)] for K, v in took.items()},
                "over_one_sample": {"K=%d" % K: round(v / med[1], 3) for K, v in med.items()}}), flush=True)
            for step in steps.values():
                step.close()
            del steps

    if not args.skip_variance:
        Q = args.variance_questions
        batch = device_batch(Q, False, False)

        def bias_gradients(step, seeds, first_seed, before=None):
            bias = step.pg._output_projection_layer.bias
            rows = []
            for s in range(seeds):
                if before is not None:
                    before()
                torch.manual_seed(first_seed + s)
                step.step(batch)
                rows.append(bias.grad.detach().clone())
            return torch.stack(rows).double()

        ms = models(False)
        loo = QuestionCodingStep(*ms, lr=0.0, num_samples=4)
        g4 = bias_gradients(loo, args.seeds, 1000)
        loo.close()

        ms = models(False)
        one = QuestionCodingStep(*ms, lr=0.0, num_samples=1)
        rewards = []
        for s in range(50):
            torch.manual_seed(500 + s)
            rewards.append(float(one.step(batch)["elbo"]["reinforce_reward"]))
        converged = statistics.mean(rewards)

        def hold():
            one.elbo._reinforce._baseline = torch.full((), converged, dtype=torch.float32, device=dev)

        g1 = bias_gradients(one, 4 * args.seeds, 100000, before=hold)
        one.close()
        trace = {"K=4 leave_one_out": float(g4.var(0, unbiased=True).sum()), "K=1 moving": float(g1.var(0, unbiased=True).sum())}
        rows = {"K=4 leave_one_out": 4 * Q, "K=1 moving": Q}
        per_row = {k: trace[k] * rows[k] for k in trace}
        print(json.dumps({
            "measurement": "variance", "questions": Q, "parameter": "program generator output bias",
            "seeds": {"K=4 leave_one_out": args.seeds, "K=1 moving": 4 * args.seeds}, "moving_baseline_held_at": round(converged, 5),
            "sampled_rows": rows, "trace_of_variance": {k: float("%.4g" % v) for k, v in trace.items()},
            "trace_times_sampled_rows": {k: float("%.4g" % v) for k, v in per_row.items()},
            "mean_gradient_distance": float("%.4g" % float((g4.mean(0) - g1.mean(0)).norm())),
            "mean_gradient_norm": float("%.4g" % float(g1.mean(0).norm())),
            "leave_one_out_over_moving_per_row": round(per_row["K=4 leave_one_out"] / per_row["K=1 moving"], 4)}), flush=True)


if __name__ == "__main__":
    main()
