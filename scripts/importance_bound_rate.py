"""What the importance-weighted bound costs: (a) the gradient-mode launch of pnmn_importance_bound (csrc/importance_bound.hip)
against the plain launch and against the composition it replaces, and (b) an ``ImportanceWeightedCodingStep`` against
``QuestionCodingStep`` with the same number of samples, of this tree and of a checkout of the parent commit.

usage: python scripts/importance_bound_rate.py [--questions 256] [--samples 8] [--launches 20] [--rounds 5]
                                               [--step-questions 128] [--step-samples 4] [--steps 10]
                                               [--parent scripts/_ab/old] [--skip-steps]

``kernel`` (a): ``--questions`` questions of ``--samples`` rows with the CLEVR shapes -- the reconstructor's term 46 steps
over 100 question tokens, the prior's and the generator's 31 steps over 44 program tokens, a quarter of the steps padding --
beta = 1.  ``gradient_mode`` is ONE launch: the bound, the per-row statistics and the gradients of all three logits tensors.
``plain`` is the launch without the gradients.  ``composition`` is what a caller had to queue before, all from this tree:
a gradient-mode ``pnmn_hypothesis_posterior`` launch over the generator's logits with every row a group of its own (log q of
the row and its cross-entropy gradient), a second one over the reconstructor's and the prior's logits with that log q and the
weights (1, beta, -beta) (logsumexp of log w, the shares, the two exact gradients), the leave-one-out terms in torch (direct
sums over a [G, K, K] mask) and the multiply of the generator's gradient by signal - beta share.  Device events around
``--launches`` back-to-back runs of each, the three alternating, ``--rounds`` rounds after a warm-up, the median and the
spread; the results are compared once.

``step`` (b): ms per step at ``--step-questions`` questions, a quarter of them with program supervision, on the full-size
models, ``--steps`` steps per turn after a warm-up turn, a host clock around steps that end in a device synchronise.  Each
variant is a child process of its own (``--child``), the variants alternating over ``--rounds`` rounds: ``importance_weighted``
(this tree, ``ImportanceWeightedCodingStep(num_samples=--step-samples)``), ``question_coding`` (this tree,
``QuestionCodingStep(num_samples=--step-samples)``, leave-one-out baseline) and ``parent_question_coding`` (the same step with
the python package of ``--parent``, a checkout of the parent commit made with
    mkdir -p scripts/_ab/old && git archive <parent> probnmn-clevr_amd/probnmn include | tar -x -C scripts/_ab/old
running on this tree's library: the core ABI is the same).  Without that directory the parent's step is reported as not
measured.  Freshly initialised models.

Prints one JSON line per measurement."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(variant: str, questions: int, samples: int, steps: int) -> None:
    """One turn of ``steps`` steps after a warm-up turn; prints {"ms_per_step"}."""
    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg, qr = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev)
    batch = synthetic_batch(vocab, questions, seed=0)
    supervision = torch.zeros(questions, dtype=torch.long)
    supervision[:questions // 4] = 1
    batch = {"question": batch["question"].to(dev), "program": batch["program"].to(dev), "supervision": supervision}
    if variant == "importance_weighted":
        from probnmn.trainers import ImportanceWeightedCodingStep

        step = ImportanceWeightedCodingStep(pg, qr, prior, num_samples=samples)
    else:
        from probnmn.trainers.joint_training import QuestionCodingStep

        step = QuestionCodingStep(pg, qr, prior, num_samples=samples)

    def turn() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step.step(batch)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    turn()
    print(json.dumps({"ms_per_step": turn()}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-questions", type=int, default=128)
    ap.add_argument("--step-samples", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed turn of a trainer")
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "_ab", "old"), help="a checkout of the parent commit")
    ap.add_argument("--skip-steps", action="store_true", help="the kernel measurement only")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", choices=("importance_weighted", "question_coding"), help=argparse.SUPPRESS)
    ap.add_argument("--package", default=os.path.join(ROOT, "probnmn-clevr_amd"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path[:0] = [ROOT, args.package]

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("importance_bound_rate.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.step_questions, args.step_samples, args.steps)

    from probnmn import _hip, _hip_importance

    dev = torch.device("cuda:0")
    G, K, beta = args.questions, args.samples, 1.0
    R = G * K
    gen = torch.Generator().manual_seed(0)

    def term(T, V):
        logits = (torch.randn(R, T, V, generator=gen) * 3).to(dev)
        tokens = torch.randint(1, V, (R, T), generator=gen)
        tokens[torch.rand(R, T, generator=gen) < 0.25] = 0  # (0 is the padding)
        return logits, tokens.to(dev), T, V

    x, p, q = term(46, 100), term(31, 44), term(31, 44)
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    lib, stream = _hip_importance.lib(), _hip.stream_ptr(dev)

    def buffers():
        out = {name: torch.empty(R, **f) for name in ("log_weight", "share", "signal", "lq", "log_posterior")}
        out.update({name: torch.empty(G, **f) for name in ("bound", "ess", "log_evidence")})
        out.update(support=torch.empty(G, **i), support_rows=torch.empty(R, **i), one_posterior=torch.empty(R, **f),
                   d_x=torch.empty_like(x[0]), d_p=torch.empty_like(p[0]), d_q=torch.empty_like(q[0]))
        return out

    one, two, three = buffers(), buffers(), buffers()
    args3 = lambda t: (t[0].data_ptr(), t[1].data_ptr(), t[2], 0, t[2], t[3])  # noqa: E731

    def bound(out, grad: bool):
        _hip.check(lib.pnmn_importance_bound(
            *args3(x), *args3(p), *args3(q), beta, G, K, 0, 0, 0, out["log_weight"].data_ptr(), out["share"].data_ptr(),
            out["signal"].data_ptr(), out["bound"].data_ptr(), out["ess"].data_ptr(), out["support"].data_ptr(),
            out["d_x"].data_ptr() if grad else 0, out["d_p"].data_ptr() if grad else 0, out["d_q"].data_ptr() if grad else 0,
            stream), "importance_bound")

    def gradient_mode():
        bound(one, True)

    def plain():
        bound(three, False)

    own_group = torch.arange(R + 1, dtype=torch.int32).to(dev)
    question_group = (torch.arange(G + 1, dtype=torch.int32) * K).to(dev)
    other = (~torch.eye(K, dtype=torch.bool)).to(dev)
    log_k = math.log(K)

    def composition():
        o = two
        # log q of every row and its cross-entropy gradient: every row a group of its own, so its share is 1
        _hip.check(lib.pnmn_hypothesis_posterior(
            q[0].data_ptr(), q[1].data_ptr(), q[2], 0, 0, 0, 0, own_group.data_ptr(), 1.0, 0.0, 0.0, 0, 0, o["d_q"].data_ptr(), 0,
            o["one_posterior"].data_ptr(), o["lq"].data_ptr(), 0, o["support_rows"].data_ptr(), R, R, q[2], q[3], 1, 1, stream),
            "hypothesis_posterior (gradient mode)")
        # logsumexp of log w = lx + beta lp - beta lq, the shares and the two exact gradients
        _hip.check(lib.pnmn_hypothesis_posterior(
            x[0].data_ptr(), x[1].data_ptr(), x[2], p[0].data_ptr(), p[1].data_ptr(), p[2], o["lq"].data_ptr(),
            question_group.data_ptr(), 1.0, beta, -beta, 0, 0, o["d_x"].data_ptr(), o["d_p"].data_ptr(),
            o["log_posterior"].data_ptr(), o["log_evidence"].data_ptr(), 0, o["support"].data_ptr(), G, R, x[2], x[3], p[2], p[3],
            stream), "hypothesis_posterior (gradient mode)")
        # the leave-one-out terms, by direct sums over the other samples
        share = o["log_posterior"].exp().view(G, K)
        log_w = o["log_posterior"].view(G, K) + o["log_evidence"].view(G, 1)
        others = log_w.view(G, 1, K).expand(G, K, K)
        m = others.masked_fill(~other, -float("inf")).amax(2)
        mean = others.masked_fill(~other, 0.0).sum(2) / (K - 1)
        se = (others - m.view(G, K, 1)).exp().masked_fill(~other, 0.0).sum(2)
        baseline = m + (se + (mean - m).exp()).log() - log_k
        signal = (o["log_evidence"] - log_k).view(G, 1) - baseline
        d_q = o["d_q"] * (signal - beta * share).view(R, 1, 1)
        return signal.view(R), share.view(R), d_q

    def events(fn, calls: int) -> float:
        """ms per call: device events around ``calls`` calls."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    gradient_mode(), plain()
    signal, share, d_q = composition()
    close = lambda a, b: bool(torch.allclose(a, b, rtol=1e-4, atol=1e-4))  # noqa: E731
    agree = (close(one["signal"], signal) and close(one["share"], share) and close(one["d_q"], d_q) and close(one["d_x"], two["d_x"])
             and close(one["d_p"], two["d_p"]) and close(one["bound"], two["log_evidence"] - log_k)
             and all(torch.equal(one[k], three[k]) for k in ("log_weight", "share", "signal", "bound", "ess")))
    fns = {"gradient_mode": gradient_mode, "plain": plain, "composition": composition}
    for fn in fns.values():
        events(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(events(fn, args.launches))
    med = {k: statistics.median(v) for k, v in ms.items()}
    words = sum(t[0].numel() for t in (x, p, q))
    print(json.dumps({
        "measurement": "kernel", "questions": G, "samples": K, "launches": args.launches, "rounds": args.rounds,
        "gradient_megabytes": round(words * 4 / 1e6, 2), "results_agree": agree,
        "us_per_call": {k: round(1e3 * v, 2) for k, v in med.items()},
        "spread_us": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
        "gradient_mode_over_plain_time": round(med["gradient_mode"] / med["plain"], 4),
        "gradient_mode_over_composition_time": round(med["gradient_mode"] / med["composition"], 4)}), flush=True)
    if args.skip_steps:
        return

    # ---- the training steps, each variant in child processes of its own, alternating
    here = os.path.join(ROOT, "probnmn-clevr_amd")
    variants = [("importance_weighted", "importance_weighted", here), ("question_coding", "question_coding", here)]
    parent = os.path.join(args.parent, "probnmn-clevr_amd")
    if os.path.isdir(os.path.join(parent, "probnmn")):
        variants.append(("parent_question_coding", "question_coding", parent))
    env = dict(os.environ, PNMN_LIB=_hip.LIB_PATH)
    took = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, variant, package in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--package", package,
                   "--step-questions", str(args.step_questions), "--step-samples", str(args.step_samples), "--steps", str(args.steps)]
            got = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            if got.returncode != 0:  # (nothing more is started on the device after a child that failed)
                raise SystemExit("%s: the child process ended with status %d" % (name, got.returncode))
            took[name].append(json.loads(got.stdout.strip().splitlines()[-1])["ms_per_step"])
    med = {name: statistics.median(v) for name, v in took.items()}
    print(json.dumps({
        "measurement": "step", "questions": args.step_questions, "samples": args.step_samples, "steps_per_turn": args.steps,
        "rounds": args.rounds, "ms_per_step": {name: round(v, 2) for name, v in med.items()},
        "spread_ms": {name: [round(min(v), 2), round(max(v), 2)] for name, v in took.items()},
        "importance_weighted_over_question_coding_time": round(med["importance_weighted"] / med["question_coding"], 3),
        "question_coding_over_parent_time": round(med["question_coding"] / med["parent_question_coding"], 3)
        if "parent_question_coding" in med else "not measured"}), flush=True)


if __name__ == "__main__":
    main()
