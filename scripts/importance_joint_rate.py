"""What the joint importance-weighted bound costs: (a) the gradient-mode launch of pnmn_importance_bound_joint
(csrc/importance_bound.hip) against its plain launch and against the composition it replaces, (b) an
``ImportanceWeightedJointStep`` against ``JointTrainingStep`` with the same number of samples under the grammar, and (c)
``JointTrainingStep`` and ``ImportanceWeightedCodingStep`` of this tree against a checkout of the parent commit.

usage: python scripts/importance_joint_rate.py [--questions 256] [--samples 8] [--answers 28] [--launches 20] [--rounds 5]
                                               [--step-questions 256] [--step-samples 4] [--steps 10]
                                               [--parent scripts/_ab/old] [--skip-steps]

``kernel`` (a): ``--questions`` questions of ``--samples`` rows with the CLEVR shapes -- the reconstructor's term 46 steps
over 100 question tokens, the prior's and the generator's 31 steps over 44 program tokens, a quarter of the steps padding,
``--answers`` answers -- beta = gamma = 1.  ``gradient_mode`` is ONE launch: the bound, the per-row statistics and the
gradients of all four logits tensors.  ``plain`` is the launch without the gradients.  ``composition`` is what a caller had
to queue before, all from this tree (``pnmn_importance_bound`` cannot take the answer term): a gradient-mode
``pnmn_hypothesis_posterior`` launch over the generator's logits with every row a group of its own (log q of the row and its
cross-entropy gradient), ``pnmn_answer_loss`` over the answer logits (log p(a | z) of the row and its cross-entropy gradient),
a second ``pnmn_hypothesis_posterior`` launch over the reconstructor's and the prior's logits with log q - (gamma / beta) log
p(a | z) as the row's weight term (logsumexp of log w, the shares, the two exact gradients), the leave-one-out terms in torch
(direct sums over a [G, K, K] mask) and the multiplies of the generator's gradient by signal - beta share and of the answer's
by gamma share.  Device events around ``--launches`` back-to-back runs of each, the three alternating, ``--rounds`` rounds
after a warm-up, the median and the spread; the results are compared once.

``step`` (b, c): ms per step at ``--step-questions`` questions, a quarter of them with program supervision, on the full-size
models, ``--steps`` steps per turn after a warm-up turn, a host clock around steps that end in a device synchronise.  Each
variant is a child process of its own (``--child``), the variants alternating over ``--rounds`` rounds:
``importance_joint`` (``ImportanceWeightedJointStep(num_samples=--step-samples, constraint=the grammar)``), ``joint_training``
(``JointTrainingStep(num_samples=--step-samples, constraint=the grammar)``), ``importance_coding``
(``ImportanceWeightedCodingStep(num_samples=--step-samples)``), and the latter two again as ``parent_*`` with the python
package AND the library of ``--parent``, a checkout of the parent commit made and built with
    mkdir -p scripts/_ab/old && git archive <parent> probnmn-clevr_amd/probnmn probnmn-clevr_amd/csrc include | tar -x -C scripts/_ab/old
    make -C scripts/_ab/old/probnmn-clevr_amd/csrc
(this change recompiles ``pnmn_importance_bound`` as well -- its kernel became a template -- so the parent's steps must run
the parent's own library).  Without that directory, or without its library, the parent's steps are reported as not measured.
Freshly initialised models.

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
VARIANTS = ("importance_joint", "joint_training", "importance_coding")


def child(variant: str, questions: int, samples: int, steps: int) -> None:
    """One turn of ``steps`` steps after a warm-up turn; prints {"ms_per_step"}."""
    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg, qr = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev)
    joint = variant != "importance_coding"
    batch = synthetic_batch(vocab, questions, seed=0, with_image=joint)
    supervision = torch.zeros(questions, dtype=torch.long)
    supervision[:questions // 4] = 1
    batch = {k: v.to(dev) for k, v in batch.items()}
    batch["supervision"] = supervision
    if joint:
        nmn = NeuralModuleNetwork(vocab).to(dev)
        compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
        exclude = [getattr(pg, n) for n in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
        grammar = compiler.decoding_automaton(exclude=exclude)
    if variant == "importance_joint":
        from probnmn.trainers import ImportanceWeightedJointStep

        step = ImportanceWeightedJointStep(pg, qr, prior, nmn, num_samples=samples, constraint=grammar)
    elif variant == "joint_training":
        from probnmn.trainers.joint_training import JointTrainingStep

        step = JointTrainingStep(pg, qr, prior, nmn, num_samples=samples, constraint=grammar)
    else:
        from probnmn.trainers import ImportanceWeightedCodingStep

        step = ImportanceWeightedCodingStep(pg, qr, prior, num_samples=samples)

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
    ap.add_argument("--answers", type=int, default=28)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-questions", type=int, default=256)
    ap.add_argument("--step-samples", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed turn of a trainer")
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "_ab", "old"), help="a checkout of the parent commit")
    ap.add_argument("--skip-steps", action="store_true", help="the kernel measurement only")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", choices=VARIANTS, help=argparse.SUPPRESS)
    ap.add_argument("--package", default=os.path.join(ROOT, "probnmn-clevr_amd"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path[:0] = [ROOT, args.package]

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("importance_joint_rate.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.step_questions, args.step_samples, args.steps)

    from probnmn import _hip, _hip_importance_joint

    dev = torch.device("cuda:0")
    G, K, A, beta, gamma = args.questions, args.samples, args.answers, 1.0, 1.0
    R = G * K
    gen = torch.Generator().manual_seed(0)

    def term(T, V):
        logits = (torch.randn(R, T, V, generator=gen) * 3).to(dev)
        tokens = torch.randint(1, V, (R, T), generator=gen)
        tokens[torch.rand(R, T, generator=gen) < 0.25] = 0  # (0 is the padding)
        return logits, tokens.to(dev), T, V

    x, p, q = term(46, 100), term(31, 44), term(31, 44)
    a_logits = (torch.randn(R, A, generator=gen) * 3).to(dev)
    answers = torch.randint(0, A, (G,), generator=gen).to(dev)
    row_answers = answers.repeat_interleave(K).contiguous()
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    lib, stream = _hip_importance_joint.lib(), _hip.stream_ptr(dev)

    def buffers():
        out = {name: torch.empty(R, **f) for name in ("log_weight", "share", "signal", "lq", "log_posterior", "log_pa", "answer_loss")}
        out.update({name: torch.empty(G, **f) for name in ("bound", "ess", "log_evidence")})
        out.update(support=torch.empty(G, **i), support_rows=torch.empty(R, **i), one_posterior=torch.empty(R, **f),
                   predictions=torch.empty(R, dtype=torch.long, device=dev), d_x=torch.empty_like(x[0]),
                   d_p=torch.empty_like(p[0]), d_q=torch.empty_like(q[0]), d_a=torch.empty_like(a_logits))
        return out

    one, two, three = buffers(), buffers(), buffers()
    args3 = lambda t: (t[0].data_ptr(), t[1].data_ptr(), t[2], 0, t[2], t[3])  # noqa: E731

    def bound(out, grad: bool):
        g = lambda name: out[name].data_ptr() if grad else 0  # noqa: E731
        _hip.check(lib.pnmn_importance_bound_joint(
            *args3(x), *args3(p), *args3(q), beta, G, K, 0, 0, 0, out["log_weight"].data_ptr(), out["share"].data_ptr(),
            out["signal"].data_ptr(), out["bound"].data_ptr(), out["ess"].data_ptr(), out["support"].data_ptr(), g("d_x"), g("d_p"),
            g("d_q"), a_logits.data_ptr(), 0, answers.data_ptr(), A, gamma, -math.log(A), 0, out["log_pa"].data_ptr(),
            out["predictions"].data_ptr(), g("d_a"), stream), "importance_bound_joint")

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
        # -log p(a | z) of every row and its cross-entropy gradient
        _hip.check(lib.pnmn_answer_loss(a_logits.data_ptr(), row_answers.data_ptr(), 0, o["predictions"].data_ptr(),
                                        o["answer_loss"].data_ptr(), o["d_a"].data_ptr(), R, A, 0, 1.0, stream), "answer_loss")
        # logsumexp of log w = lx + beta lp - beta (lq - (gamma / beta) la), the shares and the two exact gradients
        weight_term = o["lq"] + (gamma / beta) * o["answer_loss"]
        _hip.check(lib.pnmn_hypothesis_posterior(
            x[0].data_ptr(), x[1].data_ptr(), x[2], p[0].data_ptr(), p[1].data_ptr(), p[2], weight_term.data_ptr(),
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
        d_a = o["d_a"] * (gamma * share).view(R, 1)
        return signal.view(R), share.view(R), d_q, d_a

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
    signal, share, d_q, d_a = composition()
    close = lambda a, b: bool(torch.allclose(a, b, rtol=1e-4, atol=1e-4))  # noqa: E731
    agree = (close(one["signal"], signal) and close(one["share"], share) and close(one["d_q"], d_q) and close(one["d_a"], d_a)
             and close(one["d_x"], two["d_x"]) and close(one["d_p"], two["d_p"]) and close(one["log_pa"], -two["answer_loss"])
             and close(one["bound"], two["log_evidence"] - log_k)
             and all(torch.equal(one[k], three[k]) for k in ("log_weight", "share", "signal", "bound", "ess", "log_pa")))
    fns = {"gradient_mode": gradient_mode, "plain": plain, "composition": composition}
    for fn in fns.values():
        events(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(events(fn, args.launches))
    med = {k: statistics.median(v) for k, v in ms.items()}
    words = sum(t[0].numel() for t in (x, p, q)) + a_logits.numel()
    print(json.dumps({
        "measurement": "kernel", "questions": G, "samples": K, "answers": A, "launches": args.launches, "rounds": args.rounds,
        "gradient_megabytes": round(words * 4 / 1e6, 2), "results_agree": agree,
        "us_per_call": {k: round(1e3 * v, 2) for k, v in med.items()},
        "spread_us": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
        "gradient_mode_over_plain_time": round(med["gradient_mode"] / med["plain"], 4),
        "gradient_mode_over_composition_time": round(med["gradient_mode"] / med["composition"], 4)}), flush=True)
    if args.skip_steps:
        return

    # ---- the training steps, each variant in child processes of its own, alternating
    here = os.path.join(ROOT, "probnmn-clevr_amd")
    variants = [(name, name, here) for name in VARIANTS]
    parent = os.path.join(args.parent, "probnmn-clevr_amd")
    parent_lib = os.path.join(parent, "lib", os.path.basename(_hip.LIB_PATH))
    if os.path.isdir(os.path.join(parent, "probnmn")) and os.path.isfile(parent_lib):
        variants += [("parent_" + name, name, parent) for name in VARIANTS[1:]]
    took = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, variant, package in variants:
            env = dict(os.environ, PNMN_LIB=parent_lib if package == parent else _hip.LIB_PATH)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--package", package,
                   "--step-questions", str(args.step_questions), "--step-samples", str(args.step_samples), "--steps", str(args.steps)]
            got = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            if got.returncode != 0:  # (nothing more is started on the device after a child that failed)
                raise SystemExit("%s: the child process ended with status %d" % (name, got.returncode))
            took[name].append(json.loads(got.stdout.strip().splitlines()[-1])["ms_per_step"])
    med = {name: statistics.median(v) for name, v in took.items()}
    over = lambda a, b: round(med[a] / med[b], 3) if a in med and b in med else "not measured"  # noqa: E731
    print(json.dumps({
        "measurement": "step", "questions": args.step_questions, "samples": args.step_samples, "steps_per_turn": args.steps,
        "rounds": args.rounds, "ms_per_step": {name: round(v, 2) for name, v in med.items()},
        "spread_ms": {name: [round(min(v), 2), round(max(v), 2)] for name, v in took.items()},
        "importance_joint_over_joint_training_time": over("importance_joint", "joint_training"),
        "joint_training_over_parent_time": over("joint_training", "parent_joint_training"),
        "importance_coding_over_parent_time": over("importance_coding", "parent_importance_coding")}), flush=True)


if __name__ == "__main__":
    main()
