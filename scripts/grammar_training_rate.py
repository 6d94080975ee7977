"""What training the generator under the program grammar costs, and what it buys: (a) the two launches of
csrc/grammar_logits.hip against the torch composition they replace, and (b) the question-coding and the joint-training
iteration with the grammar against the same eager passes without it and against the default planned step, with the share of
valid samples and the rows the NMN runs in both modes.

usage: python scripts/grammar_training_rate.py [--rows 1024] [--steps-t 27] [--launches 20] [--rounds 5] [--qc-questions 128]
                                               [--joint-questions 256] [--steps 10] [--skip-kernel] [--skip-steps]

``kernel`` (a): ``--rows`` x ``--steps-t`` x 44 random logits, rows the constrained reference walk emits under the CLEVR
automaton (horizon = ``--steps-t``).  ``launch_*`` is ONE launch of the C entry point forward (masked logits, log_mass,
outside) and one backward, into buffers allocated once; ``node_*`` the same through ``grammar_logits`` and
``autograd.grad``.  ``torch_*`` is what a caller could queue instead, given the sets as a mask already on the device (building
that mask step by step on the host is not timed): ``where(mask, logits, -inf)``, the two ``logsumexp`` and their difference
forward, ``where(mask, d, 0)`` backward.  Device events around ``--launches`` back-to-back runs of each, alternating,
``--rounds`` rounds after a warm-up; the median and the spread.  The results are compared once.

``step`` (b): fresh models, half of the batch supervised, one process.  Three steps per trainer, each with its own models
from the same seed, alternating inside a round: ``grammar`` (``constraint=`` the compiler's automaton: eager passes, sampled
and scored under q_c), ``eager`` (``use_plan = False``, no constraint: the same passes without the grammar -- the fair
baseline) and ``planned`` (the default step: what leaving the plan costs).  ``--steps`` steps per turn after a warm-up turn,
a host clock around the turn with a device synchronisation at both ends.  ``valid_samples``: the share of the sampled
programs of the timed steps the compiler accepts, which for the joint step is the share of its unsupervised rows the NMN
runs (``nmn_rows_per_step``).

Prints one JSON line per measurement.  Not measured here: trained generators (whose unconstrained samples are mostly valid
already), two ranks, accuracy on CLEVR checkpoints."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]


def sampler_rows(automaton, end, B, T, V, pad, unk, start, seed):
    """[B, T] rows a constrained sampler could emit (uniform over each allowed set), @end@ repeated behind the first, and
    the allowed set of every step with the step's token added [B, T, V]."""
    import numpy as np

    tc, ns, ml = (np.asarray(getattr(automaton, n), dtype=np.int64) for n in ("token_class", "next_state", "min_left"))
    rng = np.random.default_rng(seed)
    state, finished = np.zeros(B, np.int64), np.zeros(B, bool)
    tokens, sets = np.zeros((B, T), np.int64), np.zeros((B, T, V), bool)
    for t in range(T):
        mask = ml[ns[state[:, None], tc[None, :]]] <= T - 1 - t
        mask[:, [pad, unk, start, end]] = False
        mask[finished] = False
        mask[:, end] = finished | (ml[state] == 0)
        draw = rng.random((B, V)) * mask
        tokens[:, t] = draw.argmax(1)
        sets[:, t] = mask
        ended = tokens[:, t] == end
        state = np.where(finished | ended, state, ns[state, tc[tokens[:, t]]])
        finished |= ended
    return tokens, sets


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--steps-t", type=int, default=27)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--qc-questions", type=int, default=128)
    ap.add_argument("--joint-questions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()

    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.modules.grammar import grammar_logits
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.trainers.joint_training import JointTrainingStep, QuestionCodingStep
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("grammar_training_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    pad, unk, start, end = (vocab.get_token_index(t, namespace="programs") for t in ("@@PADDING@@", "@@UNKNOWN@@", "@start@", "@end@"))
    compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    automaton = compiler.decoding_automaton(exclude=(pad, unk, start, end))
    V = vocab.get_vocab_size("programs")

    def events(fn, calls: int) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    if not args.skip_kernel:
        B, T = args.rows, args.steps_t
        host_tokens, host_sets = sampler_rows(automaton, end, B, T, V, pad, unk, start, 0)
        tokens, mask = torch.from_numpy(host_tokens).to(dev), torch.from_numpy(host_sets).to(dev)
        gen = torch.Generator().manual_seed(0)
        logits = (torch.randn(B, T, V, generator=gen) * 3).to(dev).requires_grad_()
        d = torch.randn(B, T, V, generator=gen).to(dev)
        neg, zero = torch.full((), float("-inf"), device=dev), torch.zeros((), device=dev)
        kept = {}

        def kernel_forward():
            kept["k"] = grammar_logits(logits, tokens, automaton, T, pad, unk, start, end)

        def kernel_backward():
            kept["kg"] = torch.autograd.grad(kept["k"][0], logits, d, retain_graph=True)[0]

        def torch_forward():
            masked = torch.where(mask, logits.detach(), neg)
            kept["t"] = masked, torch.logsumexp(masked, -1) - torch.logsumexp(logits.detach(), -1)

        def torch_backward():
            kept["tg"] = torch.where(mask, d, zero)

        # the launches alone, as a caller of the C entry points queues them: outputs allocated once, no autograd node
        from probnmn import _hip, _hip_grammar
        from probnmn.modules.seq2seq_base import constraint_tables

        tc, ns, ml, _ = constraint_tables(automaton, V, end)
        tail = (T, pad, unk, start, end, tc.ctypes.data, ns.ctypes.data, ml.ctypes.data, ns.shape[0], ns.shape[1])
        raw = {"masked": torch.empty(B, T, V, device=dev), "log_mass": torch.empty(B, T, device=dev),
               "outside": torch.empty(B, dtype=torch.int32, device=dev), "d_logits": torch.empty(B, T, V, device=dev)}
        lib, stream, z = _hip_grammar.lib(), _hip.stream_ptr(dev), logits.detach()

        def launch_forward():
            _hip.check(lib.pnmn_grammar_logits(z.data_ptr(), T * V, tokens.data_ptr(), T, raw["masked"].data_ptr(), T * V,
                                               raw["log_mass"].data_ptr(), raw["outside"].data_ptr(), B, T, V, *tail, stream),
                       "grammar_logits")

        def launch_backward():
            _hip.check(lib.pnmn_grammar_logits_bwd(d.data_ptr(), T * V, tokens.data_ptr(), T, raw["d_logits"].data_ptr(), T * V,
                                                   B, T, V, *tail, stream), "grammar_logits_bwd")

        kernel_forward(), kernel_backward(), torch_forward(), torch_backward(), launch_forward(), launch_backward()
        agree = bool(torch.equal(kept["k"][0].detach(), kept["t"][0]) and torch.equal(kept["kg"], kept["tg"])
                     and torch.allclose(kept["k"][1], kept["t"][1], rtol=1e-5, atol=1e-5) and int(kept["k"][2].sum()) == 0
                     and torch.equal(raw["masked"], kept["t"][0]) and torch.equal(raw["d_logits"], kept["tg"]))
        fns = {"launch_fwd": launch_forward, "launch_bwd": launch_backward, "node_fwd": kernel_forward, "node_bwd": kernel_backward,
               "torch_fwd": torch_forward, "torch_bwd": torch_backward}
        for fn in fns.values():
            events(fn, 3)
        took = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                took[k].append(events(fn, args.launches))
        med = {k: statistics.median(v) for k, v in took.items()}
        print(json.dumps({
            "measurement": "kernel", "rows": B, "steps": T, "tokens": V, "launches": args.launches, "rounds": args.rounds,
            "results_agree": agree, "us_per_call": {k: round(1e3 * v, 2) for k, v in med.items()},
            "spread_us": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in took.items()},
            "note": "launch_*: the C entry points alone; node_*: through grammar_logits and autograd.grad (output allocation, the "
                    "autograd engine); torch_*: given the mask on the device"}), flush=True)
        del kept, raw, logits, d, mask, z

    if args.skip_steps:
        return

    def models(joint: bool):
        torch.manual_seed(0)
        ms = [ProgramGenerator(vocab), QuestionReconstructor(vocab), ProgramPrior(vocab, hidden_size=256)]
        if joint:
            ms.append(NeuralModuleNetwork(vocab))
        return [m.to(dev) for m in ms]

    def device_batch(questions: int, joint: bool):
        b = synthetic_batch(vocab, questions, seed=1, with_image=joint)
        b["supervision"][:] = 0
        b["supervision"][::2] = 1
        out = {k: v.to(dev) for k, v in b.items()}
        out["supervision"] = b["supervision"]
        return out

    def turn(step, batch, steps: int, programs=None) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step.step(batch)
            if programs is not None:
                programs.append(out["programs"])  # (a device tensor of the step: read after the clock stops)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    for name, joint, questions in (("question_coding", False, args.qc_questions), ("joint_training", True, args.joint_questions)):
        batch = device_batch(questions, joint)
        make = (lambda ms, **kw: JointTrainingStep(*ms, lr=1e-6, **kw)) if joint else (lambda ms, **kw: QuestionCodingStep(*ms, lr=1e-6, **kw))
        steps = {"grammar": make(models(joint), constraint=automaton), "eager": make(models(joint)), "planned": make(models(joint))}
        steps["eager"].use_plan = False
        for step in steps.values():
            turn(step, batch, 3)
        took, programs = {k: [] for k in steps}, {k: [] for k in steps}
        for _ in range(args.rounds):
            for k, step in steps.items():
                took[k].append(turn(step, batch, args.steps, programs[k]))
        med = {k: statistics.median(v) for k, v in took.items()}
        valid, per_step, length = {}, {}, {}
        for k, rows in programs.items():
            flags = [c.valid for p in rows for c in compiler.compile_batch(p.cpu().numpy())]
            valid[k] = sum(flags) / len(flags)
            per_step[k] = sum(flags) / len(rows)
            length[k] = float(torch.cat([(p != pad).sum(1) for p in rows]).float().mean())
        print(json.dumps({
            "measurement": "step", "step": name, "questions": questions, "supervised": questions - questions // 2,
            "steps_per_turn": args.steps, "rounds": args.rounds, "ms_per_step": {k: round(v, 3) for k, v in med.items()},
            "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in took.items()},
            "grammar_over_eager": round(med["grammar"] / med["eager"], 3), "eager_over_planned": round(med["eager"] / med["planned"], 3),
            "valid_samples": {k: round(v, 4) for k, v in valid.items()},
            ("nmn_rows_per_step" if joint else "valid_rows_per_step"): {k: round(v, 1) for k, v in per_step.items()},
            "tokens_per_sample": {k: round(v, 2) for k, v in length.items()}, "sampled_rows_per_step": questions // 2}), flush=True)
        for step in steps.values():
            step.close()
        del steps


if __name__ == "__main__":
    main()
