"""What inferring programs from question AND answer costs: the kernel (pnmn_answer_posterior, csrc/answer_posterior.hip)
against the torch composition it replaces, and ``infer_programs`` over a beam against ``predict_answers`` over the same beam.

usage: python scripts/program_inference_rate.py [--groups 256] [--rows-per-group 8] [--answers 28] [--launches 20] [--rounds 5]
                                                [--questions 256] [--batches 2] [--skip-inference]

``kernel``: ``--groups`` groups of ``--rows-per-group`` hypothesis rows of ``--answers`` answer logits, random validity-free
log-weights, one random given answer per group, ``w_a`` = 1.  ``composition`` is the same result from torch ops on the same
device tensors (the groups are equally long, so it is dense): ``log_softmax`` of the logits, ``gather`` of the given answer,
``argmax``; ``log_softmax`` of the weights per group; the score; over the hypotheses of a group ``logsumexp`` (the evidence),
the normalised log-posterior, ``argmax``, the support and the consistent rows.  Device events around ``--launches``
back-to-back launches of each, the two alternating, ``--rounds`` rounds after a warm-up, the median and the spread; the
results are compared once.

``infer_programs``: ms per batch of ``--questions`` questions over ``--batches`` batches of full-size feature maps (a host
clock around the call, which ends with the records on the host), ``beam_size=4, constrained=True``, against
``predict_answers(..., beam_size=4, marginal=True, constrained=True)`` -- the same hypotheses, the same NMN passes, the
marginal kernel in the place of the posterior kernel --, the two alternating inside each round after one warm-up call of
each.  Random weights: the kernels' time does not depend on the values.

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
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--rows-per-group", type=int, default=8)
    ap.add_argument("--answers", type=int, default=28)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--batches", type=int, default=2, help="batches per call of an evaluator")
    ap.add_argument("--skip-inference", action="store_true", help="the kernel measurement only")
    args = ap.parse_args()

    import torch

    from probnmn import _hip
    from probnmn.evaluators import infer_programs, predict_answers
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("program_inference_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    G, K, A = args.groups, args.rows_per_group, args.answers
    R = G * K
    gen = torch.Generator().manual_seed(0)
    logits = (torch.randn(R, A, generator=gen) * 3).to(dev)
    log_weight = (torch.randn(R, generator=gen) * 4 - 20).to(dev)
    answers = torch.randint(0, A, (G,), generator=gen).to(dev)
    group_start = (torch.arange(G + 1, dtype=torch.int32) * K).to(dev)
    f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = {"log_answer": torch.empty(R, **f), "row_predictions": torch.empty(R, dtype=torch.long, device=dev),
           "log_posterior": torch.empty(R, **f), "log_evidence": torch.empty(G, **f), "best_row": torch.empty(G, **i),
           "support": torch.empty(G, **i), "consistent_count": torch.empty(G, **i), "first_consistent": torch.empty(G, **i)}
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def kernel():
        _hip.check(lib.pnmn_answer_posterior(
            logits.data_ptr(), 0, log_weight.data_ptr(), answers.data_ptr(), group_start.data_ptr(), 1.0, out["log_answer"].data_ptr(),
            out["row_predictions"].data_ptr(), out["log_posterior"].data_ptr(), out["log_evidence"].data_ptr(),
            out["best_row"].data_ptr(), out["support"].data_ptr(), out["consistent_count"].data_ptr(),
            out["first_consistent"].data_ptr(), G, R, A, A, stream), "answer_posterior")

    def composition():
        log_answer = torch.log_softmax(logits, 1).gather(1, answers.repeat_interleave(K).unsqueeze(1)).squeeze(1)
        row_predictions = logits.argmax(1)
        score = torch.log_softmax(log_weight.view(G, K), 1) + log_answer.view(G, K)
        usable = torch.isfinite(score)
        score = score.masked_fill(~usable, float("-inf"))
        log_evidence = torch.logsumexp(score, 1)
        log_posterior = score - log_evidence.unsqueeze(1)
        best_row = score.argmax(1) + torch.arange(G, device=dev) * K
        consistent = usable & (row_predictions.view(G, K) == answers.unsqueeze(1))
        return log_answer, row_predictions, log_posterior.view(-1), log_evidence, best_row, usable.sum(1), consistent.sum(1)

    def events(fn, calls: int) -> float:
        """ms per call: device events around ``calls`` calls."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    kernel()
    want = composition()
    bound = 1e-5 * (1 + float((want[2].view(G, K) + want[3].unsqueeze(1)).abs().max()))  # (1 + the largest |score|)
    agree = bool(torch.allclose(out["log_answer"], want[0], rtol=1e-5, atol=1e-5) and torch.equal(out["row_predictions"], want[1])
                 and torch.allclose(out["log_posterior"], want[2], rtol=0, atol=bound)
                 and torch.allclose(out["log_evidence"], want[3], rtol=0, atol=bound)
                 and torch.equal(out["best_row"].long(), want[4]) and torch.equal(out["support"].long(), want[5])
                 and torch.equal(out["consistent_count"].long(), want[6]))
    events(kernel, 3), events(composition, 3)
    ms = {"kernel": [], "composition": []}
    for _ in range(args.rounds):
        ms["kernel"].append(events(kernel, args.launches))
        ms["composition"].append(events(composition, args.launches))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "measurement": "kernel", "groups": G, "rows_per_group": K, "answers": A, "launches": args.launches, "rounds": args.rounds,
        "results_agree": agree, "us_per_launch": {k: round(1e3 * v, 2) for k, v in med.items()},
        "spread_us": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()},
        "kernel_over_composition_time": round(med["kernel"] / med["composition"], 4)}), flush=True)
    if args.skip_inference:
        return

    # ---- infer_programs over a beam against predict_answers over the same beam
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator

    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    B = args.questions
    pg, nmn = ProgramGenerator(vocab).to(dev), NeuralModuleNetwork(vocab).to(dev)
    batches = []
    for s in range(args.batches):
        b = synthetic_batch(vocab, B, seed=s)
        batches.append({k: b[k].to(dev) for k in ("question", "image", "answer")})
    variants = (("predict_answers_marginal", lambda: predict_answers(pg, nmn, batches, vocab, beam_size=4, marginal=True, constrained=True)),
                ("infer_programs", lambda: infer_programs(pg, nmn, batches, vocab, beam_size=4, constrained=True)))

    def run(call, rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records = call()
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        rows.append(sum(r["support"] for r in records) / len(records))
        return 1e3 * seconds / args.batches

    rows = {name: [] for name, _ in variants}
    for name, call in variants:
        run(call, [])
    took = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, call in variants:
            took[name].append(run(call, rows[name]))
    med = {name: statistics.median(v) for name, v in took.items()}
    print(json.dumps({
        "measurement": "infer_programs", "questions_per_batch": B, "batches": args.batches, "rounds": args.rounds,
        "ms_per_batch": {name: round(v, 2) for name, v in med.items()},
        "spread_ms": {name: [round(min(v), 2), round(max(v), 2)] for name, v in took.items()},
        "rows_per_question": {name: round(statistics.mean(v), 2) for name, v in rows.items()},
        "inference_over_marginal_time": round(med["infer_programs"] / med["predict_answers_marginal"], 3)}), flush=True)


if __name__ == "__main__":
    main()
