"""What a marginal answer costs: the kernel (pnmn_answer_marginal, csrc/answer_marginal.hip) against the torch composition
it replaces, and ``predict_answers`` with several programs per question against one.

usage: python scripts/marginal_answer_rate.py [--groups 256] [--rows-per-group 8] [--answers 28] [--launches 20]
                                              [--rounds 5] [--questions 256] [--batches 2]

``kernel``: ``--groups`` groups of ``--rows-per-group`` hypothesis rows, ``--answers`` answers, about 0.7 of the rows valid,
random log-weights.  ``composition`` is the same result from torch ops on the same device tensors (the groups are equally
long, so it is dense): ``log_softmax`` over the answers, the log-weights masked by validity and normalised by a
``logsumexp`` over the hypotheses, a ``logsumexp`` over the hypotheses of their sum, ``argmax`` -- and the per-row
``argmax`` and the support, which the kernel also writes.  Device events around ``--launches`` back-to-back launches of
each, the two alternating, ``--rounds`` rounds, the median and the spread; the results are compared once.

``predict_answers``: ms per batch of ``--questions`` questions over ``--batches`` batches of full-size feature maps (a host
clock around the call, which ends with the records on the host), the variants alternating inside each round after one
warm-up call of each, for two generators:
    untrained    randomly initialised: the hypotheses of a question are nearly all distinct
    peaked       its output bias made steep, so that every draw is the same program: the samples merge into one row
and three variants, all under the validity constraint so that every program runs:
    single       one sampled program per question (``constrained_sampling=True``) -- the parent behaviour, the yardstick
    beam4        ``beam_size=4, marginal=True, constrained=True``
    sampled8     ``num_programs=8, constrained_sampling=True``
``rows_per_question`` is the mean number of NMN rows a question cost (its ``support``).  Random weights: the kernels' time
does not depend on the values, only on which programs the generator emits.

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
    ap.add_argument("--batches", type=int, default=2, help="batches per predict_answers call")
    ap.add_argument("--skip-answers", action="store_true", help="the kernel measurement only")
    args = ap.parse_args()

    import torch

    from probnmn import _hip
    from probnmn.evaluators import predict_answers

    if not torch.cuda.is_available():
        raise SystemExit("marginal_answer_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    G, K, A = args.groups, args.rows_per_group, args.answers
    gen = torch.Generator().manual_seed(0)
    logits = (torch.randn(G * K, A, generator=gen) * 3).to(dev)
    valid = (torch.rand(G * K, generator=gen) < 0.7).to(torch.int32).to(dev)
    log_weight = (torch.randn(G * K, generator=gen) * 4 - 20).to(dev)
    group_start = (torch.arange(G + 1, dtype=torch.int32) * K).to(dev)
    out = {"log_marginal": torch.empty(G, A, device=dev), "predictions": torch.empty(G, dtype=torch.long, device=dev),
           "row_predictions": torch.empty(G * K, dtype=torch.long, device=dev), "row_weight": torch.empty(G * K, device=dev),
           "support": torch.empty(G, dtype=torch.int32, device=dev)}
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def kernel():
        _hip.check(lib.pnmn_answer_marginal(
            logits.data_ptr(), valid.data_ptr(), log_weight.data_ptr(), group_start.data_ptr(), out["log_marginal"].data_ptr(),
            out["predictions"].data_ptr(), out["row_predictions"].data_ptr(), out["row_weight"].data_ptr(),
            out["support"].data_ptr(), G, G * K, A, A, stream), "answer_marginal")

    def composition():
        ok = valid.view(G, K) != 0
        lw = log_weight.view(G, K).masked_fill(~ok, float("-inf"))
        log_w = lw - torch.logsumexp(lw, 1, keepdim=True)
        log_marginal = torch.logsumexp(log_w.unsqueeze(2) + torch.log_softmax(logits.view(G, K, A), 2), 1)
        support = ok.sum(1)
        predictions = torch.where(support > 0, log_marginal.argmax(1), A)
        row_predictions = torch.where(ok.view(-1), logits.argmax(1), A)
        return log_marginal, predictions, row_predictions, log_w.exp(), support

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
    supported = want[4] > 0
    agree = bool(torch.allclose(out["log_marginal"][supported], want[0][supported], rtol=1e-5, atol=1e-5)
                 and torch.equal(out["support"].long(), want[4]) and torch.equal(out["row_predictions"], want[2]))
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
    if args.skip_answers:
        return

    # ---- predict_answers: several programs per question against one
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    B = args.questions
    pg, nmn = ProgramGenerator(vocab).to(dev), NeuralModuleNetwork(vocab).to(dev)
    batches = []
    for s in range(args.batches):
        b = synthetic_batch(vocab, B, seed=s)
        batches.append({"question": b["question"].to(dev), "image": b["image"].to(dev)})
    variants = (("single", dict(constrained_sampling=True)), ("beam4", dict(beam_size=4, marginal=True, constrained=True)),
                ("sampled8", dict(num_programs=8, constrained_sampling=True)))

    def run(options, rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records = predict_answers(pg, nmn, batches, vocab, **options)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        rows.append(sum(r.get("support", 1) for r in records) / len(records))
        return 1e3 * seconds / args.batches

    def measure(generator):
        rows = {name: [] for name, _ in variants}
        for name, options in variants:
            run(options, [])
        took = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, options in variants:
                took[name].append(run(options, rows[name]))
        med = {name: statistics.median(v) for name, v in took.items()}
        print(json.dumps({
            "measurement": "predict_answers", "generator": generator, "questions_per_batch": B, "batches": args.batches,
            "rounds": args.rounds, "ms_per_batch": {name: round(v, 2) for name, v in med.items()},
            "spread_ms": {name: [round(min(v), 2), round(max(v), 2)] for name, v in took.items()},
            "rows_per_question": {name: round(statistics.mean(v), 2) for name, v in rows.items()},
            "beam4_over_single_time": round(med["beam4"] / med["single"], 3),
            "sampled8_over_single_time": round(med["sampled8"] / med["single"], 3)}), flush=True)

    measure("untrained")
    with torch.no_grad():  # every draw takes the best-ranked token the validity rule allows: one program for all
        for rank, token in enumerate(("count", "scene", "@end@"), start=1):
            pg._output_projection_layer.bias[vocab.get_token_index(token, namespace="programs")] += 40.0 * rank
    measure("peaked")


if __name__ == "__main__":
    main()
