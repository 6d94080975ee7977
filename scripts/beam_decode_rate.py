"""What beam-search decoding costs against the existing greedy free-running decode of as many rows.

usage: python scripts/beam_decode_rate.py [--questions 256] [--steps 30] [--beams 1,4,8,16] [--rounds 5] [--window 0.5]

For every beam width K: ``ProgramGenerator.decode_beam`` of B questions (one launch of the beam kernel: B*K hypotheses,
the encoder outputs read per question) against ``decode(..., "greedy")`` of the same encoder state repeated K times
(B*K independent rows, no selection, K times the encoder traffic) -- on the multi-CU decoder kernels the library picks
by default and on the one-workgroup-per-tile kernel the beam kernel is modelled on (PNMN_DECODER_CLUSTER=0).  The model
is untrained and the questions random, so no hypothesis finishes early: every step is paid.  The variants alternate
inside each round; a measurement is the host clock around as many decodes as fill ``--window`` seconds (counted from a
short trial of the variant), ending in a device synchronise, after a warm-up of every shape.  The "beam" figure is the
whole ``decode_beam`` call -- the per-call token table, the trim and the loss with the kernel -- as "greedy" is the whole
``decode`` call.  Prints one JSON line per K: median ms per decode of each variant over the rounds, the spread
(min, max) and the ratios beam / greedy."""
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
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--beams", default="1,4,8,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of decodes per measurement")
    args = ap.parse_args()

    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("beam_decode_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab, max_decoding_steps=args.steps).to(dev).eval()
    questions = synthetic_batch(vocab, args.questions, seed=1)["question"].to(dev)

    def timed(fn, calls: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    with torch.no_grad():
        state = pg.encode(questions)
        for K in [int(k) for k in args.beams.split(",")]:
            wide = {k: v.repeat_interleave(K, 0).contiguous() for k, v in state.items()}

            def beam():
                pg.decode_beam(state, K)

            def greedy():
                pg.decode(wide, decoding_strategy="greedy")

            def greedy_one_workgroup():
                os.environ["PNMN_DECODER_CLUSTER"] = "0"
                try:
                    pg.decode(wide, decoding_strategy="greedy")
                finally:
                    del os.environ["PNMN_DECODER_CLUSTER"]

            variants = (("beam", beam), ("greedy", greedy), ("greedy_one_workgroup", greedy_one_workgroup))
            for _, fn in variants:  # warm-up of every shape
                for _ in range(3):
                    fn()
            calls = {name: max(10, int(args.window * 1e3 / timed(fn, 10)) + 1) for name, fn in variants}
            ms = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    ms[name].append(timed(fn, calls[name]))
            med = {name: statistics.median(v) for name, v in ms.items()}
            print(json.dumps({
                "questions": args.questions, "beam": K, "steps": args.steps, "rows": args.questions * K, "calls": calls,
                "ms": {name: round(med[name], 4) for name in ms},
                "spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in ms.items()},
                "beam_over_greedy": round(med["beam"] / med["greedy"], 3),
                "beam_over_greedy_one_workgroup": round(med["beam"] / med["greedy_one_workgroup"], 3),
                "us_per_step": {name: round(med[name] / args.steps * 1e3, 2) for name in ms}}), flush=True)


if __name__ == "__main__":
    main()
