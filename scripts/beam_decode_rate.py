"""What beam-search decoding costs against the existing greedy free-running decode of as many rows.

usage: python scripts/beam_decode_rate.py [--questions 256] [--steps 30] [--beams 1,4,8,16] [--rounds 5] [--window 0.5]
                                          [--constrained | --variants beam,...]

For every beam width K: ``ProgramGenerator.decode_beam`` of B questions (one launch of the beam kernel: B*K hypotheses,
the encoder outputs read per question) against ``decode(..., "greedy")`` of the same encoder state repeated K times
(B*K independent rows, no selection, K times the encoder traffic) -- on the multi-CU decoder kernels the library picks
by default and on the one-workgroup-per-tile kernel the beam kernel is modelled on (PNMN_DECODER_CLUSTER=0).  The model
is untrained and the questions random, so no hypothesis finishes early: every step is paid.  The variants alternate
inside each round; a measurement is the host clock around as many decodes as fill ``--window`` seconds (counted from a
short trial of the variant), ending in a device synchronise, after a warm-up of every shape.  The "beam" figure is the
whole ``decode_beam`` call -- the per-call token table, the trim and the loss with the kernel -- as "greedy" is the whole
``decode`` call.  Prints one JSON line per K: median ms per decode of each variant over the rounds, the spread
(min, max) and the ratios beam / greedy.

``--constrained``: what the grammar constraint costs.  The variants are then "beam" and "beam_constrained" -- the same
``decode_beam`` under the program compiler's decoding automaton (``pnmn_attn_lstm_beam`` with its tables) -- alternating
inside each round, and the ratio printed is constrained / unconstrained.  ``--variants``: any subset, in the order given
(e.g. ``beam`` alone, to compare two builds of the library process against process)."""
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
    ap.add_argument("--constrained", action="store_true", help="time beam against beam under the decoding automaton")
    ap.add_argument("--variants", default=None, help="comma-separated subset of beam, beam_constrained, greedy, greedy_one_workgroup")
    args = ap.parse_args()
    if args.variants is not None:
        chosen = args.variants.split(",")
    else:
        chosen = ["beam", "beam_constrained"] if args.constrained else ["beam", "greedy", "greedy_one_workgroup"]

    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("beam_decode_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    pg = ProgramGenerator(vocab, max_decoding_steps=args.steps).to(dev).eval()
    questions = synthetic_batch(vocab, args.questions, seed=1)["question"].to(dev)
    automaton = None
    if "beam_constrained" in chosen:
        compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
        automaton = compiler.decoding_automaton(exclude=(pg._pad_index, pg._unk_index, pg._start_index, pg._end_index))

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
            wide = None
            if "greedy" in chosen or "greedy_one_workgroup" in chosen:
                wide = {k: v.repeat_interleave(K, 0).contiguous() for k, v in state.items()}

            def beam():
                pg.decode_beam(state, K)

            def beam_constrained():
                pg.decode_beam(state, K, constraint=automaton)

            def greedy():
                pg.decode(wide, decoding_strategy="greedy")

            def greedy_one_workgroup():
                os.environ["PNMN_DECODER_CLUSTER"] = "0"
                try:
                    pg.decode(wide, decoding_strategy="greedy")
                finally:
                    del os.environ["PNMN_DECODER_CLUSTER"]

            known = {"beam": beam, "beam_constrained": beam_constrained, "greedy": greedy,
                     "greedy_one_workgroup": greedy_one_workgroup}
            variants = tuple((name, known[name]) for name in chosen)
            for _, fn in variants:  # warm-up of every shape
                for _ in range(3):
                    fn()
            calls = {name: max(10, int(args.window * 1e3 / timed(fn, 10)) + 1) for name, fn in variants}
            ms = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    ms[name].append(timed(fn, calls[name]))
            med = {name: statistics.median(v) for name, v in ms.items()}
            line = {
                "questions": args.questions, "beam": K, "steps": args.steps, "rows": args.questions * K, "calls": calls,
                "ms": {name: round(med[name], 4) for name in ms},
                "spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in ms.items()}}
            for key, over, under in (("beam_over_greedy", "beam", "greedy"),
                                     ("beam_over_greedy_one_workgroup", "beam", "greedy_one_workgroup"),
                                     ("constrained_over_beam", "beam_constrained", "beam")):
                if over in med and under in med:
                    line[key] = round(med[over] / med[under], 3)
            line["us_per_step"] = {name: round(med[name] / args.steps * 1e3, 2) for name in ms}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
