"""What stochastic beam search costs against the plain beam search of the same width and against the sampled decode of as
many rows, and how many distinct programs each gives with a peaked generator.

usage: python scripts/stochastic_beam_rate.py [--questions 256] [--steps 30] [--beams 2,4,8,16] [--rounds 5] [--window 0.5]

For every width K: ``ProgramGenerator.decode_stochastic_beam`` of B questions (one launch of the beam kernel's stochastic
candidate stage) against ``decode_beam`` at the same K and against ``decode(..., "sampling")`` of the same encoder state
repeated K times (B*K independent rows: what ``num_programs=K`` decodes).  The model is untrained and the questions random,
so no hypothesis finishes early: every step is paid.  The variants alternate inside each round; a measurement is the host
clock around as many decodes as fill ``--window`` seconds, ending in a device synchronise, after a warm-up of every shape
(the method of scripts/beam_decode_rate.py).  Every figure is the whole call, seed draw, token table, trim and loss included.

Then, for a PEAKED generator (the same weights, output layer scaled by ``--peak``) and ``--steps 12``: the distinct valid
programs per question among the K hypotheses of one stochastic beam search under the program automaton, against the K
rows of the constrained sampling decode (``num_programs=K`` with ``constrained_sampling``).  One JSON line per K."""
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
    ap.add_argument("--beams", default="2,4,8,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of decodes per measurement")
    ap.add_argument("--peak", type=float, default=8.0, help="scale of the output layer of the peaked generator")
    args = ap.parse_args()

    import torch

    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import ProgramGenerator
    from probnmn.runtime.program_compiler import ProgramCompiler
    from probnmn.vocabulary import Vocabulary

    if not torch.cuda.is_available():
        raise SystemExit("stochastic_beam_rate.py measures on the GPU; none found")
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

    # the peaked generator and the automaton, for the counts
    torch.manual_seed(0)
    peaked = ProgramGenerator(vocab, max_decoding_steps=12).to(dev).eval()
    with torch.no_grad():
        peaked._output_projection_layer.weight.mul_(args.peak)
        peaked._output_projection_layer.bias.mul_(args.peak)
    compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    automaton = compiler.decoding_automaton(exclude=(pg._pad_index, pg._unk_index, pg._start_index, pg._end_index))

    def distinct_valid(tokens):  # [B, K, T] host -> mean distinct valid programs per question
        B, K, T = tokens.shape
        ok = [c.valid for c in compiler.compile_batch(tokens.reshape(B * K, T).numpy())]
        return sum(len({tuple(tokens[b, k].tolist()) for k in range(K) if ok[b * K + k]}) for b in range(B)) / B

    with torch.no_grad():
        state = pg.encode(questions)
        peaked_state = peaked.encode(questions)
        for K in [int(k) for k in args.beams.split(",")]:
            wide = {k: v.repeat_interleave(K, 0).contiguous() for k, v in state.items()}
            variants = (("stochastic_beam", lambda: pg.decode_stochastic_beam(state, K)),
                        ("beam", lambda: pg.decode_beam(state, K)),
                        ("sampling", lambda: pg.decode(wide, decoding_strategy="sampling")))
            for _, fn in variants:  # warm-up of every shape
                for _ in range(3):
                    fn()
            calls = {name: max(10, int(args.window * 1e3 / timed(fn, 10)) + 1) for name, fn in variants}
            ms = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    ms[name].append(timed(fn, calls[name]))
            med = {name: statistics.median(v) for name, v in ms.items()}
            torch.manual_seed(K)
            without = peaked.decode_stochastic_beam(peaked_state, K, constraint=automaton)
            finite = torch.isfinite(without["beam_log_probabilities"]).cpu()
            tokens = without["beam_predictions"].cpu()
            tokens[~finite] = 0  # (an empty slot: no program)
            wide_peaked = {k: v.repeat_interleave(K, 0).contiguous() for k, v in peaked_state.items()}
            drawn = peaked.decode_constrained(wide_peaked, automaton)["predictions"].cpu().view(args.questions, K, -1)
            line = {"questions": args.questions, "beam": K, "steps": args.steps, "rows": args.questions * K, "calls": calls,
                    "ms": {name: round(med[name], 4) for name in ms},
                    "spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in ms.items()},
                    "stochastic_over_beam": round(med["stochastic_beam"] / med["beam"], 3),
                    "stochastic_over_sampling": round(med["stochastic_beam"] / med["sampling"], 3),
                    "peaked_distinct_valid_per_question": {"stochastic_beam": round(distinct_valid(tokens), 3),
                                                           "num_programs": round(distinct_valid(drawn), 3)}}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
