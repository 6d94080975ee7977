"""What explaining an answer costs: ``predict_answers(..., explain=True)`` against ``explain=False``, and the overlay kernel
(pnmn_attention_overlay, csrc/attention_maps.hip) against the HBM write bandwidth.

usage: python scripts/explain_rate.py [--questions 256] [--height 320] [--width 480] [--maps-per-question 10]
                                      [--launches 20] [--rounds 5] [--batches 2]

``kernel``: device events around ``--launches`` back-to-back launches of ``pnmn_attention_overlay`` (the C entry, one
output tensor, no allocation between launches) on ``--questions`` images with ``--maps-per-question`` 14x14 maps each,
handed over sorted by image as ``attention_overlay`` does; ``--rounds`` times, the median.  The bytes the kernel must move
are computed here from the shapes: 3 * Hi * Wi written per map, 3 * Hi * Wi read per IMAGE (once: the maps of an image
are neighbours) and 4 * H * W per map.  Reported: the achieved write rate (bytes written over time) and the share of the
6.3 TB/s of HBM bandwidth that is achievable on the MI355X which all moved bytes amount to.  At the defaults the output is
1.18 GB, several times the Infinity Cache.

``predict_answers``: questions/s over ``--batches`` batches of ``--questions`` questions (a host clock around the call,
which ends with the records on the host), the variants alternating inside each round, after one warm-up call of each:
    pixels              explain=False on "pixels" batches through the extractor -- the parent behaviour, the yardstick
    pixels+overlays     explain=True on the same batches: maps, overlays, and their copies to the host
    features            explain=False on "image" batches (features extracted beforehand): the yardstick of the next line
    features+maps       explain=True on those: no pixels, so maps only
Programs are sampled under the validity constraint (``constrained_sampling=True``) from a randomly initialised generator,
so every question has a valid program and maps to show; ``steps_per_question`` is their mean number.  Random weights: the
kernels' time does not depend on the values.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]

ACHIEVABLE_HBM_BYTES_PER_S = 6.3e12


def overlay_bytes(n_images: int, maps_per_image: int, hi: int, wi: int, h: int, w: int):
    """(bytes written, bytes read) of one overlay launch, from the shapes."""
    n = n_images * maps_per_image
    return n * 3 * hi * wi, n_images * 3 * hi * wi + n * 4 * h * w


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--maps-per-question", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=2, help="batches per predict_answers call")
    ap.add_argument("--skip-answers", action="store_true", help="the kernel measurement only")
    args = ap.parse_args()

    import torch

    from probnmn import _hip
    from probnmn.evaluators import default_colormap, predict_answers

    if not torch.cuda.is_available():
        raise SystemExit("explain_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, hi, wi, per, H, W = args.questions, args.height, args.width, args.maps_per_question, 14, 14
    gen = torch.Generator().manual_seed(0)
    pixels = torch.randint(0, 256, (B, hi, wi, 3), dtype=torch.uint8, generator=gen).to(dev)

    # ---- the kernel alone
    n = B * per
    maps = torch.rand(n, H, W, generator=gen).to(dev)
    image_of = torch.arange(B, dtype=torch.int32).repeat_interleave(per).to(dev)
    lut = default_colormap().to(dev)
    out = torch.empty(n, hi, wi, 3, dtype=torch.uint8, device=dev)
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def launch():
        _hip.check(lib.pnmn_attention_overlay(maps.data_ptr(), image_of.data_ptr(), pixels.data_ptr(), 3 * hi * wi, B, hi, wi,
                                              lut.data_ptr(), 160, out.data_ptr(), n, H, W, stream), "attention_overlay")

    def events(fn, calls: int) -> float:
        """ms per call: device events around ``calls`` calls."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    events(launch, 3)
    ms = [events(launch, args.launches) for _ in range(args.rounds)]
    med = statistics.median(ms)
    written, read = overlay_bytes(B, per, hi, wi, H, W)
    print(json.dumps({
        "measurement": "kernel", "images": B, "maps": n, "map": [H, W], "image": [hi, wi], "launches": args.launches,
        "ms_per_launch": round(med, 4), "spread_ms": [round(min(ms), 4), round(max(ms), 4)],
        "bytes_written": written, "bytes_read": read,
        "write_bytes_per_s": round(written / (med * 1e-3), 0),
        "share_of_achievable_hbm": round((written + read) / (med * 1e-3) / ACHIEVABLE_HBM_BYTES_PER_S, 4)}), flush=True)
    del out, maps
    if args.skip_answers:
        return

    # ---- predict_answers with and without the explanation
    from probnmn.data.feature_extractor import ResNet101Stage3
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(0)
    extractor = ResNet101Stage3().to(dev)
    pg, nmn = ProgramGenerator(vocab).to(dev), NeuralModuleNetwork(vocab).to(dev)
    questions = [synthetic_batch(vocab, B, seed=s, with_image=False)["question"].to(dev) for s in range(args.batches)]
    with torch.no_grad():
        features = extractor.forward_pixels(pixels)
    from_pixels = [{"question": q, "pixels": pixels} for q in questions]
    from_features = [{"question": q, "image": features} for q in questions]
    steps = []

    def run(batches, explain):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records = predict_answers(pg, nmn, batches, vocab, extractor=extractor, constrained_sampling=True, explain=explain)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        if explain:
            steps.append(sum(len(r["steps"]) for r in records) / len(records))
        return len(records) / seconds

    variants = (("pixels", from_pixels, False), ("pixels+overlays", from_pixels, True),
                ("features", from_features, False), ("features+maps", from_features, True))
    for _, batches, explain in variants:
        run(batches, explain)
    rate = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, batches, explain in variants:
            rate[name].append(run(batches, explain))
    med = {name: statistics.median(v) for name, v in rate.items()}
    print(json.dumps({
        "measurement": "predict_answers", "questions_per_batch": B, "batches": args.batches, "image": [hi, wi],
        "steps_per_question": round(statistics.mean(steps), 2),
        "questions_per_s": {name: round(v, 1) for name, v in med.items()},
        "spread_questions_per_s": {name: [round(min(v), 1), round(max(v), 1)] for name, v in rate.items()},
        "ms_per_batch": {name: round(1e3 * B / v, 2) for name, v in med.items()},
        "pixels_overlays_over_pixels_time": round(med["pixels"] / med["pixels+overlays"], 4),
        "features_maps_over_features_time": round(med["features"] / med["features+maps"], 4)}), flush=True)


if __name__ == "__main__":
    main()
