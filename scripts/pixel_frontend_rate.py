"""What the image front end (pnmn_image_prep: Pillow-exact resize + normalise, csrc/image_prep.hip) costs.

usage: python scripts/pixel_frontend_rate.py [--images 128] [--height 320] [--width 480] [--size 224] [--launches 200]
                                             [--rounds 5] [--batches 4]

Two measurements on uint8 images of CLEVR's size, after a warm-up of every shape:

``kernel``: device events around ``--launches`` back-to-back launches of ``pnmn_image_prep`` into one output tensor (the
C entry, no allocation between launches), ``--rounds`` times; the median time per launch, and the bytes the transform
must move -- ``3 * Hin * Win`` in and ``16 * Hout * Wout`` out per image, computed here from the shapes -- over that time,
as bytes/s and as a share of the 6.3 TB/s of HBM bandwidth that is achievable on the MI355X.  (The input batch, 59 MB
at the defaults, and the output, 103 MB, fit in the 256 MB Infinity Cache together: the share is of the HBM figure all the
same, as the bound the kernel is held to.)

``extractor``: images/s of ``ResNet101Stage3.forward_pixels`` on the uint8 batch against ``forward`` on floats prepared
beforehand (the front end's own output, as NCHW), alternating inside each round; each measurement is device events around
``--batches`` batches.  Randomly initialised weights: the convolutions' time does not depend on the values.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]

ACHIEVABLE_HBM_BYTES_PER_S = 6.3e12


def transform_bytes(n: int, h: int, w: int, size: int) -> int:
    return n * (3 * h * w + 16 * size * size)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4, help="extractor batches per measurement")
    args = ap.parse_args()

    import torch

    from probnmn import _hip
    from probnmn.data import feature_extractor as fe

    if not torch.cuda.is_available():
        raise SystemExit("pixel_frontend_rate.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    n, h, w, size = args.images, args.height, args.width, (args.size, args.size)
    pixels = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)

    def events(fn, calls: int) -> float:
        """ms per call: device events around ``calls`` calls."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    # ---- the kernel alone
    out = fe.resize_normalize(pixels, size)  # (builds and caches the tables)
    kx, xb, ky, yb, lut, ksx, ksy = fe._prep_tables(h, w, size, dev)
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def launch():
        _hip.check(lib.pnmn_image_prep(pixels.data_ptr(), 3 * h * w, n, h, w, kx.data_ptr(), xb.data_ptr(), ksx, ky.data_ptr(),
                                       yb.data_ptr(), ksy, lut.data_ptr(), out.data_ptr(), size[0], size[1], stream), "image_prep")

    events(launch, 20)
    ms = [events(launch, args.launches) for _ in range(args.rounds)]
    med = statistics.median(ms)
    moved = transform_bytes(n, h, w, args.size)
    print(json.dumps({
        "measurement": "kernel", "images": n, "input": [h, w], "output": list(size), "launches": args.launches,
        "ms_per_launch": round(med, 4), "spread_ms": [round(min(ms), 4), round(max(ms), 4)],
        "us_per_image": round(med * 1e3 / n, 3), "bytes_per_launch": moved,
        "bytes_per_s": round(moved / (med * 1e-3), 0),
        "share_of_achievable_hbm": round(moved / (med * 1e-3) / ACHIEVABLE_HBM_BYTES_PER_S, 4)}), flush=True)

    # ---- the extractor from pixels against the extractor from prepared floats
    torch.manual_seed(0)
    model = fe.ResNet101Stage3().to(dev)
    floats = out[..., :3].permute(0, 3, 1, 2).contiguous()
    variants = (("forward_pixels", lambda: model.forward_pixels(pixels, size)), ("forward", lambda: model(floats)))
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    rate = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            rate[name].append(n / (events(fn, args.batches) * 1e-3))
    med = {name: statistics.median(v) for name, v in rate.items()}
    print(json.dumps({
        "measurement": "extractor", "images": n, "input": [h, w], "output": list(size), "batches": args.batches,
        "images_per_s": {name: round(v, 1) for name, v in med.items()},
        "spread_images_per_s": {name: [round(min(v), 1), round(max(v), 1)] for name, v in rate.items()},
        "us_per_image": {name: round(1e6 / v, 2) for name, v in med.items()},
        "forward_pixels_over_forward_time": round(med["forward"] / med["forward_pixels"], 4)}), flush=True)


if __name__ == "__main__":
    main()
