"""Half-precision and 8-bit feature stores against the fp32 ones, in ONE process, warmed, the variants alternating:

  * the gather kernel alone (PinnedFeatureStore.gather): GB/s over PCIe and questions/s at 128 and 1024 questions, for
    a pinned store of every dtype of --dtypes;
  * pnmn_expand_rows alone (ResidentRows.materialize of every narrow store of --resident) at 519 and 1024 rows against
    its HBM floor (bytes read + written over the peak bandwidth);
  * the 1024-question joint step fed through PrefetchingLoader from every pinned and every resident store, fresh
    random rows every step (what bench.py: ingest_side does for the fp32 pair);
  * what it takes to fill each store.

The comparison that counts is between the variants of one run; every timed region ends in a device synchronise.
Usage: python scripts/half_store_rate.py [--dtypes fp32,fp16,bf16,fp8e4m3] [--resident fp32,fp16,fp8e4m3] [--rows 4096]
                                         [--batch 1024] [--steps 10] [--rounds 3] [--out result.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "probnmn-clevr_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from probnmn.data.feature_store import DeviceFeatureStore, PinnedFeatureStore, PrefetchingLoader  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
C, H, W = 1024, 14, 14
NAMES = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16", torch.float8_e4m3fn: "fp8e4m3",
         torch.float8_e5m2: "fp8e5m2"}
DTYPES = {name: dtype for dtype, name in NAMES.items()}


def dtype_list(text):
    names = [n for n in text.split(",") if n]
    unknown = [n for n in names if n not in DTYPES]
    if unknown or not names:
        raise argparse.ArgumentTypeError("dtypes are a comma-separated list of %s, got %r" % (", ".join(DTYPES), text))
    return [DTYPES[n] for n in names]


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", type=dtype_list, default=dtype_list("fp32,fp16,bf16,fp8e4m3"), help="pinned stores to compare")
    ap.add_argument("--resident", type=dtype_list, default=dtype_list("fp32,fp16,fp8e4m3"), help="resident stores to compare")
    ap.add_argument("--rows", type=int, default=4096, help="rows of every store (0.8 MB each in fp32)")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10, help="timed joint steps per variant and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="kernels and fills only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, result = args.rows, {"rows": args.rows, "rounds": args.rounds}

    g = torch.Generator().manual_seed(77)
    feats = np.empty((rows, C, H, W), np.float32)
    blk = torch.randn(256, C, H, W, generator=g).relu_().numpy()
    for lo in range(0, rows, 256):
        feats[lo:lo + 256] = blk[: min(256, rows - lo)]

    # ---- fills ---------------------------------------------------------------------------------------------------
    pinned, resident, fills = {}, {}, {}
    for dtype in args.dtypes:
        t0 = time.perf_counter()
        pinned[dtype] = PinnedFeatureStore(feats, dtype=dtype)
        fills["pinned_" + NAMES[dtype]] = round(time.perf_counter() - t0, 2)
    for dtype in args.resident:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident[dtype] = DeviceFeatureStore(feats, dev, dtype=dtype)
        torch.cuda.synchronize()
        fills["resident_" + NAMES[dtype]] = round(time.perf_counter() - t0, 2)
    del feats
    result["fill_seconds"] = fills
    print("fill of %d rows (%.2f GB in fp32), seconds: %s" % (rows, rows * C * H * W * 4 / 1e9, fills), flush=True)

    # ---- the gather alone ----------------------------------------------------------------------------------------
    result["gather"] = {}
    for B in (128, 1024):
        idx = torch.randint(0, rows, (B,), generator=g).to(dev)
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        for store in pinned.values():
            store.gather(idx, dev, out=out)
        torch.cuda.synchronize()
        ms = {dtype: [] for dtype in pinned}
        for _ in range(args.rounds):
            for dtype, store in pinned.items():
                ms[dtype].append(event_ms(lambda: store.gather(idx, dev, out=out), 5))
        for dtype, store in pinned.items():
            t = median(ms[dtype])
            nbytes = B * C * H * W * store.store.element_size()
            result["gather"]["%s_%d" % (NAMES[dtype], B)] = {"ms": round(t, 3), "GBs_over_pcie": round(nbytes / t / 1e6, 1),
                                                             "questions_per_s": round(B / t * 1e3)}
            print("gather %4d questions from pinned %s: %.3f ms = %.1f GB/s over PCIe = %.0f questions/s"
                  % (B, NAMES[dtype], t, nbytes / t / 1e6, B / t * 1e3), flush=True)
        del out

    # ---- the widening of resident rows alone ---------------------------------------------------------------------
    result["expand_rows"] = {}
    narrow = [dtype for dtype in resident if dtype != torch.float32]
    for B in (519, 1024):
        index = torch.randint(0, rows, (B,), generator=g)
        batch_rows = {dtype: resident[dtype].batch(index) for dtype in narrow}
        for b in batch_rows.values():
            b.materialize()
        torch.cuda.synchronize()
        ms = {dtype: [] for dtype in narrow}
        for _ in range(args.rounds):
            for dtype in narrow:
                ms[dtype].append(event_ms(batch_rows[dtype].materialize, 10))
        for dtype in narrow:
            t = median(ms[dtype])
            floor = B * C * H * W * (resident[dtype].rows.element_size() + 4) / HBM_PEAK * 1e3
            result["expand_rows"]["%s_%d" % (NAMES[dtype], B)] = {"ms": round(t, 4), "hbm_floor_ms": round(floor, 4),
                                                                  "of_floor": round(t / floor, 2)}
            print("expand_rows %4d rows of %s: %.4f ms, HBM floor %.4f ms (x%.2f; the index upload is in it)"
                  % (B, NAMES[dtype], t, floor, t / floor), flush=True)

    # ---- the joint step fed from each store ----------------------------------------------------------------------
    if not args.no_step:
        import bench
        from probnmn.data.synthetic import synthetic_batch
        from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
        from probnmn.trainers.joint_training import JointTrainingStep
        from probnmn.vocabulary import Vocabulary

        n, k, w = args.batch, args.steps, 3
        vocab = Vocabulary.clevr()
        torch.manual_seed(0)
        nmn = NeuralModuleNetwork(vocab).to(dev)
        pg, qr = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev)
        prior = ProgramPrior(vocab, hidden_size=256).to(dev)
        fit_batch = bench.device_batch(vocab, n, 1000, dev)
        bench.fit_program_generator(pg, vocab, fit_batch, dev, 1500, 0.95)
        trainer = JointTrainingStep(pg, qr, prior, nmn, **bench.JOINT)
        for _ in range(8):
            trainer.step(fit_batch)
        torch.cuda.synchronize()
        del fit_batch
        host = synthetic_batch(vocab, n, seed=1000)
        del host["image"]

        def batches(count):
            for _ in range(count):
                b = dict(host)
                b["image_index"] = torch.randint(0, rows, (n,), generator=g)
                yield b

        def run(store):
            it = iter(PrefetchingLoader(batches(w + k + 1), store, dev, method="kernel"))
            for _ in range(w):
                trainer.step(next(it))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                trainer.step(next(it))
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            it.close()
            return elapsed / k * 1e3

        variants = [("pinned_" + NAMES[dtype], store) for dtype, store in pinned.items()] + \
                   [("resident_" + NAMES[dtype], store) for dtype, store in resident.items()]
        ms = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, store in variants:
                ms[name].append(run(store))
        result["joint_step_ms"] = {name: {"median": round(median(v), 3), "rounds": [round(x, 3) for x in v]} for name, v in ms.items()}
        for name, v in ms.items():
            print("joint step of %d questions fed from %-13s: %.2f ms per step (rounds: %s)"
                  % (n, name, median(v), ", ".join("%.2f" % x for x in v)), flush=True)
        for name in ms:
            if name != "pinned_fp32" and name.startswith("pinned_") and "pinned_fp32" in ms:
                a, b = median(ms["pinned_fp32"]), median(ms[name])
                print("%s against pinned fp32 of this run: %.2f ms against %.2f ms (x%.3f)" % (name.replace("_", " "), b, a, b / a), flush=True)

    torch.cuda.synchronize()
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
