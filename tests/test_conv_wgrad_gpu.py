"""The five convolution weight-gradient kernels (csrc/conv_wgrad.hip, csrc/conv_wgrad_stream.h) across their work splits,
through the C ABI (pnmn_conv_wgrad_cus, and pnmn_conv_wgrad once per path), against the float64 reference of
tests/wgrad_reference.py computed on the device with torch (independent of the library; tests/test_wgrad_reference.py
holds it against float64 autograd).

EXACT cases.  Inputs are small integers stored as float32 (x, dy in [-3, 3], masks in {0, 1, 2}, gates in
{-1, -0.0, 0, 1}; dw / dbias pre-filled with small integers): every product, every partial sum in any order and every
atomic add is exact in float32 as long as 18 * H * W * (items into one weight) < 2^24, which `exact_ok` asserts per
launch.  The comparison is torch.equal, so a unit visited twice, a 28-pixel stage dropped, a tap shifted by the wrong
dilation, a slab added into the neighbouring weight or a bias counted once per input slab shows as a whole number.  dw
and dbias live inside larger buffers whose other floats must stay untouched.

ROUND-OFF cases.  The data of tests/test_hip_kernels.py on a few launches per path, longest reductions included.  Per
tensor err = max|got - ref64| / max|ref64|; the bound is 4 * err32 + 2 * 2^-24 with err32 the same figure of float32 CPU
autograd on the same inputs: both are float32 sums of the same products in another order, the kernels chain their MFMA
accumulations over a whole job where the CPU blocks its sums, and every slab adds one atomic rounding per job.

Two kinds of launch exceed the factor 4 without a defect (their exact twins above pass); for those launches, at the map
sizes where they do (the set CHAINED) and nowhere else, the dw bound carries one more term, derived from the order of the
additions and computed from the inputs (wgrad_reference.chain_sigma):
  * one job of 600 items: the (job, slab) kernels keep ONE float32 accumulator per dW entry across the whole job --
    117 600 (14x14) or 470 400 (28x28) additions behind each other, each rounding a partial sum that has grown to the
    size of the result -- where the CPU sums in blocks.  The GEMM kernel cuts the job into one stage range per workgroup
    (three of 200 items at 14x14, where a one-job launch gets no more; fourteen at 28x28 without a budget, which stays
    under 4; four with cus = 2) and chains inside each;
  * 512 one-item jobs into one weight on the streamed kernel: 512 atomic additions per entry in free order put err
    between 3.4 and 4.6 err32.  (The GEMM kernel and the 28x28 band kernel stay under 4 on the same launch and are held
    to the plain bound.)
The term is six standard deviations of the round-off of the kernel's own chains: a job's items from zero for the (job,
slab) kernels; for the GEMM kernel the stage ranges of its split, restated in `gemm_chains`, piece by piece, in units of
a 28-pixel stage.  An addition rounds its partial sum S to nearest (variance ulp(S)^2 / 12, independent
between additions); the partial sums are the float64 reference's, never the kernel's.  Six because a tensor has 1.5e5
entries: a Gaussian tail of 2e-9 each, 3e-4 per tensor; the largest of 1.5e5 such errors is expected near 4.9.  One
rounding is counted per product, an upper count (an MFMA adds four products per accumulation; with one rounding per
MFMA the deviation would be half), and the measured errors sit at 1 to 3 of one such standard deviation.  dbias
stays at 4 * err32 + 2 * 2^-24 everywhere.

Measured err / err32 (MI355X; dw, dbias), and in brackets the dw bound in units of err32 where the chain term is in it:

    launch                                          14x14               28x28
    3x3, 5 items in 2 jobs                           0.75, 0.26          0.72, 0.35
    3x3, one job of 600 items                       35.38, 0.36 (155)   38.06, 0.40 (204)
    3x3, 512 one-item jobs into one weight           3.19, 1.11  (51)    2.12, 1.53
    3x3, stem (cin 1024), 12 items in 3 jobs         1.08, 0.35          2.25, 0.30
    classifier (cout 1024), 5 items in 2 jobs        0.73, 0.26          0.88, 0.36
    classifier (cout 512), 65 jobs of 0..6 items     2.50, 0.12          3.00, 0.06
    classifier (cout 256), one job of 600 items     22.29, 0.05 (107)    3.65, 0.02
    classifier, the same with cus = 2               22.74, 0.05 (107)    9.99, 0.05  (65)
    classifier (cout 512), 512 one-item jobs         3.52, 0.05          1.57, 0.02
    1x1 two sources, 65 jobs into one weight         2.32, 0.11          1.69, 0.07

(paths: 3x3 = conv_wgrad_stream_kernel at 14x14 and conv_wgrad_band_kernel<28,28,7,9> at 28x28; classifier =
conv_wgrad_1x1_gemm_kernel at both sizes; two sources = conv_wgrad_kernel<14,14,1> and conv_wgrad_band_kernel<28,28,7,1>.)

Run to run (test_rerun_report prints it): the atomics leave the order of the additions free.  With 512 one-item jobs
neither dw nor dbias repeats bit for bit (dw moves by about 1e-3 on entries of magnitude 1e3).  The classifier's
600-item job, where few workgroups add into an entry, may or may not repeat in dw; its dbias does not.

Every exact case prints the kernel the dispatch rule of pnmn_conv_wgrad_cus sends it to (`path_of`, a restatement); a
kernel trace of this file shows each of the five kernels launched as often as those lines say.
"""
import os

import numpy as np
import pytest
import torch

import wgrad_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64          # floats in front of and behind every dw / dbias
SENTINEL = 4242.0
BUDGETS = [0, 1, 2, 3, 7, 8, 13, 64, 100, 192, 256, 300, -5]
G1_MAX_JOBS = 512   # (csrc/conv_wgrad.hip)
G1_MAX_ITEMS, G1_PX = 256, 28


@pytest.fixture(scope="module")
def hip():
    from probnmn import _hip

    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a MI355X"
    return _hip


def dev():
    return torch.device("cuda:0")


def path_of(L):
    """The kernel pnmn_conv_wgrad_cus picks (its dispatch rule, restated)."""
    if L.taps == 1 and L.cin_blocks == 1 and L.cout_blocks % 2 == 0 and len(L.jobs) <= G1_MAX_JOBS:
        return "conv_wgrad_1x1_gemm_kernel"
    if L.H == 14:
        return "conv_wgrad_stream_kernel" if L.taps == 9 else "conv_wgrad_kernel<14,14,1>"
    return "conv_wgrad_band_kernel<28,28,7,%d>" % L.taps


def gemm_chains(L, cus):
    """launch_wgrad_1x1_gemm's split, restated: the stage ranges [r0, r1) of an output block's workgroups, and the stages at
    which an accumulator starts from zero in a launch of ONE weight (a range's start, and every piece of
    G1_MAX_ITEMS - 1 items' stages inside it)."""
    assert path_of(L) == "conv_wgrad_1x1_gemm_kernel"
    spi, n_cob = L.H * L.W // G1_PX, L.cout_blocks // 2
    default = int(os.environ.get("PNMN_CONV_CUS") or 256)
    default = (default & ~7) if 8 <= default <= 256 else 256
    budget = cus if 1 <= cus <= 256 else default
    wpc = max(1, min(2 * budget // n_cob, len(L.jobs) * spi // 2))
    total = sum(e - b for (b, e, _) in L.jobs) * spi
    ranges = [(total * w // wpc, total * (w + 1) // wpc) for w in range(wpc)]
    piece = (G1_MAX_ITEMS - 1) * spi
    starts = [t for (r0, r1) in ranges for t in range(r0, r1, piece)]
    return ranges, starts, spi


def exact_ok(L):
    most = max(len(L.items_of(k)) for k in range(L.n_weights))
    assert 18 * L.H * L.W * most + 8 < 2 ** 24, "the integer sums of this launch could round in float32"


class Uploaded:
    """The pools of a launch in device memory and its item records."""

    def __init__(self, hip, L):
        HW = L.H * L.W
        self.L = L
        if L.two_sources:
            assert L.cin_blocks == 2
            self.xa, self.xb = L.x_pool[:, :, :R.CB].contiguous().to(dev()), L.x_pool[:, :, R.CB:].contiguous().to(dev())
            self.x_stride = R.CB
        else:
            self.xa, self.xb = L.x_pool.to(dev()), None
            self.x_stride = L.cin
        self.m, self.dy, self.g = L.m_pool.to(dev()), L.dy_pool.to(dev()), L.g_pool.to(dev())
        self.dy_stride = L.cout
        items = np.zeros(L.n_items, hip.WGRAD_ITEM)
        u64 = np.uint64
        ix, idy, im = L.ix.astype(u64), L.idy.astype(u64), np.maximum(L.im, 0).astype(u64)
        items["x"] = u64(self.xa.data_ptr()) + ix * u64(4 * HW * self.x_stride)
        if self.xb is not None:
            items["x2"] = u64(self.xb.data_ptr()) + ix * u64(4 * HW * self.x_stride)
        items["xmask"] = np.where(L.im >= 0, u64(self.m.data_ptr()) + im * u64(4 * HW), u64(0))
        items["dy"] = u64(self.dy.data_ptr()) + idy * u64(4 * HW * self.dy_stride)
        items["gate"] = np.where(L.use_gate, u64(self.g.data_ptr()) + idy * u64(4 * HW * self.dy_stride), u64(0))
        items["dilation"] = L.dil
        self.items = items
        self.ibuf = hip.to_device(items, dev()) if L.n_items else torch.zeros(48, dtype=torch.uint8, device=dev())


def run(hip, up, cus, *, prefill, entry="cus"):
    """One launch.  Returns (dw per weight incl. the prefill, dbias per weight, prefill of dw, prefill of dbias) on the device."""
    L = up.L
    g = torch.Generator().manual_seed(99)
    n_dw = L.cout * L.taps * L.cin
    bufs, pre_w, pre_b = [], [], []
    jobs = np.zeros(len(L.jobs), hip.WGRAD_JOB)
    for k in range(L.n_weights):
        pw = torch.randint(-2, 3, (n_dw,), generator=g).float() if prefill else torch.zeros(n_dw)
        pb = torch.randint(-2, 3, (L.cout,), generator=g).float() if prefill else torch.zeros(L.cout)
        big_w = torch.full((n_dw + 2 * GUARD,), SENTINEL)
        big_b = torch.full((L.cout + 2 * GUARD,), SENTINEL)
        big_w[GUARD:GUARD + n_dw], big_b[GUARD:GUARD + L.cout] = pw, pb
        bufs.append((big_w.to(dev()), big_b.to(dev())))
        pre_w.append(pw.to(dev()))
        pre_b.append(pb.to(dev()))
    for j, (b, e, k) in enumerate(L.jobs):
        jobs[j]["dw"] = bufs[k][0].data_ptr() + 4 * GUARD
        jobs[j]["dbias"] = bufs[k][1].data_ptr() + 4 * GUARD if L.has_bias[k] else 0
        jobs[j]["item_begin"], jobs[j]["item_end"] = b, e
    jbuf = hip.to_device(jobs, dev())
    args = (up.ibuf.data_ptr(), jbuf.data_ptr(), len(L.jobs), L.H, L.W, L.taps, L.cin_blocks, L.cout_blocks, up.x_stride, up.dy_stride)
    if entry == "cus":
        hip.check(hip.lib().pnmn_conv_wgrad_cus(*args, cus, hip.stream_ptr(dev())), "wgrad (cus = %d)" % cus)
    else:
        hip.check(hip.lib().pnmn_conv_wgrad(*args, hip.stream_ptr(dev())), "wgrad")
    torch.cuda.synchronize()
    dws, dbs = [], []
    for k, (bw, bb) in enumerate(bufs):
        for what, big, n in (("dw", bw, n_dw), ("dbias", bb, L.cout)):
            assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all()), \
                "floats beside %s of weight %d were written" % (what, k)
        dws.append(bw[GUARD:GUARD + n_dw].reshape(L.cout, L.taps, L.cin))
        dbs.append(bb[GUARD:GUARD + L.cout])
    return dws, dbs, pre_w, pre_b


_REF = {}


def reference_of(name, L):
    name = (name, L.H)
    if name not in _REF:
        _REF[name] = R.reference(L, device=dev(), chunk=32 if L.cin * L.H <= 128 * 28 else 8)
    return _REF[name]


def assert_exact(L, got, ref, pre, what, k, where):
    want = ref + pre.reshape(ref.shape).double()
    if torch.equal(got.double(), want):
        return
    diff = (got.double() - want)
    bad = diff.nonzero()
    first = [tuple(int(v) for v in r) for r in bad[:6]]
    per_tap = (diff != 0).sum((0, 2)).tolist() if diff.dim() == 3 else []
    raise AssertionError("%s of weight %d differs (%s, %s): %d of %d entries, largest difference %g (reference magnitude %g), first at %s = %s; differing entries per tap %s"
                         % (what, k, path_of(L), where, len(bad), diff.numel(), float(diff.abs().max()), float(ref.abs().max()),
                            first, [float(diff[i]) for i in first], per_tap))


def check_exact(hip, name, L, budgets=(0,), entries=("cus",)):
    exact_ok(L)
    up = Uploaded(hip, L)
    ref_w, ref_b = reference_of(name, L)
    for entry in entries:
        for cus in (budgets if entry == "cus" else (0,)):
            dws, dbs, pre_w, pre_b = run(hip, up, cus, prefill=True, entry=entry)
            where = "cus = %d" % cus if entry == "cus" else "pnmn_conv_wgrad"
            for k in range(L.n_weights):
                assert_exact(L, dws[k], ref_w[k], pre_w[k], "dw", k, where)
                if L.has_bias[k]:
                    assert_exact(L, dbs[k], ref_b[k], pre_b[k], "dbias", k, where)
                else:
                    assert torch.equal(dbs[k], pre_b[k]), "dbias of weight %d (NULL in its jobs) was written" % k
    print("\n[path] %s %dx%d: %s (%d jobs, %d items)" % (name, L.H, L.W, path_of(L), len(L.jobs), L.n_items))


# ---------------------------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------------------------
def counts_0_6(rng, n_jobs):
    """Item counts drawn from 0..6; the first, the middle and the last job empty where there are at least seven."""
    c = rng.randint(0, 7, n_jobs)
    if n_jobs >= 7:
        c[0] = c[n_jobs // 2] = c[-1] = 0
        c[1] = 6
    else:
        c[c == 0] = 5
    return c


def weights_that_return(rng, n_jobs, n_weights):
    """Weights dealt to the jobs in an order that comes back to earlier ones (A, B, A, ...)."""
    w = rng.randint(0, n_weights, n_jobs)
    head = [0, 1, 0, 2, 3, 1, 0][:n_jobs] if n_weights == 4 else [0, 1, 0][:n_jobs]
    w[:len(head)] = head
    return w


DILS = (1, 2, 4, 8)


def launch_3x3(H, n_jobs, *, cin_blocks=1, cout_blocks=1, two_sources=False, seed=0, pools=None):
    rng = np.random.RandomState(1000 + n_jobs + seed)
    jd = rng.randint(0, 4, n_jobs)
    return R.make_launch(H, 9, cin_blocks, cout_blocks, counts_0_6(rng, n_jobs), weights_that_return(rng, n_jobs, 4),
                         lambda j, k: DILS[jd[j]], two_sources=two_sources, mask="some", gate="some", no_bias=(2,), seed=seed, pools=pools)


def launch_classifier(H, n_jobs, cout_blocks, maps, *, counts=None, seed=0, pools=None):
    rng = np.random.RandomState(2000 + n_jobs + cout_blocks)
    c = counts_0_6(rng, n_jobs) if counts is None else counts
    w = weights_that_return(rng, n_jobs, 2) if counts is None else [0] * n_jobs
    return R.make_launch(H, 1, 1, cout_blocks, c, w, 1, mask=maps, gate=maps, seed=seed, pools=pools)


def launch_two_sources(H, n_jobs, *, one_weight=False, seed=0, pools=None):
    rng = np.random.RandomState(3000 + n_jobs)
    w = [0] * n_jobs if one_weight else weights_that_return(rng, n_jobs, 2)
    return R.make_launch(H, 1, 2, 1, counts_0_6(rng, n_jobs), w, 1, two_sources=True, mask="some", gate="some", no_bias=(1,),
                         seed=seed, pools=pools)


SIZES = pytest.mark.parametrize("H", [14, 28], ids=["14x14", "28x28"])


@SIZES
@pytest.mark.parametrize("n_jobs", [1, 7, 8, 9, 65, 300])
def test_3x3_job_counts(hip, H, n_jobs):
    """Empty jobs first / in the middle / last, fewer jobs than XCDs, job counts that are no multiple of 8, four weights
    in an order that returns to earlier ones, one of them without a bias, a dilation per job."""
    check_exact(hip, "3x3 %d jobs" % n_jobs, launch_3x3(H, n_jobs))


@SIZES
def test_3x3_only_empty_jobs(hip, H):
    L = R.make_launch(H, 9, 1, 1, [0, 0, 0], [0, 1, 0], 1)
    check_exact(hip, "3x3 empty", L, budgets=(0, 2))


@SIZES
def test_3x3_one_long_job(hip, H):
    L = R.make_launch(H, 9, 1, 1, [3, 600, 2], [1, 0, 1], lambda j, k: DILS[(j + 1) % 4], mask="some", gate="some")
    check_exact(hip, "3x3 600 items", L)


@SIZES
def test_3x3_many_one_item_jobs(hip, H):
    rng = np.random.RandomState(7)
    jd = rng.randint(0, 4, 600)
    L = R.make_launch(H, 9, 1, 1, [1] * 600, weights_that_return(rng, 600, 4), lambda j, k: DILS[jd[j]], mask="some", gate="some",
                      no_bias=(2,))
    check_exact(hip, "3x3 600 jobs", L)


@SIZES
@pytest.mark.parametrize("shape", ["stem", "x2", "cout4"])
def test_3x3_wide_shapes(hip, H, shape):
    """cin_blocks = 8 at x_stride = 1024 (the stem), cin_blocks = 2 through the second source, cout_blocks = 4 at
    dy_stride = 512."""
    if shape == "stem":
        L = launch_3x3(H, 9, cin_blocks=8, seed=1)
    elif shape == "x2":
        L = launch_3x3(H, 9, cin_blocks=2, two_sources=True, seed=2)
    else:
        L = launch_3x3(H, 9, cout_blocks=4, seed=3)
    check_exact(hip, "3x3 " + shape, L)


@SIZES
@pytest.mark.parametrize("dilation", DILS)
def test_3x3_uniform_dilation(hip, H, dilation):
    L = R.make_launch(H, 9, 1, 1, [3, 1, 0, 4, 2], [0, 1, 0, 1, 0], dilation, mask="some", gate="some", seed=dilation)
    check_exact(hip, "3x3 dilation %d" % dilation, L)


MIXED = ([1, 2, 4, 8], [8, 1], [1, 1, 8, 8, 1])


@SIZES
def test_3x3_dilations_mixed_inside_jobs(hip, H):
    """Every item carries its own dilation (include/probnmn_hip.h): the orders 1,2,4,8 / 8,1 / 1,1,8,8,1 inside jobs, three
    times over so that a persistent workgroup meets them behind each other."""
    orders = MIXED * 3
    L = R.make_launch(H, 9, 1, 1, [len(o) for o in orders], [0, 1, 0, 1, 1, 0, 0, 0, 1], lambda j, k: orders[j][k], mask="some",
                      gate="some", seed=11)
    check_exact(hip, "3x3 mixed dilations", L, budgets=(0, 1, 3))


@SIZES
@pytest.mark.parametrize("n_jobs,cout_blocks", [(1, 2), (1, 4), (1, 8), (3, 2), (3, 4), (3, 8), (65, 2), (65, 4), (65, 8), (512, 2), (512, 4),
                                                (512, 8), (513, 2), (513, 4), (513, 8)])
def test_classifier_job_counts(hip, H, n_jobs, cout_blocks):
    """1x1 over one input block: the GEMM kernel's stage ranges over jobs of 0..6 items adding into weights A, B, A, ...;
    513 jobs: past the kernel's job table, the launch falls back to the (job, slab) kernels.  Gate and mask present on
    every other case, absent on the others."""
    maps = (n_jobs + cout_blocks // 2) % 2 == 0
    check_exact(hip, "classifier %d jobs x %d" % (n_jobs, cout_blocks), launch_classifier(H, n_jobs, cout_blocks, maps))


PIECES = {"300 items": (4, [300], [0]), "600 items": (4, [2, 600, 1], [0, 0, 0]), "600 items x 8": (8, [600], [0]),
          "weights change": (4, [200, 0, 100, 300, 0, 40], [0, 0, 1, 0, 1, 1])}


@SIZES
@pytest.mark.parametrize("case", sorted(PIECES))
def test_classifier_piece_loop(hip, H, case):
    """cus = 1 at cout_blocks >= 4 leaves ONE workgroup per output block (2 * cus / (cout_blocks / 2) <= 1), which then owns
    more item records than its LDS table holds (255): the range goes in pieces -- two for 300 items, three for 600; in
    "weights change" the pieces end inside jobs of a range that goes from weight A to B and back, past empty jobs."""
    cout_blocks, counts, weights = PIECES[case]
    L = R.make_launch(H, 1, 1, cout_blocks, counts, weights, 1, mask="some", gate="some", seed=21)
    ranges, _, spi = gemm_chains(L, 1)
    assert len(ranges) == 1 and ranges[0][1] - ranges[0][0] > (G1_MAX_ITEMS - 1) * spi, "the launch no longer reaches the piece loop"
    check_exact(hip, "classifier pieces " + case, L, budgets=(1,))


@SIZES
def test_classifier_only_empty_jobs(hip, H):
    check_exact(hip, "classifier empty", launch_classifier(H, 4, 4, True, counts=[0, 0, 0, 0]), budgets=(0, 1))


@SIZES
@pytest.mark.parametrize("n_jobs", [1, 9, 65])
def test_1x1_two_sources(hip, H, n_jobs):
    check_exact(hip, "two sources %d jobs" % n_jobs, launch_two_sources(H, n_jobs))


@SIZES
@pytest.mark.parametrize("path", ["3x3", "classifier", "classifier fallback", "two sources"])
def test_budgets(hip, H, path):
    """Every budget, sensible or not, changes the split and never the sums; pnmn_conv_wgrad is the budget 0."""
    if path == "3x3":
        L = launch_3x3(H, 65, seed=5)
    elif path == "classifier":
        L = launch_classifier(H, 65, 4, True, seed=5)
    elif path == "classifier fallback":
        L = R.make_launch(H, 1, 1, 2, [1] * 513, [0, 1, 0] * 171, 1, mask="some", gate="some", seed=5)
    else:
        L = launch_two_sources(H, 9, seed=5)
    check_exact(hip, "budgets " + path, L, budgets=BUDGETS, entries=("cus", "plain"))


# ---------------------------------------------------------------------------------------------------------------------
# round-off
# ---------------------------------------------------------------------------------------------------------------------
def roundoff_launch(name, H):
    np_ = lambda taps, cin, cout, seed: R.normal_pools(seed, H, H, taps, cin, cout)  # noqa: E731
    if name == "3x3 5 items":
        return R.make_launch(H, 9, 1, 1, [3, 2], [0, 0], 2, pools=np_(9, 128, 128, 1)), 0
    if name == "3x3 600 items":
        return R.make_launch(H, 9, 1, 1, [600], [0], 1, pools=np_(9, 128, 128, 2)), 0
    if name == "3x3 512 jobs":
        return R.make_launch(H, 9, 1, 1, [1] * 512, [0] * 512, lambda j, k: DILS[j % 4], pools=np_(9, 128, 128, 3)), 0
    if name == "3x3 stem":
        return R.make_launch(H, 9, 8, 1, [5, 4, 3], [0, 0, 0], 1, pools=np_(9, 1024, 128, 4)), 0
    if name == "classifier 5 items":
        return R.make_launch(H, 1, 1, 8, [3, 2], [0, 0], 1, pools=np_(1, 128, 1024, 8)), 0
    if name == "classifier 65 jobs":
        rng = np.random.RandomState(65)
        return R.make_launch(H, 1, 1, 4, counts_0_6(rng, 65), [0] * 65, 1, mask="some", gate="some", pools=np_(1, 128, 512, 9)), 0
    if name == "classifier 600 items":
        return R.make_launch(H, 1, 1, 2, [600], [0], 1, pools=np_(1, 128, 256, 5)), 0
    if name == "classifier 600 items cus 2":
        return R.make_launch(H, 1, 1, 2, [600], [0], 1, pools=np_(1, 128, 256, 5)), 2
    if name == "classifier 512 jobs":
        return R.make_launch(H, 1, 1, 4, [1] * 512, [0] * 512, 1, mask=False, gate=False, pools=np_(1, 128, 512, 6)), 0
    assert name == "two sources 65 jobs"
    return launch_two_sources(H, 65, one_weight=True, pools=np_(1, 256, 128, 7)), 0


def rel_err(got, ref):
    return float((got.double().cpu() - ref.cpu()).abs().max()) / float(ref.abs().max())


# (launch, map size) whose dw exceeds 4 err32 without a defect: the chain term applies to these and to no other
CHAINED = {("3x3 600 items", 14), ("3x3 600 items", 28), ("3x3 512 jobs", 14), ("classifier 600 items", 14),
           ("classifier 600 items cus 2", 14), ("classifier 600 items cus 2", 28)}


def roundoff_bounds(L, name, cus, ref_w, err32_w, err32_b):
    """(bound of dw, bound of dbias): 4 err32 + 2 * 2^-24; for the launches in CHAINED dw gets six standard deviations of the
    round-off of the kernel's own chains of additions on top (wgrad_reference.chain_sigma): a job's items from zero in
    the (job, slab) kernels; the stage ranges of the restated split, piece by piece, in the GEMM kernel."""
    bw, bb = 4 * err32_w + 2 * R.U32, 4 * err32_b + 2 * R.U32
    if (name, L.H) in CHAINED:
        if path_of(L) == "conv_wgrad_1x1_gemm_kernel":
            _, starts, _ = gemm_chains(L, cus)
            sigma = R.chain_sigma(L, 0, device=dev(), unit_px=G1_PX, chain_starts=starts)
        else:
            sigma = R.chain_sigma(L, 0, device=dev())
        bw += 6 * sigma / float(ref_w.abs().max())
    return bw, bb


@SIZES
@pytest.mark.parametrize("name", ["3x3 5 items", "3x3 600 items", "3x3 512 jobs", "3x3 stem", "classifier 5 items",
                                  "classifier 65 jobs", "classifier 600 items", "classifier 600 items cus 2",
                                  "classifier 512 jobs", "two sources 65 jobs"])
def test_roundoff(hip, H, name):
    L, cus = roundoff_launch(name, H)
    ref_w, ref_b = R.reference(L, device=dev(), chunk=32 if L.cin == 128 else 4)
    cpu_w, cpu_b = R.autograd_wgrad(L, torch.float32)
    dws, dbs, _, _ = run(hip, Uploaded(hip, L), cus, prefill=False)
    err32_w, err32_b = rel_err(cpu_w[0], ref_w[0]), rel_err(cpu_b[0], ref_b[0])
    bound_w, bound_b = roundoff_bounds(L, name, cus, ref_w[0], err32_w, err32_b)
    line = "[roundoff] %s %dx%d (%s):" % (name, H, H, path_of(L))
    fails = []
    for what, got, ref, err32, bound in (("dw", dws[0], ref_w[0], err32_w, bound_w), ("dbias", dbs[0], ref_b[0], err32_b, bound_b)):
        if what == "dbias" and not L.has_bias[0]:
            continue
        err = rel_err(got, ref)
        line += " %s err %.2e err32 %.2e ratio %.2f bound %.2e;" % (what, err, err32, err / err32, bound)
        if not err <= bound:
            fails.append((what, err, bound))
    print("\n" + line)
    assert not fails, line


@SIZES
def test_rerun_report(hip, H):
    """Atomics leave the order of the additions free: two launches run twice, bit-equality REPORTED (not asserted); both
    runs are within the round-off bound through test_roundoff's launches."""
    for name in ("3x3 512 jobs", "classifier 600 items"):
        L, cus = roundoff_launch(name, H)
        up = Uploaded(hip, L)
        a = run(hip, up, cus, prefill=False)
        b = run(hip, up, cus, prefill=False)
        same_w, same_b = torch.equal(a[0][0], b[0][0]), torch.equal(a[1][0], b[1][0])
        print("\n[rerun] %s %dx%d (%s): dw bit-equal %s (max diff %.2e), dbias bit-equal %s"
              % (name, H, H, path_of(L), same_w, float((a[0][0] - b[0][0]).abs().max()), same_b))
        assert torch.isfinite(a[0][0]).all() and torch.isfinite(b[0][0]).all()
