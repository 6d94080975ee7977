"""8-bit feature stores: rows kept as torch.float8_e4m3fn / torch.float8_e5m2 -- page-locked on the host
(PinnedFeatureStore) or in HBM (DeviceFeatureStore) -- widened to fp32 by the kernels that read them
(pnmn_gather_features_typed, pnmn_expand_rows) and rounded by the ones that fill them (the gather's write-out,
pnmn_narrow_rows).  What the networks see is exactly ``features.to(dtype).float()``: every comparison here is BITWISE
(integer views), against torch's own host conversion; only NaNs (which the every-code test meets) are compared as NaNs.
The reference keeps float64 rows in HDF5 and casts per item (readers.py:63-108, datasets.py:137-142)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
FP8 = [E4M3, E5M2]
CODE = {E4M3: 4, E5M2: 5}


@functools.lru_cache(maxsize=None)
def edge_table(dtype) -> torch.Tensor:
    """fp32 values at which the rounding to ``dtype`` can go wrong, none of which overflows: for every pair of adjacent
    finite non-negative codes the midpoint (a tie) and its fp32 neighbours on either side; zero, the smallest subnormal
    and half of it (a tie that goes to zero); the largest value and the largest that still rounds to it; all with both signs."""
    values = torch.arange(128, dtype=torch.uint8).view(dtype).float()
    values = values[torch.isfinite(values)]  # the non-negative finite codes' values, ascending: 127 (e4m3fn) or 124 (e5m2)
    mid = ((values[:-1].double() + values[1:].double()) / 2).float()  # (one more mantissa bit than the codes have: exact)
    assert bool((mid.double() * 2 == values[:-1].double() + values[1:].double()).all())
    smallest = float(values[1])
    top = [448.0, 464.0] if dtype == E4M3 else [57344.0, 61439.9]
    assert float(values[-1]) == top[0] and smallest == (2.0 ** -9 if dtype == E4M3 else 2.0 ** -16)
    table = torch.cat([mid, torch.nextafter(mid, torch.zeros_like(mid)), torch.nextafter(mid, torch.full_like(mid, float("inf"))),
                       torch.tensor([0.0, smallest, smallest / 2] + top, dtype=torch.float32)])
    table = torch.cat([table, -table])
    assert 700 < table.numel() < 800 and bool(torch.isfinite(table.to(dtype).float()).all())
    return table


@functools.lru_cache(maxsize=None)
def features(shape, dtype, seed=0):
    """Seeded relu(randn) of ``shape`` (N, C, H, W), fp32, with the edge table of ``dtype`` in it (as much of it as a row
    holds) -- at the start of every other row (so from channel 0 on) and, flipped, at its end (up to the last channel: a
    channel tail where there is one)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.relu(torch.randn(shape, generator=g))
    flat = feats.view(shape[0], -1)
    table = edge_table(dtype)
    k = min(table.numel(), flat.size(1))
    for r in range(0, shape[0], 2):
        flat[r, :k] = table[:k]
        flat[r, -k:] = table[:k].flip(0)
    return feats


@functools.lru_cache(maxsize=None)
def quantised(shape, dtype, seed=0):
    """The reference: torch's host conversion of the same features, widened again (exact)."""
    q = torch.from_numpy(features(shape, dtype, seed).numpy()).to(dtype).float()
    assert bool(torch.isfinite(q).all())
    return q


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def same_bits_or_nan(got: torch.Tensor, want: torch.Tensor) -> bool:
    got, want = got.detach().cpu().contiguous(), want.contiguous()
    nan = torch.isnan(want)
    return got.shape == want.shape and torch.equal(torch.isnan(got), nan) and \
        torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


def pinned_around(raw: torch.Tensor, shape, dtype):
    """A pinned store put together around ``store`` and ``shape`` alone (the gather takes the element type from the tensor)."""
    from probnmn.data.feature_store import PinnedFeatureStore

    store = PinnedFeatureStore.__new__(PinnedFeatureStore)
    store.shape, store.store = shape, raw.view(shape).pin_memory().view(dtype)
    return store


# (4, 8, 4, 4): rows of 128 bytes, one 16-byte aligned run each, and 128 elements per resident row: the 16-byte paths of
# the gather and of pnmn_expand_rows.  (4, 7, 3, 3) and (5, 7, 3, 3): rows of 63 bytes, the 1-byte path of the gather and
# the element-by-element one of pnmn_expand_rows; the first holds 252 bytes, codes 0 .. 251 only, the second all of them.
@pytest.mark.parametrize("dtype", FP8)
@pytest.mark.parametrize("shape", [(4, 8, 4, 4), (4, 7, 3, 3), (5, 7, 3, 3)])
def test_every_code_widens_exactly(shape, dtype):
    """All 256 codes -- subnormals, both zeros, the infinities of e5m2, the NaNs -- through the pinned gather and through
    the resident rows' widening, against torch's own ``.float()`` of the same bytes.  A conversion that took the codes for
    another 8-bit flavour (fnuz: bias 8, one NaN, no negative zero) fails here."""
    from probnmn.data.feature_store import DeviceFeatureStore

    N, C, H, W = shape
    raw = (torch.arange(N * C * H * W) % 256).to(torch.uint8)
    assert shape == (4, 7, 3, 3) or raw.unique().numel() == 256
    value = torch.arange(256, dtype=torch.uint8).view(dtype).float()  # what every code is
    assert int(torch.isnan(value).sum()) == (2 if dtype == E4M3 else 6) and int(torch.isinf(value).sum()) == (0 if dtype == E4M3 else 2)
    want = value[raw.long()]
    store = pinned_around(raw, shape, dtype)
    got = store.gather(torch.arange(N), DEV)
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    assert same_bits_or_nan(got, want.view(shape))
    there = raw.view(N, H, W, C).to(DEV).view(dtype).permute(0, 3, 1, 2)  # the same bytes as NHWC rows
    resident = DeviceFeatureStore.from_device(there)
    assert resident.dtype == dtype and resident.row_bytes == C * H * W and resident.data_ptr() == there.data_ptr()
    got = resident.batch(torch.arange(N)).materialize()
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert same_bits_or_nan(got, want.view(N, H, W, C).permute(0, 3, 1, 2))


# (9, 72, 14, 14): rows of 14 112 elements hold the whole table twice; chunks of 4, 4 and 1 rows; write_rows of 70 560 and
# 56 448 elements: 16 bytes read per thread and turn.  (6, 7, 3, 3): rows of 63 elements; write_rows of 189 elements at
# row 0 (vectors and a tail of one) and of 189 at byte 189 (no alignment: element by element).
@pytest.mark.parametrize("dtype", FP8)
@pytest.mark.parametrize("shape, split", [((9, 72, 14, 14), 5), ((6, 7, 3, 3), 3)])
def test_narrowing_is_torchs_rounding(shape, split, dtype):
    from probnmn.data.feature_store import DeviceFeatureStore, ResidentRows

    N, C, H, W = shape
    feats = features(shape, dtype)
    host = feats.to(dtype)
    assert bool(torch.isfinite(host.float()).all())
    if C * H * W >= 2 * edge_table(dtype).numel():
        assert same_bits(host.view(N, -1)[0, : edge_table(dtype).numel()], edge_table(dtype).to(dtype))
    nhwc = host.permute(0, 2, 3, 1).contiguous()
    store = DeviceFeatureStore(feats.numpy(), DEV, chunk_rows=4, dtype=dtype)
    assert store.rows.dtype == dtype == store.dtype and tuple(store.rows.shape) == (N, H, W, C)
    assert store.row_bytes == C * H * W and len(store) == N and store.overflowed() == 0
    assert same_bits(store.rows, nhwc)
    idx = torch.tensor([N - 1, 0, 3, N - 1, 1, 3])
    rows = store.batch(idx)
    assert isinstance(rows, ResidentRows) and rows.shape == (6, C, H, W) and rows.is_cuda
    got = rows.materialize()
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    assert same_bits(got, quantised(shape, dtype)[idx])
    with pytest.raises(TypeError):
        rows.pointers()
    # filled chunk by chunk from device tensors: fp32 chunks (rounded by pnmn_narrow_rows) ...
    filled = DeviceFeatureStore.empty(N, (C, H, W), DEV, dtype)
    assert filled.dtype == dtype and filled.row_bytes == store.row_bytes and filled.image_feature_size == (C, H, W)
    filled.write_rows(0, feats[:split].to(DEV).contiguous(memory_format=torch.channels_last))
    filled.write_rows(split, feats[split:].to(DEV))  # (NCHW storage: the store lays it out)
    assert same_bits(filled.rows, nhwc) and filled.overflowed() == 0
    # ... and chunks already in the store's dtype
    filled = DeviceFeatureStore.empty(N, (C, H, W), DEV, dtype)
    filled.write_rows(split, host[split:].to(DEV).contiguous(memory_format=torch.channels_last))
    filled.write_rows(0, host[:split].to(DEV))
    assert same_bits(filled.rows, nhwc) and filled.overflowed() == 0
    with pytest.raises(IndexError):
        filled.write_rows(N - 1, feats[:2].to(DEV))
    with pytest.raises(ValueError):
        filled.write_rows(0, feats[:2].half().to(DEV))


# Which loads of the gather each shape takes at ONE byte per element (a pinned store starts page aligned; an item whose
# whole map fits the tile, HW <= 400, is ONE run of (channels of the block) x HW bytes, the block 256 / 128 / 64 channels
# for HW <= 100 / 200 / 400):
#   (9, 72, 14, 14)  one block of 72 channels: runs of 14 112 bytes, rows as far apart: 16-byte loads
#   (5, 64, 28, 28)  HW = 784 > 400: pixel ranges of 400 and 384, read channel by channel (stride 784): 16-byte loads
#   (3, 136, 5, 4)   one block of 136 channels, 2 720 bytes: 16-byte loads
#   (6, 8, 3, 3)     runs of 72 bytes, rows 72 bytes apart: 8-byte loads
#   (6, 7, 3, 3)     runs of 63 bytes: 1-byte loads, one run
#   (4, 65, 14, 14)  one block of 65 channels: runs of 12 740 bytes, 4 mod 8: 4-byte loads
#   (3, 8, 15, 15)   HW = 225: runs of 1 800 bytes, 8 mod 16: 8-byte loads
#   (3, 8, 18, 12)   runs of 1 728 bytes: 16-byte loads
#   (3, 8, 17, 12)   runs of 1 632 bytes: 16-byte loads
#   (3, 8, 21, 21)   HW = 441 > 400, odd: ranges of 400 and 41 pixels, 1-byte loads channel by channel (tile rows of 400)
#   (3, 8, 21, 20)   HW = 420 > 400, a multiple of 4 only: ranges of 400 and 20, 4-byte loads channel by channel
#   (3, 8, 24, 17)   HW = 408 > 400, a multiple of 8 only: ranges of 400 and 8, 8-byte loads channel by channel
#   (3, 130, 14, 14) blocks of 128 channels (25 088 bytes; rows are 25 480 bytes apart, 8 mod 16: 16-byte loads in even
#                    rows, 8-byte loads in odd ones) and a 2-channel tail of 392 bytes: 8-byte loads
#   (3, 66, 15, 15)  HW = 225: blocks of 64 channels (14 400 bytes: 16-byte loads in even rows, rows being 14 850 bytes
#                    apart, 2-byte aligned: 1-byte loads in odd ones) and a 2-channel tail of 450 bytes: 1-byte loads
#   (3, 260, 5, 4)   blocks of 256 channels and a 4-channel tail of 80 bytes: 16-byte loads
GATHER_SHAPES = [(9, 72, 14, 14), (5, 64, 28, 28), (3, 136, 5, 4), (6, 8, 3, 3), (6, 7, 3, 3), (4, 65, 14, 14), (3, 8, 15, 15),
                 (3, 8, 18, 12), (3, 8, 17, 12), (3, 8, 21, 21), (3, 8, 21, 20), (3, 8, 24, 17), (3, 130, 14, 14), (3, 66, 15, 15),
                 (3, 260, 5, 4)]


@pytest.mark.parametrize("dtype", FP8)
@pytest.mark.parametrize("shape", GATHER_SHAPES)
def test_gather_from_an_8bit_pinned_store_is_exact(shape, dtype):
    from probnmn.data.feature_store import PinnedFeatureStore

    feats = features(shape, dtype).numpy()
    N = shape[0]
    store = PinnedFeatureStore(feats, chunk_rows=4, dtype=dtype)
    assert store.store.dtype == dtype and store.store.is_pinned() and tuple(store.store.shape) == shape
    assert same_bits(store.store, torch.from_numpy(feats).to(dtype))
    idx = torch.tensor([N - 1, 0, 2, N - 1, 1, 2, 0])  # repeated, out of order
    want = quantised(shape, dtype)[idx]
    for index in (idx, idx.to(DEV)):  # from the host (validated there) and already on the device
        got = store.gather(index, DEV)
        assert got.dtype == torch.float32 and tuple(got.shape) == (7,) + shape[1:]
        assert got.is_contiguous(memory_format=torch.channels_last)
        assert same_bits(got, want)
    with pytest.raises(IndexError):
        store.gather(torch.tensor([0, N]), DEV)
    with pytest.raises(ValueError):
        store.copy_rows(idx, DEV)  # (the copy engines cannot widen)


@pytest.mark.parametrize("dtype", FP8)
def test_expand_rows_element_by_element_and_out_of_range(dtype):
    """Rows of 72 and of 45 elements: no multiple of the 16 elements of a load, so element by element; rows of 16 384
    elements: 16-byte loads, exactly one work item per row; rows of 16 640 and of 16 407: a second work item per row, with
    and without 16-byte loads.  An index outside the store reads row 0 (the gather's rule)."""
    from probnmn import _hip
    from probnmn.data.feature_store import DeviceFeatureStore

    for shape in [(7, 8, 3, 3), (7, 5, 3, 3), (3, 1024, 4, 4), (3, 1040, 4, 4), (3, 1823, 3, 3)]:
        feats = features(shape, dtype)
        store = DeviceFeatureStore(feats.numpy(), DEV, dtype=dtype)
        idx = torch.tensor([6 % shape[0], 0, 2, 2])
        assert same_bits(store.batch(idx).materialize(), quantised(shape, dtype)[idx])
        raw = torch.tensor([1, shape[0], -1], dtype=torch.long, device=DEV)
        out = torch.empty((3,) + shape[1:], dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
        elems = shape[1] * shape[2] * shape[3]
        _hip.check(_hip.lib().pnmn_expand_rows(store.data_ptr(), CODE[dtype], raw.data_ptr(), out.data_ptr(), 3, shape[0], elems,
                                               _hip.stream_ptr(DEV)), "expand_rows")
        assert same_bits(out, quantised(shape, dtype)[[1, 0, 0]])


def test_overflow_is_refused_where_the_8bit_type_has_no_such_value():
    from probnmn.data.feature_store import DeviceFeatureStore, PinnedFeatureStore

    shape = (6, 8, 3, 3)
    feats = features(shape, E4M3).numpy().copy()
    builds = (lambda **kw: PinnedFeatureStore(feats, chunk_rows=4, **kw), lambda **kw: DeviceFeatureStore(feats, DEV, chunk_rows=4, **kw))
    feats[4, 3, 1, 1] = 464.5  # beyond the tie above the largest e4m3fn: NaN there
    for build in builds:
        with pytest.raises(OverflowError) as e:
            build(dtype=E4M3)
        assert "row 4" in str(e.value) and "NaN" in str(e.value)
        build(dtype=E5M2)
        build()
    feats[4, 3, 1, 1] = 464.0  # the tie goes to even: 448
    assert float(PinnedFeatureStore(feats, chunk_rows=4, dtype=E4M3).store[4, 3, 1, 1].float()) == 448.0
    resident = DeviceFeatureStore(feats, DEV, chunk_rows=4, dtype=E4M3)
    assert float(resident.rows[4, 1, 1, 3].float()) == 448.0
    assert same_bits(resident.rows, torch.from_numpy(feats).to(E4M3).permute(0, 2, 3, 1).contiguous())
    feats[4, 3, 1, 1] = 61440.0  # the smallest value that e5m2 rounds to infinity
    for build in builds:
        with pytest.raises(OverflowError) as e:
            build(dtype=E5M2)
        assert "row 4" in str(e.value)
    feats[4, 3, 1, 1] = 1.0
    feats[1, 0, 0, 0] = np.inf  # an infinity of the source is the source's business
    assert bool(torch.isinf(PinnedFeatureStore(feats, dtype=E5M2).store[1, 0, 0, 0].float()))
    assert bool(torch.isnan(PinnedFeatureStore(feats, dtype=E4M3).store[1, 0, 0, 0].float()))


@pytest.mark.parametrize("dtype, beyond", [(E4M3, [464.5, -1e6]), (E5M2, [-61440.0, 3e38])])
def test_write_rows_counts_what_it_could_not_keep_finite(dtype, beyond):
    """write_rows cannot raise without waiting for the device; an 8-bit store counts instead.  An infinity or a NaN of
    the source is not counted."""
    from probnmn.data.feature_store import DeviceFeatureStore

    shape = (6, 8, 3, 3)
    feats = features(shape, dtype)
    store = DeviceFeatureStore.empty(6, shape[1:], DEV, dtype)
    assert store.overflowed() == 0  # a fresh store
    chunk = feats[:4].clone()
    chunk[1, 2, 0, 1], chunk[3, 7, 2, 2] = beyond
    chunk[0, 0, 0, 0], chunk[2, 5, 1, 1], chunk[2, 5, 1, 2] = float("inf"), float("-inf"), float("nan")
    store.write_rows(0, chunk.to(DEV).contiguous(memory_format=torch.channels_last))
    assert store.overflowed() == 2
    want = chunk.to(dtype).permute(0, 2, 3, 1).contiguous()
    assert int((~torch.isfinite(want.float())).sum()) == 5
    assert same_bits_or_nan(store.rows[:4].cpu().float(), want.float())  # (widened on the host)
    store.write_rows(4, feats[4:].to(DEV))  # a clean chunk
    assert store.overflowed() == 2
    store.write_rows(0, feats[:4].to(dtype).to(DEV))  # a chunk in the store's dtype is taken as it is
    assert store.overflowed() == 2
    assert same_bits(store.rows, feats.to(dtype).permute(0, 2, 3, 1).contiguous())
    assert DeviceFeatureStore.empty(2, shape[1:], DEV, dtype).overflowed() == 0
    with pytest.raises(TypeError):
        DeviceFeatureStore.empty(2, shape[1:], DEV, torch.float16).overflowed()  # (only an 8-bit store counts)


def test_the_library_refuses_other_element_pairs():
    from probnmn import _hip

    assert (_hip.ELEM_F8E4M3, _hip.ELEM_F8E5M2) == (4, 5)
    lib = _hip.lib()
    src = torch.zeros(2 * 8 * 4, dtype=torch.float32, device=DEV)
    dst = torch.zeros(2 * 8 * 4, dtype=torch.float32, device=DEV)
    idx = torch.zeros(2, dtype=torch.long, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = _hip.stream_ptr(DEV)
    pairs = [(4, 4), (4, 5), (5, 4), (5, 5)] + [(a, b) for a in (4, 5) for b in (1, 2)] + [(b, a) for a in (4, 5) for b in (1, 2)]
    for s, d in pairs + [(3, 0), (0, 3), (3, 4), (5, 3), (6, 0), (0, 6)]:
        assert lib.pnmn_gather_features_typed(src.data_ptr(), s, idx.data_ptr(), dst.data_ptr(), d, 2, 2, 8, 4, st) == _hip.EINVAL, (s, d)
    for s in (0, 3, 6, -1):
        assert lib.pnmn_expand_rows(src.data_ptr(), s, idx.data_ptr(), dst.data_ptr(), 2, 2, 32, st) == _hip.EINVAL
    for d in (0, 1, 2, 3, 6, -1):
        assert lib.pnmn_narrow_rows(src.data_ptr(), dst.data_ptr(), d, 64, count.data_ptr(), st) == _hip.EINVAL
    assert lib.pnmn_narrow_rows(src.data_ptr(), dst.data_ptr(), 4, 64, 0, st) == _hip.EINVAL  # (no counter)
    torch.cuda.synchronize()
    assert int(count) == 0 and not bool(dst.any())


def test_the_network_sees_exactly_the_quantised_features():
    """A module-training step and a joint-training step fed with rows of an e4m3fn resident store against the same steps
    fed with the tensor ``feats.to(dtype).float()[idx]``: the same losses, objective and sampled programs (bit-equal
    forward pass) and the same gradients up to the order of the weight gradients' atomic adds -- the bar, models, shapes
    and indices of tests/test_feature_store_half_gpu.py.  The module step once more from the e4m3fn pinned store's gather."""
    from probnmn.data.feature_store import DeviceFeatureStore, PinnedFeatureStore
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.trainers.joint_training import JointTrainingStep
    from probnmn.trainers.module_training import ModuleTrainingStep
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    shape, dtype = (23, 1024, 14, 14), E4M3
    feats = features(shape, dtype, seed=5)
    idx = torch.tensor([3, 22, 3, 0, 17, 9, 9, 21, 1, 14, 6, 2])
    store8 = DeviceFeatureStore(feats.numpy(), DEV, chunk_rows=7, dtype=dtype)
    want = quantised(shape, dtype, seed=5)[idx]
    assert same_bits(store8.batch(idx).materialize(), want)
    batch = synthetic_batch(vocab, 12, seed=8)

    def module_step(image):
        torch.manual_seed(0)
        net = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64).to(DEV)
        step = ModuleTrainingStep(net, lr=1e-4, report_metrics=False)
        b = {k: (v.to(DEV) if k != "program" else v) for k, v in batch.items() if k != "image"}
        b["image"] = image
        out = step.step(b)
        torch.cuda.synchronize()
        return out["loss"].detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    def close(g_t, g_r):
        assert sorted(g_t) == sorted(g_r)
        for k in g_t:
            assert float((g_t[k] - g_r[k]).abs().max()) <= 1e-4 * (float(g_t[k].abs().max()) + 1e-12), k

    loss_t, grads_t = module_step(want.to(DEV))
    loss_r, grads_r = module_step(store8.batch(idx))
    assert torch.equal(loss_t, loss_r)
    close(grads_t, grads_r)
    pinned8 = PinnedFeatureStore(feats.numpy(), dtype=dtype)
    loss_p, grads_p = module_step(pinned8.gather(idx, DEV))
    assert torch.equal(loss_t, loss_p)
    close(grads_t, grads_p)

    def joint_step(image):
        torch.manual_seed(1)
        pg, qr = ProgramGenerator(vocab).to(DEV), QuestionReconstructor(vocab).to(DEV)
        prior = ProgramPrior(vocab, hidden_size=256).to(DEV)
        net = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=64).to(DEV)
        step = JointTrainingStep(pg, qr, prior, net, objective="ours", alpha=100.0, beta=0.1, gamma=1.0, delta=0.99, lr=1e-4)
        b = {k: v.to(DEV) for k, v in batch.items() if k != "image"}
        b["supervision"] = batch["supervision"]
        b["image"] = image
        out = step.step(b)
        torch.cuda.synchronize()
        return float(out["objective"]), out["programs"].cpu(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    obj_t, z_t, g_t = joint_step(want.to(DEV))
    obj_r, z_r, g_r = joint_step(store8.batch(idx))  # (the step takes its unsupervised subset, then widens only that)
    assert torch.equal(z_t, z_r) and obj_t == obj_r
    close(g_t, g_r)


@pytest.mark.parametrize("dtype", FP8)
def test_prefetching_loader_over_an_8bit_pinned_store(dtype):
    from probnmn.data.feature_store import PinnedFeatureStore, PrefetchingLoader

    shape = (50, 1024, 14, 14)
    store = PinnedFeatureStore(features(shape, dtype, seed=1).numpy(), dtype=dtype)
    want = quantised(shape, dtype, seed=1)
    rng = np.random.Generator(np.random.Philox(1))
    host_batches = []
    for k in range(5):
        idx = torch.from_numpy(rng.integers(0, 50, 8 if k != 3 else 5))
        host_batches.append({"image_index": idx, "question": torch.full((idx.numel(), 4), k), "answer": idx % 28,
                             "supervision": (idx % 2)})
    seen = 0
    for k, batch in enumerate(PrefetchingLoader(host_batches, store, DEV, method="kernel")):
        hb = host_batches[k]
        assert set(batch) == {"image", "question", "answer", "supervision"}
        assert batch["supervision"].device.type == "cpu" and batch["question"].is_cuda
        image = batch["image"]
        assert image.dtype == torch.float32 and image.is_contiguous(memory_format=torch.channels_last)
        assert same_bits(image, want[hb["image_index"]])
        assert torch.equal(batch["question"].cpu(), hb["question"])
        seen += 1
    assert seen == 5
    with pytest.raises(ValueError):
        PrefetchingLoader(host_batches, store, DEV, method="dma")
