"""Half-precision feature stores: rows kept as fp16 / bf16 -- page-locked on the host (PinnedFeatureStore) or in HBM
(DeviceFeatureStore) -- and widened to fp32 by the kernels that read them (pnmn_gather_features_typed, pnmn_expand_rows).
What the networks see is exactly ``features.to(dtype).float()``: every comparison of stored or gathered values here is
BITWISE (int32 / int16 views: ``torch.equal`` on floats does not see the sign of a zero), against torch's own host
conversion.  The reference keeps float64 rows in HDF5 and casts per item (readers.py:63-108, datasets.py:137-142)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HALF = [torch.float16, torch.bfloat16]

# Values at which a conversion can go wrong, written over the first elements of every other row: ties of fp16 (1 + 2^-11
# rounds down to even, 1 + 3 * 2^-11 up to even), just above a tie, the smallest fp16 subnormal (6e-8 -> 2^-24) and just
# below half of it (-> 0), an fp16 subnormal, the largest fp16 and the largest value that still rounds to it, a negative
# zero, a tie of bf16 (1 + 2^-8 rounds down to even) and a value between two bf16.  All of them stay finite in both half types.
EDGES = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 6e-8, 2.98e-8, 1e-6, 65504.0, 65519.9, -0.0,
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -9]


@functools.lru_cache(maxsize=None)
def features(shape, seed=0):
    """Seeded relu(randn) of ``shape`` (N, C, H, W), fp32, with the edge values in it -- at the start of every other
    row (so in channel 0) and, shifted, at its end (the last channel: a channel tail where there is one)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.relu(torch.randn(shape, generator=g))
    flat = feats.view(shape[0], -1)
    edges = torch.tensor(EDGES, dtype=torch.float32)
    for r in range(0, shape[0], 2):
        flat[r, : len(EDGES)] = edges
        flat[r, -len(EDGES):] = edges.flip(0)
    return feats


@functools.lru_cache(maxsize=None)
def quantised(shape, dtype, seed=0):
    """The reference: torch's host conversion of the same features, widened again (exact)."""
    return torch.from_numpy(features(shape, seed).numpy()).to(dtype).float()


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def check_edge_table():
    """The table itself, as torch converts it on the host: what the tests below rely on."""
    e = torch.tensor(EDGES, dtype=torch.float32)
    for dtype in HALF:
        assert bool(torch.isfinite(e.to(dtype)).all())
    h = e.half().float()
    assert h[0] == 1.0 and h[1] == 1 + 2.0 ** -9 and h[2] == 1 + 2.0 ** -10 and h[3] == 2.0 ** -24 and h[4] == 0.0
    assert h[7] == 65504.0 and bits(h)[8] == -2 ** 31
    b = e.bfloat16().float()
    assert b[9] == 1.0 and b[10] == 1 + 2.0 ** -7


# Which loads of the half gather each shape takes (a pinned store starts page aligned; an item whose whole map fits the
# tile is ONE run of (channels of the block) x HW elements):
#   (9, 72, 14, 14)  a channel's run is 392 bytes, 8 mod 16; rows of 28 224 bytes; the 64-channel block and the 8-channel
#                    tail (1 568 elements) are 16-byte aligned runs of a multiple of 8 elements: 16-byte loads
#   (5, 64, 28, 28)  the map is cut into pixel ranges of 200, 200, 200 and 184 pixels, read channel by channel: 16-byte loads
#   (3, 136, 5, 4)   three channel blocks, the last one 8 wide (160 elements): 16-byte loads
#   (6, 8, 3, 3)     odd HW, but the item's run is 72 elements and rows are 144 bytes apart: still 16-byte loads
#   (6, 7, 3, 3)     runs of 63 elements: 2-byte loads, one run
#   (4, 65, 14, 14)  rows of 25 480 bytes, 8 mod 16: the odd rows' 64-channel block is only 8-byte aligned, and the
#                    1-channel tail is 196 elements, no multiple of 8: 8-byte loads (even rows' blocks: 16-byte)
#   (3, 8, 15, 15)   HW = 225 > 200: ranges of 200 and 25 pixels, odd: 2-byte loads channel by channel (stride HW, tile
#                    rows of 200)
#   (3, 8, 18, 12)   HW = 216 > 200, a multiple of 8: ranges of 200 and 16 pixels, 16-byte loads channel by channel
#   (3, 8, 17, 12)   HW = 204 > 200, a multiple of 4 only: ranges of 200 and 4 pixels, 8-byte loads channel by channel
GATHER_SHAPES = [(9, 72, 14, 14), (5, 64, 28, 28), (3, 136, 5, 4), (6, 8, 3, 3), (6, 7, 3, 3), (4, 65, 14, 14), (3, 8, 15, 15),
                 (3, 8, 18, 12), (3, 8, 17, 12)]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shape", GATHER_SHAPES)
def test_gather_from_a_half_pinned_store_is_exact(shape, dtype):
    from probnmn.data.feature_store import PinnedFeatureStore

    check_edge_table()
    feats = features(shape).numpy()
    N = shape[0]
    store = PinnedFeatureStore(feats, chunk_rows=4, dtype=dtype)
    assert store.store.dtype == dtype and store.store.is_pinned() and tuple(store.store.shape) == shape
    assert same_bits(store.store, torch.from_numpy(feats).to(dtype))
    idx = torch.tensor([N - 1, 0, 2, N - 1, 1, 2, 0])  # repeated, out of order
    want = quantised(shape, dtype)[idx]
    assert same_bits(want, torch.from_numpy(feats).to(dtype)[idx].float())
    for index in (idx, idx.to(DEV)):  # from the host (validated there) and already on the device
        got = store.gather(index, DEV)
        assert got.dtype == torch.float32 and tuple(got.shape) == (7,) + shape[1:]
        assert got.is_contiguous(memory_format=torch.channels_last)
        assert same_bits(got, want)
    with pytest.raises(IndexError):
        store.gather(torch.tensor([0, N]), DEV)
    with pytest.raises(ValueError):
        store.copy_rows(idx, DEV)  # (the copy engines cannot widen)


def test_a_store_keeps_only_the_three_float_types():
    from probnmn.data.feature_store import DeviceFeatureStore, PinnedFeatureStore

    feats = features((6, 8, 3, 3)).numpy()
    for dtype in (torch.float64, torch.int16, torch.uint8):
        with pytest.raises(ValueError):
            PinnedFeatureStore(feats, dtype=dtype)
        with pytest.raises(ValueError):
            DeviceFeatureStore(feats, DEV, dtype=dtype)
    # the default is what it was: fp32, bit for bit
    store = PinnedFeatureStore(feats)
    assert store.store.dtype == torch.float32
    assert same_bits(store.gather(torch.tensor([5, 0, 5]), DEV), torch.from_numpy(feats)[[5, 0, 5]])


def test_the_library_refuses_other_element_pairs():
    from probnmn import _hip

    assert (_hip.ELEM_F32, _hip.ELEM_F16, _hip.ELEM_BF16) == (0, 1, 2)
    lib = _hip.lib()
    src = torch.zeros(2 * 8 * 4, dtype=torch.float32, device=DEV)
    dst = torch.zeros(2 * 8 * 4, dtype=torch.float32, device=DEV)
    idx = torch.zeros(2, dtype=torch.long, device=DEV)
    st = _hip.stream_ptr(DEV)
    for s, d in [(1, 1), (1, 2), (2, 1), (2, 2), (3, 0), (0, 3), (-1, 0)]:
        assert lib.pnmn_gather_features_typed(src.data_ptr(), s, idx.data_ptr(), dst.data_ptr(), d, 2, 2, 8, 4, st) == _hip.EINVAL
    for s in (0, 3, -1):
        assert lib.pnmn_expand_rows(src.data_ptr(), s, idx.data_ptr(), dst.data_ptr(), 2, 2, 32, st) == _hip.EINVAL
    torch.cuda.synchronize()


def test_overflow_is_refused_where_the_half_type_has_no_such_value():
    from probnmn.data.feature_store import DeviceFeatureStore, PinnedFeatureStore

    feats = features((6, 8, 3, 3)).numpy().copy()
    feats[4, 3, 1, 1] = 65520.0  # the smallest value that fp16 rounds to infinity
    for build in (lambda **kw: PinnedFeatureStore(feats, chunk_rows=4, **kw), lambda **kw: DeviceFeatureStore(feats, DEV, chunk_rows=4, **kw)):
        with pytest.raises(OverflowError) as e:
            build(dtype=torch.float16)
        assert "row 4" in str(e.value)
        build(dtype=torch.bfloat16)  # (bf16 has fp32's range)
        build()
    got = PinnedFeatureStore(feats, dtype=torch.bfloat16).gather(torch.tensor([4]), DEV)
    assert same_bits(got, torch.from_numpy(feats).bfloat16()[[4]].float())
    feats[1, 0, 0, 0] = 3.4e38  # beyond the largest bf16 (3.3895e38) by more than half a unit of its last place
    for build in (lambda: PinnedFeatureStore(feats, dtype=torch.bfloat16), lambda: DeviceFeatureStore(feats, DEV, dtype=torch.bfloat16)):
        with pytest.raises(OverflowError) as e:
            build()
        assert "row 1" in str(e.value)
    feats[1, 0, 0, 0] = np.inf  # an infinity of the source is the source's business
    feats[4, 3, 1, 1] = 1.0
    assert bool(torch.isinf(PinnedFeatureStore(feats, dtype=torch.float16).store[1, 0, 0, 0]))


@pytest.mark.parametrize("dtype", HALF)
def test_device_fill_and_expand_rows_are_exact(dtype):
    from probnmn.data.feature_store import DeviceFeatureStore, ResidentRows

    shape = (9, 72, 14, 14)
    feats = features(shape)
    nhwc = feats.to(dtype).permute(0, 2, 3, 1).contiguous()
    store = DeviceFeatureStore(feats.numpy(), DEV, chunk_rows=4, dtype=dtype)  # (chunks of 4, 4 and 1 rows)
    assert store.rows.dtype == dtype == store.dtype and tuple(store.rows.shape) == (9, 14, 14, 72)
    assert store.row_bytes == 72 * 196 * 2 and len(store) == 9
    assert same_bits(store.rows, nhwc)
    idx = torch.tensor([8, 0, 3, 8, 1, 3])
    rows = store.batch(idx)
    assert isinstance(rows, ResidentRows) and rows.shape == (6, 72, 14, 14) and rows.is_cuda
    got = rows.materialize()
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    assert same_bits(got, quantised(shape, dtype)[idx])
    with pytest.raises(TypeError):
        rows.pointers()
    # adopted without a copy
    there = nhwc.to(DEV).permute(0, 3, 1, 2)
    adopted = DeviceFeatureStore.from_device(there)
    assert adopted.data_ptr() == there.data_ptr() and adopted.dtype == dtype and adopted.row_bytes == 72 * 196 * 2
    assert same_bits(adopted.batch(idx).materialize(), quantised(shape, dtype)[idx])
    with pytest.raises(ValueError):
        DeviceFeatureStore.from_device(there.contiguous())  # NCHW storage
    # filled chunk by chunk from device tensors: one fp32 chunk (rounded by copy_), one already in the store's dtype
    filled = DeviceFeatureStore.empty(9, (72, 14, 14), DEV, dtype)
    assert filled.dtype == dtype and filled.row_bytes == store.row_bytes and filled.image_feature_size == (72, 14, 14)
    filled.write_rows(0, feats[:5].to(DEV).contiguous(memory_format=torch.channels_last))
    filled.write_rows(5, feats[5:].to(dtype).to(DEV).contiguous(memory_format=torch.channels_last))
    assert same_bits(filled.rows, nhwc)
    with pytest.raises(IndexError):
        filled.write_rows(6, feats[5:].to(DEV))
    with pytest.raises(ValueError):
        filled.write_rows(0, feats[:2].double().to(DEV))


@pytest.mark.parametrize("dtype", HALF)
def test_expand_rows_element_by_element_and_out_of_range(dtype):
    """Rows of 9 * 8 = 72 and of 3 * 3 * 5 = 45 elements: the 16-byte path and the scalar one of pnmn_expand_rows, more
    rows than one work item each; an index outside the store reads row 0 (the gather's rule)."""
    from probnmn import _hip
    from probnmn.data.feature_store import DeviceFeatureStore

    for shape in [(7, 8, 3, 3), (7, 5, 3, 3), (3, 1024, 4, 4)]:  # (the last: two 8192-element work items per row)
        feats = features(shape)
        store = DeviceFeatureStore(feats.numpy(), DEV, dtype=dtype)
        idx = torch.tensor([6 % shape[0], 0, 2, 2])
        assert same_bits(store.batch(idx).materialize(), quantised(shape, dtype)[idx])
        raw = torch.tensor([1, shape[0], -1], dtype=torch.long, device=DEV)
        out = torch.empty((3,) + shape[1:], dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
        elems = shape[1] * shape[2] * shape[3]
        _hip.check(_hip.lib().pnmn_expand_rows(store.data_ptr(), 1 if dtype == torch.float16 else 2, raw.data_ptr(), out.data_ptr(),
                                               3, shape[0], elems, _hip.stream_ptr(DEV)), "expand_rows")
        assert same_bits(out, quantised(shape, dtype)[[1, 0, 0]])


def test_the_network_sees_exactly_the_quantised_features():
    """A module-training step and a joint-training step fed with rows of an fp16 resident store against the same steps
    fed with the tensor ``feats.half().float()[idx]``: the same losses, objective and sampled programs (bit-equal forward
    pass) and the same gradients up to the order of the weight gradients' atomic adds -- the bar, models and indices of
    tests/test_feature_store_gpu.py: test_resident_store_feeds_the_network_without_a_copy.  The module step once more from
    the fp16 pinned store's gather."""
    from probnmn.data.feature_store import DeviceFeatureStore, PinnedFeatureStore
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.trainers.joint_training import JointTrainingStep
    from probnmn.trainers.module_training import ModuleTrainingStep
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    shape = (23, 1024, 14, 14)
    feats = features(shape, seed=5)
    idx = torch.tensor([3, 22, 3, 0, 17, 9, 9, 21, 1, 14, 6, 2])
    store16 = DeviceFeatureStore(feats.numpy(), DEV, chunk_rows=7, dtype=torch.float16)
    want = feats.half().float()[idx]
    assert same_bits(store16.batch(idx).materialize(), want)
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
    loss_r, grads_r = module_step(store16.batch(idx))
    assert torch.equal(loss_t, loss_r)
    close(grads_t, grads_r)
    pinned16 = PinnedFeatureStore(feats.numpy(), dtype=torch.float16)
    loss_p, grads_p = module_step(pinned16.gather(idx, DEV))
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
    obj_r, z_r, g_r = joint_step(store16.batch(idx))  # (the step takes its unsupervised subset, then widens only that)
    assert torch.equal(z_t, z_r) and obj_t == obj_r
    close(g_t, g_r)


@pytest.mark.parametrize("dtype", HALF)
def test_prefetching_loader_over_a_half_pinned_store(dtype):
    from probnmn.data.feature_store import PinnedFeatureStore, PrefetchingLoader

    shape = (50, 1024, 14, 14)
    store = PinnedFeatureStore(features(shape, seed=1).numpy(), dtype=dtype)
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


def test_evaluators_take_resident_batches():
    """evaluate_answer_accuracy and predict_answers over batches whose "image" is a ResidentRows -- of an fp32 store (which
    used to end in an AttributeError: the loops ask ``image.is_cuda``) and of an fp16 one -- return what they return for
    the materialised tensors."""
    from probnmn.data.feature_store import DeviceFeatureStore
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import evaluate_answer_accuracy, predict_answers
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(3)
    pg = ProgramGenerator(vocab).to(DEV).eval()
    nmn = NeuralModuleNetwork(vocab).to(DEV).eval()
    host = synthetic_batch(vocab, 16, seed=8)
    feats = features((16, 1024, 14, 14), seed=2)
    splits = [torch.tensor([5, 0, 15, 5, 9, 2, 11, 7]), torch.tensor([1, 14, 3, 3, 8, 6, 13, 10])]
    for dtype in (torch.float32, torch.float16):
        store = DeviceFeatureStore(feats.numpy(), DEV, dtype=dtype)
        resident, plain = [], []
        for rows in splits:
            b = {k: v[rows].to(DEV) for k, v in host.items() if k != "image"}
            resident.append(dict(b, image=store.batch(rows)))
            plain.append(dict(b, image=store.batch(rows).materialize()))
            assert same_bits(plain[-1]["image"], feats.to(dtype).float()[rows])
        got, want = evaluate_answer_accuracy(pg, nmn, resident), evaluate_answer_accuracy(pg, nmn, plain)
        assert got == want and "nmn" in got
        torch.manual_seed(11)
        records = predict_answers(pg, nmn, resident, vocab)
        torch.manual_seed(11)
        assert records == predict_answers(pg, nmn, plain, vocab) and len(records) == 16
