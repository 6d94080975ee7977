"""``pnmn_attention_overlay`` and ``pnmn_attention_gather`` (csrc/attention_maps.hip) on the MI355X: the overlay bit for
bit against its numpy restatement (tests/helpers/overlay_reference.py) over map and image sizes, item counts, image
indices, strides and strengths, with nothing written past the output; the gather against slices of the arena."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import overlay_reference as ref  # noqa: E402

from probnmn import _hip  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 37  # poison bytes between two images (also makes every image but the first start off a dword boundary)


def _case(seed, n, H, W, Hi, Wi):
    """Maps with NaN, negative values and values above 1; ``image_of`` repeated, out of order, one index out of range."""
    gen = np.random.default_rng(seed)
    maps = (gen.random((n, H, W), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    maps.reshape(n, -1)[:, 3] = np.nan
    maps.reshape(n, -1)[:, 5] = 7.0
    n_images = 3
    images = gen.integers(0, 256, size=(n_images, Hi, Wi, 3), dtype=np.uint8)
    image_of = np.array([2, 0, 2, 1, 5][:n] if n > 1 else [-3], np.int32)
    lut = gen.integers(0, 256, size=(256, 3), dtype=np.uint8)
    return maps, image_of, images, lut


def _overlay(maps, image_of, images, lut, strength, dev, offset=0):
    """The kernel on images ``GAP`` poison bytes apart, into a buffer with canaries on both sides; ``offset``: the output
    starts that many bytes past an aligned address."""
    n, H, W = maps.shape
    n_images, Hi, Wi, _ = images.shape
    stride = Hi * Wi * 3 + GAP
    packed = np.full(n_images * stride, 0xEE, np.uint8)
    for i in range(n_images):
        packed[i * stride: i * stride + Hi * Wi * 3] = images[i].reshape(-1)
    size = n * Hi * Wi * 3
    buf = torch.full((64 + offset + size + 64,), CANARY, dtype=torch.uint8, device=dev)
    out = buf[64 + offset: 64 + offset + size]
    d = [torch.from_numpy(a).to(dev) for a in (maps, image_of, packed, lut)]
    rc = _hip.lib().pnmn_attention_overlay(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), stride, n_images, Hi, Wi,
                                           d[3].data_ptr(), strength, out.data_ptr(), n, H, W, _hip.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[: 64 + offset] == CANARY) and np.all(host[64 + offset + size:] == CANARY)
    return host[64 + offset: 64 + offset + size].reshape(n, Hi, Wi, 3)


@pytest.mark.parametrize("size", [14, 28])
@pytest.mark.parametrize("Hi, Wi", [(14, 14), (13, 29), (7, 5), (1, 1), (320, 480)])
def test_overlay_is_bit_exact(size, Hi, Wi):
    dev = torch.device("cuda:0")
    for n in (1, 5):
        maps, image_of, images, lut = _case(size * 1000 + Hi + n, n, size, size, Hi, Wi)
        for strength in (0, 160, 255):
            want = ref.overlay(maps, image_of, images, lut, strength)
            got = _overlay(maps, image_of, images, lut, strength, dev)
            assert np.array_equal(got, want), (n, strength, int((got != want).sum()))
            if strength == 0:
                assert np.array_equal(got, images[np.clip(image_of, 0, 2)])


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_overlay_into_an_unaligned_output_and_a_rectangular_map(offset):
    """Rows that begin and end inside a dword (3 * 29 bytes per row, an output ``offset`` bytes past a dword boundary): the
    bytes at a row's ends are stored one by one and the neighbours' are left alone."""
    dev = torch.device("cuda:0")
    maps, image_of, images, lut = _case(77 + offset, 5, 14, 28, 13, 29)
    got = _overlay(maps, image_of, images, lut, 200, dev, offset=offset)
    assert np.array_equal(got, ref.overlay(maps, image_of, images, lut, 200))


def test_overlay_rejects_what_is_beyond_its_limits_and_launches_nothing():
    dev = torch.device("cuda:0")
    maps, image_of, images, lut = _case(1, 2, 14, 14, 8, 8)
    d = [torch.from_numpy(a).to(dev) for a in (maps, image_of, images.reshape(-1), lut)]
    out = torch.full((2 * 8 * 8 * 3,), CANARY, dtype=torch.uint8, device=dev)
    ok = dict(maps=d[0].data_ptr(), image_of=d[1].data_ptr(), images=d[2].data_ptr(), image_stride=192, n_images=3, Hi=8, Wi=8,
              lut=d[3].data_ptr(), strength=160, out=out.data_ptr(), n=2, H=14, W=14)

    def call(**change):
        a = dict(ok, **change)
        return _hip.lib().pnmn_attention_overlay(a["maps"], a["image_of"], a["images"], a["image_stride"], a["n_images"], a["Hi"],
                                                 a["Wi"], a["lut"], a["strength"], a["out"], a["n"], a["H"], a["W"],
                                                 _hip.stream_ptr(dev))

    for change in (dict(maps=None), dict(image_of=None), dict(images=None), dict(lut=None), dict(out=None), dict(H=0), dict(W=0),
                   dict(H=65), dict(W=65), dict(Hi=0), dict(Wi=0), dict(Hi=16385), dict(Wi=16385), dict(strength=-1),
                   dict(strength=256), dict(image_stride=191), dict(n_images=0), dict(n=-1)):
        assert call(**change) == _hip.EINVAL, change
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())  # none of the calls above wrote anything
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(2, 8, 8, 3), ref.overlay(maps, image_of, images, lut, 160))


def test_gather_copies_the_maps_and_zeroes_the_rest():
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    for HW in (196, 784, 1):
        act = torch.randn(64 * 40 + HW, device=dev)
        offsets = torch.tensor([64 * 3, -1, 0, 64 * 39, -1, 64 * 3, 64 * 40], dtype=torch.int64, device=dev)
        n = offsets.numel()
        buf = torch.full((n * HW + 32,), float("nan"), device=dev)
        assert lib.pnmn_attention_gather(act.data_ptr(), offsets.data_ptr(), buf.data_ptr(), n, HW, _hip.stream_ptr(dev)) == 0
        torch.cuda.synchronize()
        got = buf[: n * HW].view(n, HW)
        for j, off in enumerate(offsets.tolist()):
            want = torch.zeros(HW, device=dev) if off < 0 else act[off: off + HW]
            assert torch.equal(got[j], want), (HW, j)
        assert bool(torch.isnan(buf[n * HW:]).all())  # the canary behind the output
    for args in ((None, offsets.data_ptr(), buf.data_ptr(), n, 196), (act.data_ptr(), None, buf.data_ptr(), n, 196),
                 (act.data_ptr(), offsets.data_ptr(), None, n, 196), (act.data_ptr(), offsets.data_ptr(), buf.data_ptr(), n, 0)):
        assert lib.pnmn_attention_gather(*args, _hip.stream_ptr(dev)) == _hip.EINVAL
    before = buf.clone()
    assert lib.pnmn_attention_gather(act.data_ptr(), offsets.data_ptr(), buf.data_ptr(), 0, 196, _hip.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(buf), torch.nan_to_num(before))
