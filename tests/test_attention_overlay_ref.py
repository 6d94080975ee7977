"""The numpy restatement of ``pnmn_attention_overlay`` (tests/helpers/overlay_reference.py), which the GPU tests hold the
kernel to bit for bit, against the properties that define it: identity at the map's own size, the two ends of the blend,
closeness to exact bilinear interpolation, and the quantiser's treatment of values outside [0, 1]."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import overlay_reference as ref  # noqa: E402

MAP_SIZES = [(14, 14), (28, 28), (14, 28), (28, 14)]
IMAGE_SIZES = [(14, 14), (13, 29), (7, 5), (1, 1), (320, 480)]


def _inputs(seed, n, H, W, Hi, Wi, n_images=2):
    gen = np.random.default_rng(seed)
    maps = gen.random((n, H, W), dtype=np.float32)
    images = gen.integers(0, 256, size=(n_images, Hi, Wi, 3), dtype=np.uint8)
    lut = gen.integers(0, 256, size=(256, 3), dtype=np.uint8)
    return maps, images, lut


def test_quantiser_clamps_and_rounds():
    got = ref.quantise(np.array([np.nan, -1.0, 2.0, 0.0, 1.0, 0.5, 1.0 / 255, 0.49 / 255, 0.51 / 255, -np.inf, np.inf], np.float32))
    assert got.tolist() == [0, 0, 255, 0, 255, 128, 1, 0, 1, 0, 255]


@pytest.mark.parametrize("H, W", MAP_SIZES)
def test_resize_to_the_maps_own_size_is_the_identity(H, W):
    q = np.random.default_rng(H * 100 + W).integers(0, 256, size=(3, H, W)).astype(np.int64)
    assert np.array_equal(ref.resize(q, H, W), q)


def test_strength_zero_returns_the_image():
    maps, images, lut = _inputs(1, 3, 14, 14, 13, 29)
    out = ref.overlay(maps, [1, 0, 1], images, lut, 0)
    assert np.array_equal(out, images[[1, 0, 1]])


def test_strength_255_blends_by_the_maps_value_and_returns_the_colour_where_it_is_full():
    """w = (v * 255 + 127) / 255 = v: the colour table's entry where the map is 1, the image where it is 0, and
    (img * (255 - v) + lut[v] * v + 127) / 255 between."""
    maps, images, lut = _inputs(2, 3, 14, 14, 13, 29)
    maps[0] = 1.0
    maps[1] = 0.0
    out = ref.overlay(maps, [0, 1, 0], images, lut, 255)
    assert np.array_equal(out[0], np.broadcast_to(lut[255], out[0].shape))
    assert np.array_equal(out[1], images[1])
    v = ref.resize(ref.quantise(maps[2]), 13, 29)
    want = (images[0].astype(np.int64) * (255 - v[..., None]) + lut.astype(np.int64)[v] * v[..., None] + 127) // 255
    assert np.array_equal(out[2], want.astype(np.uint8))


@pytest.mark.parametrize("H, W", MAP_SIZES)
def test_resize_is_within_two_and_a_half_levels_of_exact_bilinear(H, W):
    """Two weights truncated by less than 1/256 each on a range of 255, plus the final rounding: |v - exact| < 2.5."""
    gen = np.random.default_rng(7 * H + W)
    q = gen.integers(0, 256, size=(4, H, W)).astype(np.int64)
    q[1] = (np.indices((H, W)).sum(0) % 2) * 255  # a checkerboard: the largest steps between neighbours
    worst = 0.0
    for Hi, Wi in IMAGE_SIZES:
        exact = F.interpolate(torch.from_numpy(q).double()[None], size=(Hi, Wi), mode="bilinear", align_corners=False)[0].numpy()
        got = ref.resize(q, Hi, Wi)
        assert got.min() >= 0 and got.max() <= 255
        worst = max(worst, float(np.abs(got - exact).max()))
    print("largest |v - exact| for %dx%d maps: %.3f" % (H, W, worst))
    assert worst < 2.5


def test_image_index_is_clamped_into_range():
    maps, images, lut = _inputs(3, 2, 14, 14, 7, 5)
    assert np.array_equal(ref.overlay(maps, [-4, 9], images, lut, 160), ref.overlay(maps, [0, 1], images, lut, 160))
