"""The image front end without a GPU: the numpy restatement of Pillow's 8-bit bilinear resize
(tests/helpers/pil_resize_reference.py) against Pillow's recorded outputs and against Pillow itself, the package's
coefficient tables and normalisation table against it, and what ``resize_normalize`` / ``forward_pixels`` /
``pnmn_image_prep`` refuse.  Reference: scripts/preprocess/extract_features.py:60-73 (Resize, ToTensor, Normalize)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import make_image_prep_golden as golden  # noqa: E402
import pil_resize_reference as ref  # noqa: E402

from probnmn import _hip  # noqa: E402
from probnmn.data import feature_extractor as fe  # noqa: E402

# (input (H, W), output (H, W)): the shapes the restatement was first held against Pillow on
PILLOW_CASES = [((320, 480), (224, 224)), ((37, 53), (32, 32)), ((20, 24), (32, 64)), ((224, 224), (224, 224)),
                ((64, 100), (64, 32)), ((7, 9), (32, 32)), ((500, 33), (32, 32)), ((97, 224), (32, 224))]
AXES = [(480, 224), (320, 224), (53, 32), (24, 64), (7, 32), (500, 32), (33, 32), (224, 224), (9, 9), (70, 33), (50, 45),
        (512, 32), (1, 4), (4, 1)]


def test_restatement_equals_pillows_recorded_outputs(golden_dir):
    data = np.load(os.path.join(golden_dir, "image_prep.npz"))
    for i, (in_hw, out_hw) in enumerate(golden.CASES):
        image, want = data["in_%d" % i], data["out_%d" % i]
        assert image.shape == in_hw + (3,) and want.shape == out_hw + (3,) and want.dtype == np.uint8
        assert np.array_equal(image, golden.seeded_image(in_hw, out_hw))  # (the fixture is what the script writes)
        assert np.array_equal(ref.resize(image, out_hw), want), (in_hw, out_hw)


@pytest.mark.parametrize("in_hw, out_hw", PILLOW_CASES)
def test_restatement_equals_pillow(in_hw, out_hw):
    pytest.importorskip("PIL")
    image = golden.seeded_image(in_hw, out_hw)
    assert np.array_equal(ref.resize(image, out_hw), golden.pillow_resize(image, out_hw))


@pytest.mark.parametrize("in_size, out_size", AXES)
def test_package_coefficients_equal_the_restatements(in_size, out_size):
    k, bounds = fe.resize_coefficients(in_size, out_size)
    want_k, want_bounds = ref.coefficients(in_size, out_size)
    assert k.dtype == np.int32 and bounds.dtype == np.int32
    assert k.shape == want_k.shape and bounds.shape == (out_size, 2)
    assert np.array_equal(k, want_k) and np.array_equal(bounds, want_bounds)
    # every row's taps sum to one in fixed point, within the rounding of its taps; none beyond its count, none negative
    ksize = k.shape[1]
    assert np.all(np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= ksize)
    assert np.all(k >= 0) and np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 0] + bounds[:, 1] <= in_size)
    assert np.all((np.arange(ksize)[None, :] < bounds[:, 1:2]) | (k == 0))


def test_coefficient_known_answers():
    k, bounds = fe.resize_coefficients(224, 224)
    assert k.shape == (224, 3) and np.array_equal(k, np.tile(np.array([1 << 22, 0, 0], np.int32), (224, 1)))
    assert np.array_equal(bounds[:, 0], np.arange(224))  # the identity: output i is input i
    k, bounds = fe.resize_coefficients(480, 224)
    assert k.shape == (224, 7)  # support 480 / 224 = 2.14 -> 2 * 3 + 1
    assert fe.resize_coefficients(512, 32)[0].shape[1] == 33 == _hip.IMAGE_PREP_MAX_TAPS  # a 16x downscale
    # upscale 2 -> 4: centres 0.25, 0.75, 1.25, 1.75 between the input's 0.5 and 1.5; the border taps are renormalised
    k, bounds = fe.resize_coefficients(2, 4)
    assert np.array_equal(bounds, [[0, 1], [0, 2], [0, 2], [1, 1]])
    assert np.array_equal(k[:, :2], [[1 << 22, 0], [3 << 20, 1 << 20], [1 << 20, 3 << 20], [1 << 22, 0]])
    with pytest.raises(ValueError):
        fe.resize_coefficients(0, 4)


def test_normalization_table_is_preprocess_of_every_byte():
    lut = fe.normalization_table()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32 and lut.is_contiguous()
    image = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    assert torch.equal(lut.view(1, 3, 16, 16), fe.preprocess(image))
    assert float(lut[2, 255]) == pytest.approx((1.0 - 0.406) / 0.224, abs=1e-6)


def test_cpu_tensors_and_wrong_inputs_are_refused():
    images = torch.zeros(2, 40, 48, 3, dtype=torch.uint8)
    with pytest.raises(_hip.HipLibraryError):
        fe.resize_normalize(images, (32, 32))
    with pytest.raises(_hip.HipLibraryError):
        fe.ResNet101Stage3().forward_pixels(images, (32, 32))
    for wrong in (images.float(), images[0], images.permute(0, 3, 1, 2), torch.zeros(2, 0, 48, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            fe.resize_normalize(wrong, (32, 32))
    with pytest.raises(ValueError):
        fe.resize_normalize(images, (32,))


def _call(**changes):
    """pnmn_image_prep with arguments that pass every check (pointers it would never follow: the checks come first),
    then ``changes``."""
    args = dict(images=64, image_stride=3 * 40 * 48, N=0, Hin=40, Win=48, kx=64, xbounds=64, ksx=5, ky=64, ybounds=64, ksy=5,
                lut=64, out=64, Hout=32, Wout=32, stream=0)
    assert not set(changes) - set(args)
    args.update(changes)
    return _hip.lib().pnmn_image_prep(*args.values())


def test_entry_point_refuses_before_launching():
    """No device is needed: the entry returns before it launches anything."""
    assert _call() == 0  # N == 0: nothing to do
    for pointer in ("images", "kx", "xbounds", "ky", "ybounds", "lut", "out"):
        assert _call(**{pointer: 0}) == _hip.EINVAL, pointer
        assert _call(**{pointer: 0, "N": 2}) == _hip.EINVAL, pointer
    for name in ("Hin", "Win", "Hout", "Wout", "ksx", "ksy"):
        assert _call(**{name: 0}) == _hip.EINVAL and _call(**{name: -3, "N": 2}) == _hip.EINVAL, name
    assert _call(N=-1) == _hip.EINVAL
    assert _call(image_stride=3 * 40 * 48 - 1) == _hip.EINVAL  # images would overlap
    # beyond the limits the header states
    assert _call(ksx=_hip.IMAGE_PREP_MAX_TAPS) == 0 and _call(ksy=_hip.IMAGE_PREP_MAX_TAPS) == 0
    assert _call(ksx=_hip.IMAGE_PREP_MAX_TAPS + 1) == _hip.EINVAL and _call(ksy=_hip.IMAGE_PREP_MAX_TAPS + 1, N=2) == _hip.EINVAL
    assert _call(Wout=_hip.IMAGE_PREP_MAX_WIDTH) == 0 and _call(Wout=_hip.IMAGE_PREP_MAX_WIDTH + 1, N=2) == _hip.EINVAL
    big = _hip.IMAGE_PREP_MAX_SIZE + 1
    assert _call(Hout=big, N=2) == _hip.EINVAL
    assert _call(Hin=big, image_stride=3 * big * 48, N=2) == _hip.EINVAL
    assert _call(Win=big, image_stride=3 * 40 * big, N=2) == _hip.EINVAL
    assert (_hip.IMAGE_PREP_MAX_TAPS, _hip.IMAGE_PREP_MAX_WIDTH, _hip.IMAGE_PREP_MAX_SIZE) == (33, 448, 16384)
