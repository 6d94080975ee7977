"""``resize_normalize`` (pnmn_image_prep, csrc/image_prep.hip) on the device against ``preprocess`` of the numpy restatement
of Pillow's resize (tests/helpers/pil_resize_reference.py, held against Pillow by tests/test_image_prep_ref.py): integer
arithmetic and a table lookup, so the comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pil_resize_reference as ref  # noqa: E402

from probnmn import _hip  # noqa: E402
from probnmn.data import feature_extractor as fe  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [  # (N, input (H, W), output (H, W))
    (1, (7, 9), (32, 32)),           # upscale, taps clamped at both borders
    (2, (37, 53), (32, 32)),         # row bytes 159, not a multiple of 4
    (1, (64, 100), (64, 32)),        # the vertical pass is the identity
    (1, (97, 224), (32, 224)),       # the horizontal pass is the identity
    (2, (50, 70), (45, 33)),         # odd output sizes, partial last band and row
    (1, (500, 33), (32, 32)),        # 33 taps: the bands shrink to fit the rows their taps span
    (3, (320, 480), (224, 224)),     # CLEVR: several bands and images
]


def expected(images: np.ndarray, size) -> torch.Tensor:
    """(N, size[0], size[1], 3) fp32 on the CPU: ``preprocess`` of the restatement's resize."""
    resized = torch.from_numpy(ref.resize_batch(images, size))
    return fe.preprocess(resized.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


def run(images: np.ndarray, size, monkeypatch) -> torch.Tensor:
    """``resize_normalize`` into memory filled with NaN beforehand: a pixel the kernel does not write fails ``equal``."""
    dev = torch.device("cuda:0")
    real_empty = torch.empty

    def nan_filled(*shape, **kwargs):
        t = real_empty(*shape, **kwargs)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    monkeypatch.setattr(torch, "empty", nan_filled)
    out = fe.resize_normalize(torch.from_numpy(images).to(dev), size)
    monkeypatch.setattr(torch, "empty", real_empty)
    assert out.shape == (images.shape[0], size[0], size[1], 4) and out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("n, in_hw, out_hw", CASES)
def test_resize_normalize_is_pillow_then_preprocess(n, in_hw, out_hw, monkeypatch):
    rng = np.random.default_rng(in_hw[0] * 1000 + in_hw[1])
    images = rng.integers(0, 256, size=(n,) + in_hw + (3,), dtype=np.uint8)
    got = run(images, out_hw, monkeypatch)
    assert torch.equal(got[..., :3], expected(images, out_hw))
    assert torch.equal(got[..., 3], torch.zeros(n, *out_hw))


def test_constant_images_stay_constant(monkeypatch):
    """All 0 and all 255: every tap row sums to one in fixed point closely enough that the extremes come back."""
    images = np.zeros((2, 37, 53, 3), np.uint8)
    images[1] = 255
    got = run(images, (32, 32), monkeypatch)
    lut = fe.normalization_table()
    assert torch.equal(got[..., :3], expected(images, (32, 32)))
    assert torch.equal(got[0, ..., :3], lut[:, 0].expand(32, 32, 3)) and torch.equal(got[1, ..., :3], lut[:, 255].expand(32, 32, 3))
    assert torch.equal(got[..., 3], torch.zeros(2, 32, 32))


def test_over_limit_downscale_is_refused_and_launches_nothing(monkeypatch):
    calls = []
    real = _hip.lib().pnmn_image_prep
    monkeypatch.setattr(_hip.lib(), "pnmn_image_prep", lambda *a: calls.append(a) or real(*a))
    dev = torch.device("cuda:0")
    images = torch.zeros(1, 17 * 32, 40, 3, dtype=torch.uint8, device=dev)  # 17x down: 2 * 17 + 1 = 35 taps
    with pytest.raises(NotImplementedError, match="33 taps"):
        fe.resize_normalize(images, (32, 32))
    with pytest.raises(NotImplementedError, match="width <= 448"):
        fe.resize_normalize(images, (32, 480))
    assert not calls
    out = fe.resize_normalize(images[:, :512], (32, 32))  # 16x: the limit itself runs
    assert len(calls) == 1 and torch.equal(out[..., :3].cpu(), expected(np.zeros((1, 512, 40, 3), np.uint8), (32, 32)))
    empty = fe.resize_normalize(images[:0, :512], (32, 32))  # no images: nothing to launch
    assert empty.shape == (0, 32, 32, 4) and len(calls) == 1
