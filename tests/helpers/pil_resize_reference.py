"""Pillow's 8-bit bilinear ``Image.resize`` restated in numpy: the reference for ``pnmn_image_prep`` and for
``probnmn.data.feature_extractor.resize_coefficients`` (written independently of the latter: one output index at a time,
as Pillow's C loops go, in Python floats -- which are C doubles).

Pillow resizes an 8-bit image in two separable passes with a uint8 image between them, horizontal first.  Per axis it
builds, for every output index, the taps of a triangle filter whose support grows with the downscale factor, normalises
them to sum 1, and rounds them to 22-bit fixed point; a pass is then integer arithmetic.  tests/test_image_prep_ref.py
holds this file against Pillow itself (where it is installed) and against Pillow's recorded outputs in
tests/golden/image_prep.npz."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def triangle(a: float) -> float:
    a = abs(a)
    return 1.0 - a if a < 1.0 else 0.0


def coefficients(in_size: int, out_size: int):
    """(k int32 [out_size][ksize], bounds int32 [out_size][2] = (first input index, tap count)) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale  # (bilinear: a support of 1)
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))   # int(): truncation toward zero, as the C cast
        xmax = min(in_size, int(center + support + 0.5))
        n = xmax - xmin
        w = [triangle((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(0.5 + v * (1 << PRECISION_BITS))  # (a triangle's taps are never negative)
        bounds[xx] = (xmin, n)
    return k, bounds


def one_pass(image: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    """One pass of the resampler along ``axis`` of a uint8 (H, W, C) image: uint8, ``out_size`` long on that axis."""
    k, bounds = coefficients(image.shape[axis], out_size)
    src = np.moveaxis(image, axis, 0).astype(np.int64)
    out = np.zeros((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(n):
            acc += src[xmin + x] * int(k[xx, x])
        assert int(acc.max()) < 2 ** 31 and int(acc.min()) >= 0  # (the C accumulator is an int)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(image: np.ndarray, size) -> np.ndarray:
    """``np.asarray(Image.fromarray(image).resize((size[1], size[0]), BILINEAR))`` for a uint8 (H, W, 3) image and
    ``size`` = (H_out, W_out): the horizontal pass, rounded to uint8, then the vertical pass on its result.  (A pass whose
    size does not change is the identity -- Pillow skips it -- and comes out as such here.)"""
    assert image.dtype == np.uint8 and image.ndim == 3
    return one_pass(one_pass(image, size[1], axis=1), size[0], axis=0)


def resize_batch(images: np.ndarray, size) -> np.ndarray:
    return np.stack([resize(im, size) for im in images])
