"""``pnmn_attention_overlay`` restated in numpy (include/probnmn_hip.h states the arithmetic): quantise the map to bytes,
resize it with 8-bit bilinear weights (half-pixel centres), colour it through a table and blend it over the image --
integers throughout, so the kernel's result is these bytes exactly."""
import numpy as np


def quantise(maps):
    """fp32 maps -> int64 0 .. 255: clamp to [0, 1] (NaN -> 0), one fused multiply-add, truncate."""
    a = np.asarray(maps, dtype=np.float32)
    a = np.where(np.isnan(a), np.float32(0), np.minimum(np.maximum(a, np.float32(0)), np.float32(1))).astype(np.float32)
    # (the float64 sum is exact for a >= 2^-22; below that it is 0.5 and a little, which truncates to 0 however it is rounded)
    return np.float32(a.astype(np.float64) * 255.0 + 0.5).astype(np.int64)


def axis_taps(n_in, n_out):
    """(i0, i1, f) per output index: first / second input index and the 8-bit weight of the second."""
    X = np.arange(n_out, dtype=np.int64)
    num = (2 * X + 1) * n_in - n_out
    den = 2 * n_out
    i0 = np.where(num < 0, 0, num // den)
    f = np.where(num < 0, 0, ((num - i0 * den) * 256) // den)
    i0 = np.minimum(i0, n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), f


def resize(q, Hi, Wi):
    """int64 [..., H, W] bytes -> [..., Hi, Wi]."""
    H, W = q.shape[-2:]
    y0, y1, fy = axis_taps(H, Hi)
    x0, x1, fx = axis_taps(W, Wi)
    fy = fy[:, None]
    top = q[..., y0, :][..., x0] * (256 - fx) + q[..., y0, :][..., x1] * fx
    bottom = q[..., y1, :][..., x0] * (256 - fx) + q[..., y1, :][..., x1] * fx
    return (top * (256 - fy) + bottom * fy + 32768) >> 16


def overlay(maps, image_of, images, lut, strength):
    """maps fp32 [n, H, W], image_of int [n] (clamped into range), images uint8 [n_images, Hi, Wi, 3], lut uint8 [256, 3]
    -> uint8 [n, Hi, Wi, 3]."""
    images = np.asarray(images)
    Hi, Wi = images.shape[1:3]
    v = resize(quantise(maps), Hi, Wi)
    w = ((v * int(strength) + 127) // 255)[..., None]
    img = images[np.clip(np.asarray(image_of, dtype=np.int64), 0, images.shape[0] - 1)].astype(np.int64)
    colour = np.asarray(lut).astype(np.int64)[v]
    return ((img * (255 - w) + colour * w + 127) // 255).astype(np.uint8)
