"""Host reference of the dropout mask between an encoder's LSTM layers (``pnmn_lstm_dropout`` and the dropout
instantiations of ``pnmn_lstm_stack_*``), numpy only, written from the contract in include/probnmn_hip.h:

* keep(row, t, u): Philox4x32-10 under key ``{seed lo, seed hi}`` with counter ``{row lo, row hi, t, u}``; output word 0
  gives ``u01 = (x0 >> 8) * 2**-24``; the element is kept iff ``u01 < 1.0f - p`` (fp32);
* row = ``row_offset`` + the row's index in the pass;
* ``y = x * keep * scale`` with ``scale = 1.0f / (1.0f - p)`` (fp32): a dropped element is ``x * 0``."""
import numpy as np

from token_choice import philox4x32_10

_LO = np.uint64(0xFFFFFFFF)


def keep_mask(seed: int, rows: int, T: int, H: int, p: float, row_offset: int = 0) -> np.ndarray:
    """bool [rows, T, H]: which elements the mask keeps."""
    row = (np.uint64(row_offset) + np.arange(rows, dtype=np.uint64))[:, None, None]
    t = np.arange(T, dtype=np.uint64)[None, :, None]
    u = np.arange(H, dtype=np.uint64)[None, None, :]
    row, t, u = np.broadcast_arrays(row, t, u)
    ctr = np.stack([row & _LO, row >> np.uint64(32), t, u], -1).astype(np.uint32)
    seed = np.uint64(seed)
    key = np.array([seed & _LO, seed >> np.uint64(32)], dtype=np.uint64).astype(np.uint32)
    x0 = philox4x32_10(ctr, key)[..., 0]
    u01 = (x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u01 < np.float32(1.0) - np.float32(p)


def scale_of(p: float) -> np.float32:
    """1.0f / (1.0f - p) in fp32 (+inf for p = 1, where nothing is kept)."""
    with np.errstate(divide="ignore"):
        return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def multiplier(seed: int, rows: int, T: int, H: int, p: float, row_offset: int = 0) -> np.ndarray:
    """float32 [rows, T, H]: keep * scale per element (0 where dropped)."""
    return np.where(keep_mask(seed, rows, T, H, p, row_offset), scale_of(p), np.float32(0.0)).astype(np.float32)


def apply(x: np.ndarray, seed: int, p: float, row_offset: int = 0) -> np.ndarray:
    """The kernel's fp32 result for x [rows, T, H] (float32): x * (keep ? scale : 0)."""
    x = np.asarray(x, dtype=np.float32)
    rows, T, H = x.shape
    return x * multiplier(seed, rows, T, H, p, row_offset)
