"""pnmn_length_order / pnmn_length_order_steps as one workgroup of up to sixteen waves, against numpy's stable sort: the order
is longest first and stable in the row index, tile_steps the longest row of every 16-row tile -- at row counts around a wave
and around sixteen waves, step counts up to the largest the entry point takes (where fewer waves fit), all-equal lengths, and
lengths outside [0, T), which the kernel clamps."""
import numpy as np
import pytest
import torch

from probnmn import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_T = 4096  # the largest T the entry point accepts (include/probnmn_hip.h)


def _run(values, T, entry="pnmn_length_order"):
    B = len(values)
    v = torch.from_numpy(np.asarray(values, np.int32)).to(DEV)
    order = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tile_steps = torch.full(((B + 15) // 16,), -1, dtype=torch.int32, device=DEV)
    rc = getattr(_hip.lib(), entry)(v.data_ptr(), B, T, order.data_ptr(), tile_steps.data_ptr(), _hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, order.cpu().numpy(), tile_steps.cpu().numpy()


def _check(steps, order, tile_steps):
    want = np.argsort(-steps, kind="stable")
    assert np.array_equal(order, want)
    assert np.array_equal(tile_steps, np.array([steps[want[k:k + 16]].max() for k in range(0, len(steps), 16)]))


@pytest.mark.parametrize("T", [1, 8, 64, MAX_T])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 64, 65, 1000, 1031])
def test_against_numpys_stable_sort(B, T):
    rng = np.random.Generator(np.random.Philox(B * 7 + T))
    last = rng.integers(0, T, B)
    rc, order, tile_steps = _run(last, T)
    assert rc == 0
    _check(last + 1, order, tile_steps)
    rc, order, tile_steps = _run(last + 1, T, "pnmn_length_order_steps")  # the same lists from the step counts
    assert rc == 0
    _check(last + 1, order, tile_steps)


@pytest.mark.parametrize("T", [1, 8, 64, MAX_T])
def test_all_equal_lengths_keep_the_row_order(T):
    rc, order, tile_steps = _run(np.full(1031, T // 2), T)
    assert rc == 0
    assert np.array_equal(order, np.arange(1031)) and bool((tile_steps == T // 2 + 1).all())


@pytest.mark.parametrize("B", [17, 1031])
def test_lengths_outside_the_range_are_clamped(B):
    T = 8
    rng = np.random.Generator(np.random.Philox(B))
    last = rng.integers(-5, T + 5, B)
    last[:4] = [-2 ** 31, 2 ** 31 - 2, -1, T]
    rc, order, tile_steps = _run(last, T)
    assert rc == 0
    _check(np.clip(last.astype(np.int64) + 1, 1, T), order, tile_steps)
    steps_in = rng.integers(-5, T + 6, B)
    rc, order, tile_steps = _run(steps_in, T, "pnmn_length_order_steps")
    assert rc == 0
    _check(np.clip(steps_in, 1, T), order, tile_steps)


def test_more_steps_than_the_entry_point_takes():
    assert _run(np.zeros(16), MAX_T + 1)[0] == _hip.CONSTANTS["PNMN_ESHAPE"]
