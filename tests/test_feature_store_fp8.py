"""8-bit feature stores, the host side alone (no device work): which dtypes a store takes, and that ``_check_overflow``
refuses exactly the finite values that torch's own conversion does not keep finite -- NaN beyond 464 for
``torch.float8_e4m3fn`` (which has no infinity; the tie at 464 goes to 448), infinity from 61440 on for ``torch.float8_e5m2``."""
import numpy as np
import pytest
import torch

from probnmn import _hip
from probnmn.data import feature_store as fs

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


def refused(value: float, dtype) -> bool:
    chunk = torch.zeros((6, 8, 3, 3), dtype=torch.float32)
    chunk[4, 3, 1, 1] = value
    try:
        fs._check_overflow(chunk, dtype, 0)
    except OverflowError as e:
        assert "row 4" in str(e)
        return True
    return False


def test_elem_accepts_exactly_five_dtypes():
    every = [torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2,
             torch.float8_e4m3fnuz, torch.float8_e5m2fnuz, torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64,
             torch.bool, torch.complex64]
    taken = {}
    for dtype in every:
        try:
            taken[dtype] = fs._elem(dtype)
        except ValueError as e:
            assert str(dtype) in str(e)
    assert taken == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, E4M3: 4, E5M2: 5}
    assert (_hip.ELEM_F32, _hip.ELEM_F16, _hip.ELEM_BF16, _hip.ELEM_F8E4M3, _hip.ELEM_F8E5M2) == (0, 1, 2, 4, 5)
    assert 3 not in taken.values()  # (no element type: the library refuses it)


def test_what_torch_does_at_the_edges():
    """The facts the thresholds rest on, as this torch converts on the host."""
    x = torch.tensor([448.0, 464.0, float(np.nextafter(np.float32(464.0), np.float32(np.inf))), 1e9, float("inf"), 2.0 ** -10,
                      1.0001 * 2.0 ** -10, 2.0 ** -9], dtype=torch.float32)
    got = x.to(E4M3).float()
    assert got[:2].tolist() == [448.0, 448.0] and bool(torch.isnan(got[2:5]).all())
    assert got[5:].tolist() == [0.0, 2.0 ** -9, 2.0 ** -9]
    y = torch.tensor([57344.0, 61439.9, 61440.0, float("inf"), 2.0 ** -17, 2.0 ** -16], dtype=torch.float32)
    got = y.to(E5M2).float()
    assert got.tolist() == [57344.0, 57344.0, float("inf"), float("inf"), 0.0, 2.0 ** -16]


@pytest.mark.parametrize("dtype, last_kept", [(E4M3, 464.0), (E5M2, float(np.nextafter(np.float32(61440.0), np.float32(0.0))))])
def test_check_overflow_refuses_exactly_what_torch_does_not_keep_finite(dtype, last_kept):
    """Every fp32 within 64 units of the last place on either side of the threshold, both signs, plus far values: refused
    if and only if the host conversion of the (finite) value is not finite."""
    centre = np.float32(last_kept)
    around = [centre]
    lo = hi = centre
    for _ in range(64):
        lo, hi = np.nextafter(lo, np.float32(0.0)), np.nextafter(hi, np.float32(np.inf))
        around += [lo, hi]
    values = [float(v) for v in around] + [0.0, 1.0, 447.0, 448.0, 480.0, 57344.0, 61439.9, 65504.0, 1e9, 3e38]
    values += [-v for v in values]
    finite_after = torch.isfinite(torch.tensor(values, dtype=torch.float32).to(dtype).float()).tolist()
    assert True in finite_after and False in finite_after
    for value, kept in zip(values, finite_after):
        assert refused(value, dtype) == (not kept), value
    assert not refused(last_kept, dtype) and refused(float(np.nextafter(centre, np.float32(np.inf))), dtype)
    # what is not finite in the source is the source's business
    for value in (float("inf"), float("-inf"), float("nan")):
        assert not refused(value, dtype)


def test_messages_and_the_types_that_never_refuse():
    chunk = torch.zeros((6, 8, 3, 3), dtype=torch.float32)
    chunk[5, 0, 0, 0] = -464.5
    with pytest.raises(OverflowError) as e:
        fs._check_overflow(chunk, E4M3, 100)
    assert "row 105" in str(e.value) and "NaN" in str(e.value) and "464" in str(e.value)
    fs._check_overflow(chunk, E5M2, 100)
    chunk[5, 0, 0, 0] = 61440.0
    with pytest.raises(OverflowError) as e:
        fs._check_overflow(chunk, E5M2, 0)
    assert "row 5" in str(e.value) and "infinity" in str(e.value)
    chunk[5, 0, 0, 0] = 3e38
    fs._check_overflow(chunk, torch.float32, 0)
    fs._check_overflow(chunk[:0], E4M3, 0)  # (an empty chunk)
