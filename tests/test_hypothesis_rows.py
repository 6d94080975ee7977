"""``probnmn.hypothesis_rows`` without a device: ``question_rows`` as the callers hand them over, the rows a question owns
(questions without a hypothesis at the front, in the middle and at the end; no row; no question) and the two messages the
callers' tests match on."""
import numpy as np
import pytest
import torch

from probnmn import hypothesis_rows


def test_on_host_takes_what_the_callers_hand_over():
    want = np.array([0, 0, 2, 5], np.int64)
    for given in ([0, 0, 2, 5], want.astype(np.int32), torch.tensor([0, 0, 2, 5]), torch.tensor([0, 0, 2, 5], dtype=torch.int32),
                  want[::-1][::-1], np.stack([want, want], 1)[:, 0]):
        rows = hypothesis_rows.on_host(given)
        assert rows.dtype == np.int64 and rows.flags["C_CONTIGUOUS"] and np.array_equal(rows, want)
    assert hypothesis_rows.on_host([]).shape == (0,) and hypothesis_rows.on_host(torch.zeros(0, dtype=torch.long)).dtype == np.int64
    assert hypothesis_rows.on_host([[0, 1], [1, 2]]).shape == (2, 2)  # (the callers refuse it: their messages name their shapes)


def test_group_start_with_empty_groups_at_the_front_in_the_middle_and_at_the_end():
    rows = hypothesis_rows.on_host([2, 2, 2, 3, 6, 6])  # questions 0, 1 | 4, 5 | 7, 8 have no hypothesis
    hypothesis_rows.check(rows, 9)
    start = hypothesis_rows.group_start(rows, 9)
    assert start.tolist() == [0, 0, 0, 3, 4, 4, 4, 6, 6, 6] and start.dtype.kind == "i"
    for g in range(9):  # question g owns exactly the rows that name it
        assert np.array_equal(np.arange(start[g], start[g + 1]), np.nonzero(rows == g)[0])
    # one hypothesis per question; every hypothesis on the last question
    assert hypothesis_rows.group_start(hypothesis_rows.on_host(np.arange(4)), 4).tolist() == [0, 1, 2, 3, 4]
    assert hypothesis_rows.group_start(hypothesis_rows.on_host([3, 3, 3]), 4).tolist() == [0, 0, 0, 0, 3]


def test_no_row_and_no_question():
    none = hypothesis_rows.on_host(np.zeros(0, np.int64))
    for G in (0, 1, 5):
        hypothesis_rows.check(none, G)  # (nothing to be out of range)
        assert hypothesis_rows.group_start(none, G).tolist() == [0] * (G + 1)
    with pytest.raises(ValueError, match=r"question_rows must be non-decreasing and in 0 \.\. -1"):
        hypothesis_rows.check(hypothesis_rows.on_host([0]), 0)  # a row, but no question it could belong to


@pytest.mark.parametrize("rows", [[1, 0], [0, 2, 1, 2], [0, 3], [3], [-1, 0], [0, 1, 2, 3]])
def test_decreasing_and_out_of_range_rows_are_refused(rows):
    with pytest.raises(ValueError, match=r"question_rows must be non-decreasing and in 0 \.\. 2"):
        hypothesis_rows.check(hypothesis_rows.on_host(rows), 3)
    hypothesis_rows.check(hypothesis_rows.on_host(sorted(max(0, min(r, 2)) for r in rows)), 3)  # (clamped and sorted: accepted)


def test_row_vector_names_its_argument():
    cpu = torch.device("cpu")  # (the conversion is torch's own: nothing of it needs the ROCm device)
    for name in ("log_weights", "log_q"):
        v = hypothesis_rows.row_vector(np.array([-1.0, -np.inf, 2.5]), name, 3, cpu)
        assert v.dtype == torch.float32 and v.is_contiguous() and v.tolist() == [-1.0, -float("inf"), 2.5]
        assert hypothesis_rows.row_vector(torch.arange(6.0)[::2], name, 3, cpu).is_contiguous()
        assert hypothesis_rows.row_vector([], name, 0, cpu).shape == (0,)
        for bad in (np.zeros(4), np.zeros((3, 1)), 1.0):
            with pytest.raises(ValueError, match=r"%s \[3\]; got " % name):
                hypothesis_rows.row_vector(bad, name, 3, cpu)
