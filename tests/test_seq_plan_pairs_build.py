"""Where the seq2seq plan sums its weight gradients over the valid (row, step) pairs (seq_plan.py: VALID_PAIRS_ABOVE_ROWS), on
the CPU against the call-recording stand-in of test_seq_plan_build: above the threshold every product with a transposed
first operand goes through pnmn_gemm_rows with a list that a pnmn_valid_rows call in front of it builds; with the switch off,
or at 24 rows, the calls are the ones they were."""
import numpy as np

from test_seq_plan_build import LISTS, build_plan, calls_of, expected_order


def _at(address, dtype, n):
    return np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dtype) * n).from_address(address)).copy()


def _entries(plan, lib):
    return {name: calls_of(plan, lib, name) for name in LISTS}


def test_above_the_threshold_every_weight_gradient_has_a_list(monkeypatch):
    from probnmn import _hip

    monkeypatch.delenv("PNMN_GEMM_VALID_PAIRS", raising=False)
    plan, _, lib = build_plan(monkeypatch, 0.0, False, n=272, m=264)
    calls = _entries(plan, lib)
    built, products = {}, 0
    for name in LISTS:
        for entry, args in calls[name]:
            assert len(args) == len(_hip.SIGNATURES[entry]), entry
            if entry == "pnmn_valid_rows":
                assert name == "bwd_b"
                n = args[8]
                last, mask, rows, T, lists, counts = (_at(args[k], t, n) for k, t in
                                                      ((0, np.uint64), (1, np.uint64), (4, np.int32), (5, np.int32), (6, np.uint64), (7, np.uint64)))
                assert n <= 8 and all((a == 0) != (b == 0) for a, b in zip(last, mask))
                for k in range(n):
                    built.setdefault((int(lists[k]), int(counts[k])), []).append(int(rows[k]) * int(T[k]))
            elif entry in ("pnmn_gemm", "pnmn_gemm_cus", "pnmn_gemm_rows"):
                rec = _at(args[0], np.uint8, args[1] * _hip.GEMM_DESC.itemsize).view(_hip.GEMM_DESC)
                listed = entry == "pnmn_gemm_rows"
                rows, counts = (_at(args[k], np.uint64, args[1]) for k in (2, 3)) if listed else ((0,) * args[1],) * 2
                for d, r, c in zip(rec, rows, counts):
                    if d["flags"] & _hip.GEMM_A_T:
                        # a list built earlier in this backward, over exactly this product's k rows
                        assert listed and name == "bwd_b" and sum(built[(int(r), int(c))]) == d["K"]
                        products += 1
                    else:
                        assert r == 0 and c == 0
    # two encoders x three products, the generator's decoder 2 + its two passes, the reconstructor's 2 + 1; six lists
    assert products == 13 and len(built) == 6
    order = [entry for entry, _ in calls["bwd_b"]]
    assert order.index("pnmn_valid_rows") < order.index("pnmn_gemm_rows") and order.count("pnmn_valid_rows") == 1


def _names(monkeypatch, switch, n, m):
    monkeypatch.setenv("PNMN_GEMM_VALID_PAIRS", switch)
    plan, _, lib = build_plan(monkeypatch, 0.0, False, n=n, m=m)
    return {name: [entry[len("pnmn_"):] for entry, _ in calls] for name, calls in _entries(plan, lib).items()}, plan


def test_at_24_rows_the_plan_is_call_for_call_what_it_was(monkeypatch):
    names, plan = _names(monkeypatch, "1", 24, 7)
    assert names == expected_order(False, False)
    assert not any(".valid" in name for name in plan._bufs)


def test_switch_off_selects_the_whole_products(monkeypatch):
    on, _ = _names(monkeypatch, "1", 272, 264)
    off, plan = _names(monkeypatch, "0", 272, 264)
    assert not any(entry in ("gemm_rows", "valid_rows") for calls in off.values() for entry in calls)
    assert not any(".valid" in name for name in plan._bufs)
    # otherwise the same launches in the same order
    assert off == {name: ["gemm_cus" if e == "gemm_rows" else e for e in calls if e != "valid_rows"] for name, calls in on.items()}
