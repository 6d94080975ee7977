"""Where the seq2seq plan groups a decoder pass's rows by length (seq_plan.py: PNMN_DECODER_LENGTH_ORDER), on the CPU against
the call-recording stand-in of test_seq_plan_build: above 256 rows a teacher-forced pass gets one order, built behind the token
matrix it is counted from and handed to the forward and the backward call; the sampling pass never; with the switch off, or at
24 rows, the calls are the ones they were."""
import numpy as np

from test_seq_plan_build import LISTS, build_plan, calls_of, expected_order


def _at(address, n):
    return np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(np.uint64) * n).from_address(address)).copy()


def _calls(monkeypatch, switch, n, m):
    if switch is None:
        monkeypatch.delenv("PNMN_DECODER_LENGTH_ORDER", raising=False)
    else:
        monkeypatch.setenv("PNMN_DECODER_LENGTH_ORDER", switch)
    plan, _, lib = build_plan(monkeypatch, 0.0, False, n=n, m=m)
    return plan, {name: calls_of(plan, lib, name) for name in LISTS}


def test_large_teacher_forced_passes_get_one_order_each(monkeypatch):
    from probnmn import _hip

    plan, calls = _calls(monkeypatch, "1", 272, 264)
    ptr = {name: t.data_ptr() for name, t in plan._bufs.items()}
    for name in LISTS:
        for entry, args in calls[name]:
            assert len(args) == len(_hip.SIGNATURES[entry]), entry
    # generator: [sampling, teacher forced] -- only the second has an order; reconstructor: its one pass
    for lst, tags in (("fwd_pg", [None, "pg.t"]), ("fwd_qr", ["qr.q"])):
        names = [entry for entry, _ in calls[lst]]
        fwd = [args for entry, args in calls[lst] if entry == "pnmn_attn_lstm_fwd_group_ordered"]
        assert len(fwd) == 1 and "pnmn_attn_lstm_fwd_group" not in names
        order, steps = (_at(fwd[0][k], len(tags)) for k in (10, 11))
        assert [int(o) for o in order] == [ptr[t + ".order"] if t else 0 for t in tags]
        assert [int(s) for s in steps] == [ptr[t + ".tile_steps"] if t else 0 for t in tags]
        # the lists are built behind the token matrix and in front of the decoder launch
        i = names.index("pnmn_decoder_last")
        assert names[i - 1] == "pnmn_token_prep" and names[i + 1] == "pnmn_length_order" and names.count("pnmn_decoder_last") == 1
        assert i + 1 < names.index("pnmn_attn_lstm_fwd_group_ordered")
    bwd = [args for entry, args in calls["bwd_a"] if entry == "pnmn_attn_lstm_bwd_group_ordered"]
    assert len(bwd) == 1
    order, steps = (_at(bwd[0][k], 3) for k in (3, 4))
    assert [int(o) for o in order] == [0, ptr["pg.t.order"], ptr["qr.q.order"]]
    assert [int(s) for s in steps] == [0, ptr["pg.t.tile_steps"], ptr["qr.q.tile_steps"]]
    # the steps are counted from the tokens that mask the pass's loss
    last = [args for lst in ("fwd_pg", "fwd_qr") for entry, args in calls[lst] if entry == "pnmn_decoder_last"]
    assert [(a[0], a[3], a[4]) for a in last] == [(ptr["pg.tgt"] + 8, 264, 13), (ptr["qr.tgt"] + 8, 536, 21)]


def test_switch_off_selects_the_old_calls(monkeypatch):
    _, on = _calls(monkeypatch, "1", 272, 264)
    plan, off = _calls(monkeypatch, "0", 272, 264)
    assert not any(name.startswith(("pg.t.", "qr.q.")) and name.endswith((".last", ".order", ".tile_steps")) for name in plan._bufs)
    for lst in LISTS:
        want, entries = [], [entry for entry, _ in on[lst]]
        for i, e in enumerate(entries):  # the same launches without a decoder's pnmn_decoder_last + pnmn_length_order
            if e == "pnmn_decoder_last" or (e == "pnmn_length_order" and entries[i - 1] == "pnmn_decoder_last"):
                continue
            want.append(e.replace("_group_ordered", "_group"))
        assert [entry for entry, _ in off[lst]] == want, lst


def test_at_24_rows_the_plan_is_call_for_call_what_it_was(monkeypatch):
    plan, calls = _calls(monkeypatch, "1", 24, 7)
    assert {lst: [entry[len("pnmn_"):] for entry, _ in c] for lst, c in calls.items()} == expected_order(False, False)
    assert not any(name.endswith((".order", ".tile_steps")) for name in plan._bufs)
