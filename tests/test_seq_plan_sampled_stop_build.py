"""Where the seq2seq plan lets the sampling pass's tiles stop (seq_plan.py: PNMN_SAMPLED_PASS_STOP), on the CPU against the
call-recording stand-in of test_seq_plan_build: with the switch off the calls are the parent's, call for call; with it on the
plan differs by the stop entry point in the place of the forward group call, one pnmn_length_order_steps behind it, and the
ordered backward; at 256 sampled rows and below nothing changes; a plan built without the ``sampled_stop`` argument and without
the switch is the parent's too, and the trainers pass the argument."""
from test_seq_plan_build import LISTS, build_plan, calls_of


def _entries(monkeypatch, stop, order, n, m):
    monkeypatch.setenv("PNMN_SAMPLED_PASS_STOP", stop)
    monkeypatch.setenv("PNMN_DECODER_LENGTH_ORDER", order)
    plan, _, lib = build_plan(monkeypatch, 0.0, False, n=n, m=m)
    return plan, {name: [entry for entry, _ in calls_of(plan, lib, name)] for name in LISTS}


def test_switch_on_differs_from_off_by_the_stop_call_its_order_and_the_ordered_backward(monkeypatch):
    for order in ("1", "0"):
        _, on = _entries(monkeypatch, "1", order, 272, 264)
        plan, off = _entries(monkeypatch, "0", order, 272, 264)
        assert not any(name.startswith("pg.s.") and name.endswith((".steps", ".order", ".tile_steps")) for name in plan._bufs)
        for lst in LISTS:
            want = []
            for e in on[lst]:
                if e == "pnmn_length_order_steps":
                    continue
                if e == "pnmn_attn_lstm_fwd_group_stop":
                    e = "pnmn_attn_lstm_fwd_group_ordered" if order == "1" else "pnmn_attn_lstm_fwd_group"
                if e == "pnmn_attn_lstm_bwd_group_ordered" and order == "0":
                    e = "pnmn_attn_lstm_bwd_group"
                want.append(e)
            assert off[lst] == want, (order, lst)
        assert on["fwd_pg"].count("pnmn_attn_lstm_fwd_group_stop") == 1 and on["fwd_pg"].count("pnmn_length_order_steps") == 1
        assert "pnmn_attn_lstm_bwd_group_ordered" in on["bwd_a"]


def test_at_256_sampled_rows_the_switch_changes_nothing(monkeypatch):
    _, on = _entries(monkeypatch, "1", "1", 256, 280)
    _, off = _entries(monkeypatch, "0", "1", 256, 280)
    assert on == off
    assert not any(e in ("pnmn_attn_lstm_fwd_group_stop", "pnmn_length_order_steps") for calls in on.values() for e in calls)


def test_a_plan_asks_for_the_stop_and_the_switch_overrides_either_way(monkeypatch):
    """Without the argument and without the switch a plan is the parent's; the argument (what the trainers pass) turns the stop
    on; the switch wins over the argument in both directions."""
    from probnmn.runtime import seq_plan

    def names(env, arg):
        if env is None:
            monkeypatch.delenv("PNMN_SAMPLED_PASS_STOP", raising=False)
        else:
            monkeypatch.setenv("PNMN_SAMPLED_PASS_STOP", env)
        real = seq_plan.Seq2SeqPlan
        monkeypatch.setattr(seq_plan, "Seq2SeqPlan", lambda *a: real(*a, sampled_stop=arg))
        plan, _, lib = build_plan(monkeypatch, 0.0, False, n=272, m=264)
        monkeypatch.setattr(seq_plan, "Seq2SeqPlan", real)
        return [entry for lst in LISTS for entry, _ in calls_of(plan, lib, lst)]
    for env, arg, on in ((None, False, False), (None, True, True), ("0", True, False), ("1", False, True)):
        assert ("pnmn_attn_lstm_fwd_group_stop" in names(env, arg)) == on, (env, arg)


def test_the_trainer_asks_for_it(monkeypatch):
    import types

    import torch

    from probnmn.runtime import seq_plan
    from probnmn.trainers import joint_training

    seen = []
    monkeypatch.setattr(seq_plan, "Seq2SeqPlan", lambda *a, **kw: seen.append(kw) or types.SimpleNamespace(still_valid=lambda: True))
    trainer = types.SimpleNamespace(pg=types.SimpleNamespace(_max_decoding_steps=26), qr=None, prior=None)
    assert joint_training._TrainerBase._plan(trainer, torch.device("cpu"), 272, 264, 20, 12) is not None
    assert seen == [dict(sampled_stop=True)]
