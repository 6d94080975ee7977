"""The host beam-search reference (tests/helpers/beam_reference.py) that the GPU beam tests measure against, pinned
on its own: K = 1 is greedy decoding, a hand-worked 3-token example, finished hypotheses, tie-breaking, and
replay = search on the search's own trace.  No GPU."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import beam_reference as br  # noqa: E402

from oracle.seq2seq_oracle import END, PAD, START, UNK, seq2seq_forward, seq2seq_param_shapes  # noqa: E402

NEG = float("-inf")


def _random_sd(v_src, v_tgt, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(s, generator=g, dtype=torch.float64) - 0.5) * 0.4 for k, s in seq2seq_param_shapes(v_src, v_tgt).items()}


def _sources(v_src, rows, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(rows, 6, dtype=torch.long)
    for r in range(rows):
        n = int(torch.randint(2, 7, (1,), generator=g))
        src[r, :n] = torch.randint(4, v_src, (n,), generator=g)
    return src


def test_beam_of_one_is_greedy_up_to_the_first_end():
    sd = _random_sd(20, 15, 0)
    # make @end@ likely enough that some rows finish inside the horizon
    sd["_output_projection_layer.bias"][END] += 1.5
    src = _sources(20, 24, 1)
    T = 10
    greedy = seq2seq_forward(sd, src, None, "greedy", max_decoding_steps=T)
    raw = greedy["raw_predictions"]
    out = br.beam_search(sd, src, 1, T)
    checked = finished = 0
    for b in range(src.size(0)):
        row = raw[b].tolist()
        n = row.index(END) + 1 if END in row else T
        if any(tok in (PAD, UNK, START) for tok in row[:n]):
            continue  # greedy may pick what the beam (as the sampler) never does
        checked += 1
        finished += END in row
        assert out["tokens"][b, 0, :n].tolist() == row[:n]
        assert out["tokens"][b, 0, n:].tolist() == [END] * (T - n)
        want = float(greedy["step_logprobs"][b, :n].sum())
        assert abs(float(out["scores"][b, 0]) - want) < 1e-9
    assert checked >= 12 and finished >= 3, (checked, finished)


def test_hand_worked_two_best():
    """V = 7 (pad, unk, start, end, a, b, c); two hypotheses; probabilities chosen by hand."""
    a, b, c = 4, 5, 6

    def table(pa, pb, pc, pe):  # log-probabilities of a row; pad / unk / start get what is left (they are never chosen)
        rest = (1.0 - pa - pb - pc - pe) / 3
        row = torch.full((7,), math.log(rest), dtype=torch.float64)
        for i, p in ((a, pa), (b, pb), (c, pc), (END, pe)):
            row[i] = math.log(p)
        return row

    # step 0: one live state: a 0.5, b 0.3, c 0.1, end 0.04 -> beams (a, b)
    logp = torch.stack([table(0.5, 0.3, 0.1, 0.04), table(0.1, 0.1, 0.1, 0.1)]).unsqueeze(0)
    last = torch.tensor([[START, START]])
    score = torch.tensor([[0.0, NEG]], dtype=torch.float64)
    tok, bp, score, _ = br.select(br.candidate_table(logp, last, score), 2)
    assert tok.tolist() == [[a, b]] and bp.tolist() == [[0, 0]]
    assert torch.allclose(score, torch.tensor([[math.log(0.5), math.log(0.3)]], dtype=torch.float64))
    # step 1: after a: c 0.4, end 0.3 (0.20, 0.15); after b: end 0.9 (0.27) -> beams (b end 0.27, a c 0.20)
    logp = torch.stack([table(0.1, 0.1, 0.4, 0.3), table(0.02, 0.02, 0.02, 0.9)]).unsqueeze(0)
    tok, bp, score, ranked = br.select(br.candidate_table(logp, tok, score), 2)
    assert tok.tolist() == [[END, c]] and bp.tolist() == [[1, 0]]
    assert torch.allclose(score, torch.tensor([[math.log(0.27), math.log(0.20)]], dtype=torch.float64))
    assert abs(float(ranked[0, 2]) - math.log(0.15)) < 1e-12  # third: a end
    # step 2: the finished one keeps 0.27; after a c: end 0.8 (0.16), a 0.1 (0.02) -> (b end end 0.27, a c end 0.16)
    logp = torch.stack([table(0.3, 0.3, 0.3, 0.05), table(0.1, 0.03, 0.03, 0.8)]).unsqueeze(0)
    tok, bp, score, _ = br.select(br.candidate_table(logp, tok, score), 2)
    assert tok.tolist() == [[END, END]] and bp.tolist() == [[0, 1]]
    assert torch.allclose(score, torch.tensor([[math.log(0.27), math.log(0.16)]], dtype=torch.float64))
    trace_tokens = torch.tensor([[[a, b], [END, c], [END, END]]])
    trace_backptr = torch.tensor([[[0, 0], [1, 0], [0, 1]]])
    assert br.backtrack(trace_tokens, trace_backptr).tolist() == [[[b, END, END], [a, c, END]]]


def test_finished_hypothesis_keeps_its_score_and_offers_only_end():
    logp = torch.log_softmax(torch.randn(1, 2, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(0)), -1)
    last = torch.tensor([[END, 5]])
    score = torch.tensor([[-1.25, -0.5]], dtype=torch.float64)
    cand = br.candidate_table(logp, last, score).view(2, 9)
    assert float(cand[0, END]) == -1.25 and int(torch.isfinite(cand[0]).sum()) == 1
    assert all(float(cand[1, i]) == NEG for i in (PAD, UNK, START))
    assert torch.equal(cand[1, 3:], score[0, 1] + logp[0, 1, 3:])
    # no finite candidate at all: token @end@, back-pointer 0, score -inf
    tok, bp, sc, _ = br.select(torch.full((1, 18), NEG, dtype=torch.float64), 2)
    assert tok.tolist() == [[END, END]] and bp.tolist() == [[0, 0]] and sc.tolist() == [[NEG, NEG]]
    # one finite candidate for two slots
    one = torch.full((1, 18), NEG, dtype=torch.float64)
    one[0, 9 + 6] = -2.0
    tok, bp, sc, _ = br.select(one, 2)
    assert tok.tolist() == [[6, END]] and bp.tolist() == [[1, 0]] and sc.tolist() == [[-2.0, NEG]]


def test_ties_break_by_flat_index():
    cand = torch.full((1, 3 * 8), NEG, dtype=torch.float64)
    for flat, v in ((2 * 8 + 4, -1.0), (0 * 8 + 7, -1.0), (1 * 8 + 5, -1.0), (1 * 8 + 6, -0.5)):
        cand[0, flat] = v
    tok, bp, sc, _ = br.select(cand, 3)
    assert list(zip(bp[0].tolist(), tok[0].tolist())) == [(1, 6), (0, 7), (1, 5)]
    assert sc.tolist() == [[-0.5, -1.0, -1.0]]


def test_replay_of_the_search_trace_reproduces_the_search():
    sd = _random_sd(18, 12, 3)
    sd["_output_projection_layer.bias"][END] += 1.0
    src = _sources(18, 9, 4)
    out = br.beam_search(sd, src, 4, 7)
    tables = br.replay(sd, src, out["trace_tokens"], out["trace_backptr"])
    V = 12
    for t, cand in enumerate(tables):
        tok, bp, sc, _ = br.select(cand, 4)
        assert torch.equal(tok, out["trace_tokens"][:, t]) and torch.equal(bp, out["trace_backptr"][:, t])
        assert torch.equal(sc, out["trace_scores"][:, t])
        assert cand.shape == (9, 4 * V)
    assert torch.equal(br.backtrack(out["trace_tokens"], out["trace_backptr"]), out["tokens"])
    assert torch.equal(out["scores"], out["trace_scores"][:, -1])
