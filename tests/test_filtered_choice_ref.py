"""The host reference of filtered sampling (tests/helpers/filtered_choice.py) that the GPU tests measure against, held to
the rule's own consequences without a device; and the python layer's argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import filtered_inputs as fi  # noqa: E402
from filtered_choice import filtered_sample_ref, kernel_uniform, ranks_within_allowed  # noqa: E402
from token_choice import sample_ref  # noqa: E402

PAD, UNK, START = fi.PAD, fi.UNK, fi.START


def _rows(N, V, seed, scales=(1.0, 2.0, 5.0, 20.0)):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, V)) * np.asarray(scales)[np.arange(N) % len(scales), None]
    return z.astype(np.float32).astype(np.float64), rng.integers(0, 2 ** 24, N) / 2.0 ** 24


@pytest.mark.parametrize("V", [1, 3, 4, 5, 44, 129])
def test_identity_filter_is_sample_ref(V):
    z, u = _rows(500, V, V)
    z[::7, V // 2] = -np.inf
    z[5::50] = np.nan
    z[6::50, -1] = np.inf
    tok, margin, kept = filtered_sample_ref(z, u, PAD, UNK, START)
    want, want_margin = sample_ref(z, u, PAD, UNK, START)
    assert np.array_equal(tok, want)
    np.testing.assert_array_equal(margin, want_margin)
    assert kept[np.arange(len(tok)), tok].all()


@pytest.mark.parametrize("V", [4, 5, 44, 100])
def test_top_k_one_is_the_first_allowed_argmax_for_every_u(V):
    z, _ = _rows(300, V, 3 * V)
    z[::3, V - 1] = z[::3, 3:].max(1)  # an exact tie for the largest allowed logit in every third row
    want = 3 + np.argmax(z[:, 3:], 1)
    for u in (0.0, 0.25, 0.999, 1.0 - 2.0 ** -24):
        for temperature in (0.25, 1.0, 2.0):
            tok, margin, kept = filtered_sample_ref(z, np.full(len(z), u), PAD, UNK, START, temperature, 1, 1.0)
            assert np.array_equal(tok, want)
            assert (kept.sum(1) == 1).all()


@pytest.mark.parametrize("filt", fi.FILTERS + [(1.0, 3, 0.3), (0.5, 1000, 1.0)])
def test_a_token_is_never_outside_the_kept_set(filt):
    for V in (4, 5, 44, 128):
        z, u = _rows(400, V, V + int(100 * filt[0]))
        tok, _, kept = filtered_sample_ref(z, u, PAD, UNK, START, *filt)
        assert kept[np.arange(len(tok)), tok].all()
        assert not kept[:, :3].any() and (tok >= 3).all()
        n_allowed = V - 3
        if filt[1] > 0:
            assert (kept.sum(1) <= min(filt[1], n_allowed)).all()
        if filt[1] >= n_allowed and filt[2] == 1.0:
            assert (kept.sum(1) == n_allowed).all()
        rank = ranks_within_allowed(z, PAD, UNK, START, filt[0])
        assert (np.where(kept, rank, -1).max(1) == kept.sum(1) - 1).all()  # a prefix of the ranking


@pytest.mark.parametrize("top_p", [0.1, 0.5, 0.9, 0.95])
def test_top_p_keeps_the_smallest_prefix_that_reaches_p(top_p):
    V = 60
    z, u = _rows(500, V, int(top_p * 100))  # (continuous values: no ties)
    for temperature in (0.7, 1.0):
        _, _, kept = filtered_sample_ref(z, u, PAD, UNK, START, temperature, 0, top_p)
        for row in range(len(z)):
            p = np.exp(z[row, 3:] / temperature - (z[row, 3:] / temperature).max())
            p /= p.sum()
            order = np.argsort(-p)
            n = int(np.searchsorted(np.cumsum(p[order]), top_p, side="left")) + 1  # smallest prefix with mass >= top_p
            assert set(np.flatnonzero(kept[row])) == set(3 + order[:n])


def test_exact_ties_resolve_to_the_lower_index():
    z = np.array([[9.0, 9.0, 9.0, 1.0, 2.0, 2.0, 2.0, 0.5, 2.0]])
    for k, want in ((1, [4]), (2, [4, 5]), (3, [4, 5, 6]), (4, [4, 5, 6, 8]), (5, [3, 4, 5, 6, 8])):
        tok, margin, kept = filtered_sample_ref(z, [0.5], PAD, UNK, START, 1.0, k, 1.0)
        assert np.flatnonzero(kept[0]).tolist() == want
        assert np.isfinite(margin).all() or k in (1, 4, 5)
    # top-p over four equal weights (and two small ones): mass before the third tied index is 2 / (4 + e^-1 + e^-1.5) < 0.5
    _, _, kept = filtered_sample_ref(z, [0.5], PAD, UNK, START, 1.0, 0, 0.5)
    assert np.flatnonzero(kept[0]).tolist() == [4, 5, 6]
    assert ranks_within_allowed(z, PAD, UNK, START, 1.0)[0].tolist()[3:] == [4, 0, 1, 2, 5, 3]


def test_rows_the_fallback_serves_ignore_the_filter():
    V = 44
    z, u = _rows(40, V, 1)
    z[0::4, 7] = np.nan
    z[1::4, 9] = np.inf
    z[2::4, 3:] = -np.inf
    z[3::4, :3], z[3::4, 3:] = 100.0, z[3::4, 3:] - 60.0  # allowed softmax weights that round to 0 in fp32
    want, _ = sample_ref(z, u, PAD, UNK, START)
    for filt in fi.FILTERS:
        tok, _, _ = filtered_sample_ref(z, u, PAD, UNK, START, *filt)
        assert np.array_equal(tok, want)


def test_sampling_filter_block_matches_the_c_struct(tmp_path):
    """``struct pnmn_sampling_filter`` is a host argument block, not a work-item record: the binding derives its dtype
    from the header beside the records (``HOST_BLOCKS``).  Size and offsets against the C compiler's."""
    import subprocess

    from probnmn import _hip

    dtype = _hip.HOST_BLOCKS["pnmn_sampling_filter"]
    assert dtype is _hip.SAMPLING_FILTER and "pnmn_sampling_filter" not in _hip.RECORDS
    assert dtype.names == ("temperature", "top_k", "top_p", "reserved")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "probnmn_hip.h"\nint main(){printf("%zu", '
                   'sizeof(struct pnmn_sampling_filter));'
                   + "".join('printf(" %%zu", offsetof(struct pnmn_sampling_filter, %s));' % f for f in dtype.names)
                   + "return 0;}")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.dirname(_hip.HEADER_PATH), str(src), "-o", str(exe)])
    seen = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert seen == [16, 0, 4, 8, 12] == [dtype.itemsize] + [dtype.fields[f][1] for f in dtype.names]
    for name in ("pnmn_sample_tokens", "pnmn_attn_lstm_fwd", "pnmn_attn_lstm_fwd_group"):
        assert name in _hip.SIGNATURES
        assert name + "_filtered" not in _hip.SIGNATURES  # (an option is an argument, not a second entry point)
    # the reader takes a plain struct by the same field rules, and refuses what it refuses in a record
    _hip.read_header(text="struct pnmn_blk { float a; int32_t n[2]; };\nint pnmn_f(const struct pnmn_blk* b, void* stream);")
    assert _hip.HOST_BLOCKS.pop("pnmn_blk").itemsize == 12
    with pytest.raises(_hip.HipLibraryError):
        _hip.read_header(text="struct pnmn_blk { int16_t n; };")


def test_python_layer_refuses_values_out_of_range():
    """``sampling_filter`` is what ``choose_tokens``, ``Seq2SeqBase.forward`` / ``decode`` and ``predict_answers`` check
    their arguments with; none of this touches a device."""
    from probnmn.evaluators import predict_answers
    from probnmn.models import ProgramGenerator
    from probnmn.modules.seq2seq_base import Seq2SeqBase, sampling_filter
    from probnmn.vocabulary import Vocabulary

    model = ProgramGenerator(Vocabulary.clevr())  # (on the CPU: every check below comes before the first device call)
    question = torch.zeros(2, 5, dtype=torch.long)

    assert sampling_filter() is None and sampling_filter(1, 0, 1) is None
    assert sampling_filter(0.7, 10, 0.9) == (0.7, 10, 0.9)
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
           dict(top_k=-1), dict(top_k=2.5), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1),
           dict(top_p=float("nan")), dict(temperature=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            sampling_filter(**kw)
        with pytest.raises(ValueError):
            Seq2SeqBase._check_filter("sampling", **{**dict(temperature=1.0, top_k=0, top_p=1.0), **kw})
        with pytest.raises(ValueError):
            predict_answers(None, None, [], None, **kw)
    for strategy in ("greedy", "beam"):
        assert Seq2SeqBase._check_filter(strategy, 1.0, 0, 1.0) is None
        with pytest.raises(ValueError):
            Seq2SeqBase._check_filter(strategy, 0.7, 0, 1.0)
        with pytest.raises(ValueError):
            model(question, decoding_strategy=strategy, top_k=5)
        with pytest.raises(ValueError):
            model.decode({}, decoding_strategy=strategy, top_p=0.9)
    with pytest.raises(ValueError):
        model(question, temperature=0.0)
    with pytest.raises(ValueError):
        model.decode({}, top_p=2.0)
    with pytest.raises(ValueError):
        predict_answers(None, None, [], None, beam_size=4, temperature=0.7)


def _ambiguous_share(z, u, filt, delta):
    _, margin, _ = filtered_sample_ref(z, u, PAD, UNK, START, *filt)
    return int((margin < delta).sum())


@pytest.mark.parametrize("filt", fi.FILTERS)
def test_the_reference_leaves_few_rows_ambiguous_on_the_gpu_tests_inputs(filt):
    """The GPU tests excuse at most 5 % (+ 5) of a case's rows; the reference itself must need at most 2.5 % -- over the
    rows of every standalone vocabulary (the very inputs of the GPU test, its cases pooled: a case of one or five rows has
    no percentage), and over the decoder cases' rows: their logits come from the device's own hidden states, so here from
    the same decoder run in fp64 on the host from the same inputs under the reference's own draws -- the device's rows up
    to round-off."""
    for V in fi.STANDALONE_V:
        n = rows = 0
        for logits, seed, step, row_offset in fi.standalone_inputs(V):
            B = logits.size(0)
            u = kernel_uniform(seed, row_offset + np.arange(B, dtype=np.uint64), step)
            n += _ambiguous_share(logits.double().numpy(), u, filt, fi.STANDALONE_DELTA)
            rows += B
        print("standalone V=%d filter=%s: %d of %d rows within %g" % (V, filt, n, rows, fi.STANDALONE_DELTA))
        assert n <= 0.025 * rows, (V, filt, n, rows)
    pooled_n = pooled_rows = 0
    for B, T, S, V in fi.DECODER_SHAPES:
        d = fi.decoder_inputs(B, S, V, B + T + S + V)
        for f, seed, row_offset in fi.decoder_filter_cases():
            if f != filt:
                continue
            rows = row_offset + np.arange(B, dtype=np.uint64)
            z = fi.emulate_decoder_logits(
                d, T, lambda logits, t: filtered_sample_ref(logits, kernel_uniform(seed, rows, t), PAD, UNK, START, *filt)[0])
            u = kernel_uniform(seed, rows[:, None], np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
            n = _ambiguous_share(z, u, filt, fi.DECODER_DELTA)
            print("decoder %dx%d S=%d V=%d filter=%s: %d of %d rows within %g" % (B, T, S, V, filt, n, B * T, fi.DECODER_DELTA))
            if B * T >= 200:
                assert n <= 0.025 * B * T, (B, T, V, filt, n)
            pooled_n, pooled_rows = pooled_n + n, pooled_rows + B * T
    assert pooled_n <= 0.025 * pooled_rows, (filt, pooled_n, pooled_rows)  # (with the shapes of 1 and 35 rows)
