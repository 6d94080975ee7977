"""The host reference of the kernels' token choice (tests/token_choice.py) on its own: the Random123 known-answer vectors
of Philox4x32-10, the uniforms it makes, and hand-made rows whose token is known exactly."""
import numpy as np
import pytest

from token_choice import greedy_ref, kernel_uniform, philox4x32_10, sample_ref

PAD, UNK, START = 0, 1, 2


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, out):
    got = philox4x32_10(np.array([ctr], dtype=np.uint32), np.array([key], dtype=np.uint32))
    assert [int(x) for x in got[0]] == list(out)
    # vectorised over rows: the same vector among others gives the same output
    many = philox4x32_10(np.array([ctr, (1, 2, 3, 4), ctr], dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert [int(x) for x in many[2]] == list(out) and [int(x) for x in many[0]] == list(out)


def test_kernel_uniform_counter_layout():
    """Counter {row lo, row hi, step, 0x9E3779B9}, key {seed lo, seed hi}, u = (x0 >> 8) / 2**24."""
    seed, row, step = (5 << 32) | 7, (3 << 32) | 11, 9
    x0 = philox4x32_10(np.array([11, 3, 9, 0x9E3779B9], dtype=np.uint32), np.array([7, 5], dtype=np.uint32))[0]
    assert kernel_uniform(seed, row, step) == (int(x0) >> 8) / 2.0 ** 24
    # each part of the counter and key matters
    base = kernel_uniform(seed, row, step)
    for s, r, t in ((seed ^ 1, row, step), (seed ^ (1 << 40), row, step), (seed, row ^ 1, step), (seed, row ^ (1 << 40), step),
                    (seed, row, step + 1)):
        assert kernel_uniform(s, r, t) != base


def test_uniforms_are_24_bit_and_in_range():
    u = kernel_uniform(2 ** 62 - 1, np.arange(2 ** 32 - 5000, 2 ** 32 + 5000, dtype=np.uint64), 2 ** 31)
    assert u.dtype == np.float64 and u.min() >= 0.0 and u.max() < 1.0
    scaled = u * 2.0 ** 24
    assert np.array_equal(scaled, np.floor(scaled))
    assert len(np.unique(u)) > 9990  # (no short cycle across the 32-bit word of the row)


def test_uniforms_chi_square():
    """10**6 uniforms over (row, step) into 1000 equal bins: chi-square with 999 degrees of freedom, within ~6 sigma."""
    rows = np.arange(250000, dtype=np.uint64)
    u = np.concatenate([kernel_uniform(1234, rows, t) for t in range(4)])
    counts = np.bincount((u * 1000).astype(np.int64), minlength=1000)
    expect = u.size / 1000
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert 999 - 6 * np.sqrt(2 * 999) < chi2 < 999 + 6 * np.sqrt(2 * 999), chi2
    # consecutive draws of one row are not correlated
    a, b = kernel_uniform(99, rows, 0), kernel_uniform(99, rows, 1)
    assert abs(np.corrcoef(a, b)[0, 1]) < 6 / np.sqrt(rows.size)


def _row(V, fill=-np.inf, **entries):
    z = np.full(V, fill)
    for j, x in entries.items():
        z[int(j[1:])] = x
    return z


def test_sampling_excludes_pad_unk_start():
    # equal weights on 3, 4 (pad / unk / start huge): u < 1/2 -> 3, else 4
    z = _row(6, 0.0, i0=50.0, i1=50.0, i2=50.0, i5=-np.inf)
    tok, margin = sample_ref(np.stack([z] * 4), np.array([0.0, 0.49, 0.5, 0.99]), PAD, UNK, START)
    assert tok.tolist() == [3, 3, 4, 4]
    np.testing.assert_allclose(margin, [0.5, 0.01, 0.0, 0.49], atol=1e-12)
    # other excluded indices
    tok, _ = sample_ref(np.zeros((2, 5)), np.array([0.0, 0.999]), 4, 3, 0)
    assert tok.tolist() == [1, 2]


def test_sampling_inverse_cdf_with_minus_inf_entries():
    # weights 1 : 2 : 1 on indices 3, 5, 7 (log-weights), -inf elsewhere
    z = _row(8, -np.inf, i3=0.0, i5=np.log(2.0), i7=0.0, i0=3.0)
    u = np.array([0.0, 0.2499, 0.25, 0.7499, 0.75, 1 - 2.0 ** -24])
    tok, margin = sample_ref(np.stack([z] * len(u)), u, PAD, UNK, START)
    assert tok.tolist() == [3, 3, 5, 5, 7, 7]
    np.testing.assert_allclose(margin[:3], [0.25, 1e-4, 0.0], atol=1e-12)


@pytest.mark.parametrize("V", [63, 64, 65])
def test_sampling_across_the_64_lane_chunk(V):
    """Equal weights on the allowed indices 3..V-1: u picks index 3 + floor(u * (V - 3)) -- across the chunk boundary."""
    n = V - 3
    u = (np.arange(n) + 0.5) / n
    tok, margin = sample_ref(np.zeros((n, V)), u, PAD, UNK, START)
    assert tok.tolist() == list(range(3, V))
    np.testing.assert_allclose(margin, 0.5 / n, rtol=1e-9)
    # all mass on the last index
    z = np.full((1, V), -np.inf)
    z[0, V - 1] = 1.0
    assert sample_ref(z, np.array([0.3]), PAD, UNK, START)[0].tolist() == [V - 1]


def test_greedy_is_torch_argmax():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    z = rng.standard_normal((200, 65)).astype(np.float32)
    z[10, 7] = z[10, 40] = 9.0  # exact tie: first wins
    z[11, :] = -np.inf
    z[12, 64] = np.inf
    z[13, 30] = np.nan
    z[14, 5] = np.inf
    z[14, 6] = np.nan  # NaN beats +inf
    z[15, :] = np.nan
    tok, gap = greedy_ref(z)
    assert np.array_equal(tok, torch.argmax(torch.from_numpy(z), 1).numpy())
    assert tok[10] == 7 and gap[10] == 0.0 and tok[13] == 30 and tok[14] == 6 and tok[15] == 0
    srt = np.sort(z[0].astype(np.float64))
    assert gap[0] == srt[-1] - srt[-2]


def test_fallbacks():
    """The rule for rows the inverse CDF cannot serve (include/probnmn_hip.h)."""
    V = 70
    rows, want = [], []
    z = _row(V, 0.0, i66=np.nan)  # one NaN (allowed): the NaN
    rows.append(z), want.append(66)
    z = _row(V, 0.0, i1=np.nan, i9=4.0)  # NaN only on an excluded index: first allowed maximum
    rows.append(z), want.append(9)
    rows.append(np.full(V, np.nan)), want.append(3)  # all NaN: first allowed
    z = _row(V, 0.0, i65=np.inf, i66=np.inf)  # +inf: first allowed +inf
    rows.append(z), want.append(65)
    z = _row(V, -np.inf, i0=1.0, i2=5.0)  # every allowed logit -inf: first allowed index
    rows.append(z), want.append(3)
    rows.append(np.full(V, -np.inf)), want.append(3)
    z = _row(V, -10.0, i0=100.0, i1=100.0, i2=100.0, i64=-8.0)  # allowed weights underflow in fp32: drawn relative to -8
    rows.append(z), want.append(None)
    u = np.full(len(rows), 0.5)
    tok, margin = sample_ref(np.stack(rows), u, PAD, UNK, START)
    for i, w in enumerate(want):
        if w is not None:
            assert tok[i] == w and margin[i] == np.inf, (i, tok[i], w)
    # the underflow row: softmax over allowed = e^2 on 64, 1 elsewhere -> the same draw as with the excluded entries gone
    z = rows[-1].copy()
    z[:3] = -np.inf
    ref, _ = sample_ref(z[None], u[:1], PAD, UNK, START)
    assert tok[-1] == ref[0]
    us = (np.arange(1000) + 0.5) / 1000
    t_under, _ = sample_ref(np.stack([rows[-1]] * 1000), us, PAD, UNK, START)
    w = np.exp(rows[-1] + 8.0)
    w[:3] = 0
    cdf = np.cumsum(w) / w.sum()
    assert np.array_equal(t_under, np.searchsorted(cdf, us, side="right"))
    # no allowed token (V <= 3): the greedy choice, NaN largest
    for z, w in (([1.0, 3.0, 2.0], 1), ([1.0, np.nan, 5.0], 1), ([np.nan] * 3, 0), ([4.0, 4.0], 0), ([-np.inf], 0)):
        assert sample_ref(np.array([z]), np.array([0.7]), PAD, UNK, START)[0][0] == w, z
