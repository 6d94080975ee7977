"""Host reference of the token choice of ``pnmn_sample_tokens`` and the decoder kernels (csrc/sampling.h), numpy only.

Written from the header's contract (include/probnmn_hip.h, beside ``pnmn_sample_tokens``), not from device output:

* the uniform of (seed, row, step) is Philox4x32-10 (Salmon et al. 2011, the Random123 generator) with counter
  ``{row lo, row hi, step, 0x9E3779B9}`` and key ``{seed lo, seed hi}``; ``u = (x0 >> 8) / 2**24``;
* sampling is the index-order inverse CDF of the softmax restricted to the allowed tokens (all but pad, unk, start);
* greedy is ``torch.argmax``: a NaN counts as the largest value, the first index wins;
* rows that hold a NaN or +inf, or whose allowed weights vanish, follow the fallback rule of the header.

Everything is fp64; the kernels work in fp32, so a draw whose ``u`` lies within round-off of a CDF boundary may land on
either side: ``sample_ref`` reports that distance (the margin) so a test can tell such rows apart."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 of counters ``ctr`` [..., 4] under keys ``key`` [..., 2] (uint32, broadcast against each other);
    returns [..., 4] uint32."""
    ctr = np.asarray(ctr, dtype=np.uint32)
    key = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).astype(np.uint64) for i in range(4)]
    k0 = np.broadcast_to(key[..., 0], shape).astype(np.uint32)
    k1 = np.broadcast_to(key[..., 1], shape).astype(np.uint32)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _LO, p1 >> np.uint64(32), p1 & _LO
        c = [hi1 ^ c[1] ^ k0.astype(np.uint64), lo1, hi0 ^ c[3] ^ k1.astype(np.uint64), lo0]
        with np.errstate(over="ignore"):
            k0, k1 = k0 + _W0, k1 + _W1
    return np.stack([x.astype(np.uint32) for x in c], -1)


def kernel_uniform(seed, row, step):
    """The uniform the kernels draw for (seed, row, step), each an integer or an array of them (broadcast): float64
    values, each a multiple of 2**-24 in [0, 1) (and exactly the kernels' fp32 value)."""
    seed = np.asarray(seed, dtype=np.uint64)
    row = np.asarray(row, dtype=np.uint64)
    step = np.asarray(step, dtype=np.uint64)
    seed, row, step = np.broadcast_arrays(seed, row, step)
    ctr = np.stack([row & _LO, row >> np.uint64(32), step & _LO, np.full(row.shape, 0x9E3779B9, np.uint64)], -1)
    key = np.stack([seed & _LO, seed >> np.uint64(32)], -1)
    x0 = philox4x32_10(ctr.astype(np.uint32), key.astype(np.uint32))[..., 0]
    return (x0 >> np.uint32(8)).astype(np.float64) / 2.0 ** 24


def greedy_ref(logits):
    """``torch.argmax`` of every row of ``logits`` [N, V] (NaN largest, first index wins) and the gap between the row's
    two largest values (0 for an exact tie, inf for V = 1; NaN when the row holds a NaN or an infinity is involved)."""
    z = np.asarray(logits, dtype=np.float64)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    nan = np.isnan(z)
    token = np.where(nan.any(1), nan.argmax(1), np.argmax(np.where(nan, -np.inf, z), 1))
    if z.shape[1] < 2:
        return token, np.full(z.shape[0], np.inf)
    top2 = -np.sort(-z, 1)[:, :2]  # (NaN sorts last: the gap of a row with a NaN comes out NaN below)
    with np.errstate(invalid="ignore"):
        gap = top2[:, 0] - top2[:, 1]
    gap[nan.any(1)] = np.nan
    return token, gap


def _first_allowed_argmax(z, allowed):
    """First allowed index of the largest value of each row, NaN largest; -1 where no index is allowed."""
    nan = np.isnan(z) & allowed
    masked = np.where(allowed & ~nan, z, -np.inf)
    m = masked.max(1, keepdims=True)
    at_max = allowed & ~nan & (masked == m)
    token = np.where(nan.any(1), nan.argmax(1), at_max.argmax(1))
    return np.where(allowed.any(1), token, -1)


def sample_ref(logits, u, pad, unk, start):
    """The sampled token of every row of ``logits`` [N, V] for uniforms ``u`` [N] (fp64), and its margin: the distance
    from ``u * total`` to the nearest inner boundary of the row's CDF, as a fraction of the total (inf where the choice
    does not depend on ``u``).

    Rule (include/probnmn_hip.h): the allowed tokens are all but pad, unk and start.  A row with no NaN and no +inf and
    a finite allowed logit draws from the softmax over the allowed tokens (weights relative to the largest allowed logit,
    so the allowed total never underflows; -inf entries weigh 0) by inverse CDF in index order.  Otherwise the token is
    the first allowed index with the largest logit, NaN counting as the largest; with no allowed token at all it is the
    greedy choice."""
    z = np.asarray(logits, dtype=np.float64)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    N, V = z.shape
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), (N,))
    allowed = np.ones((N, V), dtype=bool)
    for j in (pad, unk, start):
        if 0 <= j < V:
            allowed[:, j] = False
    token = np.empty(N, dtype=np.int64)
    margin = np.full(N, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(allowed, z, -np.inf).max(1)  # (NaN propagates)
        drawn = ~(np.isnan(z) | (z == np.inf)).any(1) & np.isfinite(m)
    if drawn.any():
        zd, ad = z[drawn], allowed[drawn]
        w = np.where(ad, np.exp(zd - m[drawn, None]), 0.0)
        cdf = np.cumsum(w, 1)
        total = cdf[:, -1:]
        target = u[drawn, None] * total
        # first index with w > 0 whose inclusive prefix sum exceeds the target (the kernels' scan)
        hit = (w > 0) & (cdf > target)
        token[drawn] = hit.argmax(1)
        # inner boundaries: the prefix sums before every positive weight but the first
        pos = w > 0
        first = pos.argmax(1)
        inner = pos & (np.arange(V)[None, :] > first[:, None])
        before = cdf - w
        dist = np.where(inner, np.abs(before - target) / total, np.inf)
        margin[drawn] = dist.min(1)
    rest = ~drawn
    if rest.any():
        t = _first_allowed_argmax(z[rest], allowed[rest])
        g, _ = greedy_ref(z[rest])
        token[rest] = np.where(t >= 0, t, g)
    return token, margin
