"""Host reference of stochastic beam search (``pnmn_attn_lstm_beam_stochastic``, ``decoding_strategy="stochastic_beam"``),
numpy, fp64, vectorised over N independent questions (the importance weights at the end integrate with scipy).

Written from the header's contract (include/probnmn_hip.h, beside ``pnmn_attn_lstm_beam_stochastic``), not from device
output.  Per question, with K slots that carry phi (log-probability) and G (perturbed value):

* start: slot 0 has phi = G = 0, the others -inf; every slot's last token is @start@;
* each step t a hypothesis k that has not finished offers the tokens of ``offered`` (never pad / unk / start; a caller's
  mask or automaton on top); ``lse`` runs over the offered tokens with a finite logit and
  ``phi(k,v) = phi(k) + logit(v) - lse``;
* ``u(k,v) = (2 * (x0 >> 9) + 1) * 2**-24`` with x0 = word 0 of Philox4x32-10 (``tests/token_choice.philox4x32_10``) under
  counter ``{row lo, row hi, t, 0x9E3779B9}`` and key ``{seed lo, seed hi}``, ``row = ((question * 16 + k) * 128 + v``;
* ``g = phi(k,v) - log(-log u)``, ``Z = max g`` over the candidates with a finite phi,
  ``w = G(k) - g + log(1 - exp(g - Z))``, ``G~ = G(k) - max(0, w) - log1p(exp(-|w|))``;
* a finished hypothesis offers only @end@ with phi and G unchanged; a candidate with a non-finite phi or G~ counts as -inf;
* the K largest G~ survive, best first, equal G~ by the smaller flat index k * V + v; a slot left without a finite
  candidate gets (@end@, back-pointer 0, -inf, -inf)."""
import numpy as np

from token_choice import philox4x32_10

NEG = -np.inf
SLOT_STRIDE, TOKEN_STRIDE = 16, 128
_LO = np.uint64(0xFFFFFFFF)


def uniform_from_word(x0):
    """The open uniform of a Philox word: an odd multiple of 2**-24, so 0 < u < 1 exactly in fp32 and fp64."""
    x0 = np.asarray(x0, dtype=np.uint64)
    return (2.0 * (x0 >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def philox_words(seed, row, step):
    """Word 0 of the kernels' Philox stream for (seed, row, step), broadcast against each other (uint64 in, uint32 out)."""
    seed, row, step = np.broadcast_arrays(np.asarray(seed, dtype=np.uint64), np.asarray(row, dtype=np.uint64),
                                          np.asarray(step, dtype=np.uint64))
    ctr = np.stack([row & _LO, row >> np.uint64(32), step & _LO, np.full(row.shape, 0x9E3779B9, np.uint64)], -1)
    key = np.stack([seed & _LO, seed >> np.uint64(32)], -1)
    return philox4x32_10(ctr.astype(np.uint32), key.astype(np.uint32))[..., 0]


def uniforms(seed, question, K, V, t):
    """u [N, K, V] of step ``t`` for seeds ``seed`` [N] (or one) and global question indices ``question`` [N]."""
    question = np.asarray(question, dtype=np.uint64).reshape(-1, 1, 1)
    seed = np.asarray(seed, dtype=np.uint64).reshape(-1, 1, 1)
    k = np.arange(K, dtype=np.uint64).reshape(1, K, 1)
    v = np.arange(V, dtype=np.uint64).reshape(1, 1, V)
    row = (question * np.uint64(SLOT_STRIDE) + k) * np.uint64(TOKEN_STRIDE) + v
    return uniform_from_word(philox_words(seed, row, t))


def log1mexp(d):
    """log(1 - exp(d)) for d <= 0 without cancellation (-inf at d = 0)."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(d > -np.log(2.0), np.log(-np.expm1(d)), np.log1p(-np.exp(d)))


def gumbel(phi_c, u):
    """g = phi - log(-log u) where phi is finite, -inf elsewhere."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(phi_c), phi_c - np.log(-np.log(u)), NEG)


def candidates(phi, G, finished, logits, offered, u, end):
    """One step's candidate tables (phi(k,v), G~(k,v)), [N, K, V] each, from the slots' phi, G, finished [N, K], the
    logits and the offered mask [N, K, V] and the uniforms ``u`` [N, K, V]."""
    phi, G = np.asarray(phi, dtype=np.float64), np.asarray(G, dtype=np.float64)
    logits = np.asarray(logits, dtype=np.float64)
    finished = np.asarray(finished, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inside = np.asarray(offered, dtype=bool) & np.isfinite(logits) & ~finished[..., None]
        z = np.where(inside, logits, NEG)
        mx = z.max(-1, keepdims=True)
        lse = mx + np.log(np.exp(z - np.where(np.isfinite(mx), mx, 0.0)).sum(-1, keepdims=True))
        phi_c = np.where(inside, phi[..., None] + (logits - lse), NEG)
        phi_c = np.where(np.isfinite(phi_c), phi_c, NEG)
        g = gumbel(phi_c, u)
        Z = g.max(-1, keepdims=True)
        w = G[..., None] - g + log1mexp(g - Z)
        gt = G[..., None] - np.maximum(0.0, w) - np.log1p(np.exp(-np.abs(w)))
        ok = np.isfinite(phi_c) & np.isfinite(gt)
        phi_c, gt = np.where(ok, phi_c, NEG), np.where(ok, gt, NEG)
        keep = finished & np.isfinite(phi) & np.isfinite(G)  # a finished hypothesis: @end@ alone, phi and G unchanged
        phi_c[..., end] = np.where(keep, phi, phi_c[..., end])
        gt[..., end] = np.where(keep, G, gt[..., end])
    return phi_c, gt


def select(phi_c, gt, K, end):
    """The K largest G~ of every question, best first, equal values by the smaller flat index:
    (token, back-pointer, phi, G), [N, K] each."""
    N, _, V = gt.shape
    flat_g, flat_p = gt.reshape(N, -1), phi_c.reshape(N, -1)
    order = np.argsort(-flat_g, axis=1, kind="stable")[:, :K]
    G = np.take_along_axis(flat_g, order, 1)
    phi = np.take_along_axis(flat_p, order, 1)
    ok = G > NEG
    tok = np.where(ok, order % V, end)
    bp = np.where(ok, order // V, 0)
    return tok, bp, np.where(ok, phi, NEG), np.where(ok, G, NEG)


def table_logits(table, V):
    """A ``prefixes -> logits`` callable from a mapping {prefix tuple: logits [V]} (a missing prefix: all -inf)."""
    def fn(prefixes):
        out = np.full(prefixes.shape[:-1] + (V,), NEG)
        for idx in np.ndindex(*prefixes.shape[:-1]):
            row = table.get(tuple(int(x) for x in prefixes[idx]))
            if row is not None:
                out[idx] = row
        return out
    return fn


def search(logits, K, T, V, seed, question, end, pad=-1, unk=-1, start=-1, allowed=None):
    """Stochastic beam search of N questions.  ``logits``: a callable ``prefixes [N, K, t] -> [N, K, V]`` or a mapping
    {prefix tuple: logits [V]}; ``seed`` [N] or one; ``question`` [N]: the global index (question_offset + b);
    ``allowed(prefixes, t) -> bool [N, K, V]``: a caller's mask on top of "never pad / unk / start".
    Returns tokens [N, K, T], phi [N, K], G [N, K] and the per-step trace (token, back-pointer, phi, G, [N, T, K] each)
    plus ``trace_gumbel_argmax`` [N, T, K]: per parent slot the arg-max token of g (-1 where nothing was offered)."""
    if not callable(logits):
        logits = table_logits(logits, V)
    question = np.asarray(question).reshape(-1)
    N = question.shape[0]
    prefixes = np.zeros((N, K, 0), dtype=np.int64)
    phi = np.full((N, K), NEG)
    phi[:, 0] = 0.0
    G = phi.copy()
    finished = np.zeros((N, K), dtype=bool)
    base = np.ones(V, dtype=bool)
    for j in (pad, unk, start):
        if 0 <= j < V:
            base[j] = False
    trace = {k: [] for k in ("tokens", "backpointers", "scores", "perturbed", "gumbel_argmax")}
    for t in range(T):
        z = logits(prefixes)
        offered = np.broadcast_to(base, (N, K, V))
        if allowed is not None:
            offered = offered & allowed(prefixes, t)
        u = uniforms(seed, question, K, V, t)
        phi_c, gt = candidates(phi, G, finished, z, offered, u, end)
        live = np.isfinite(phi_c) & ~finished[..., None]
        g = gumbel(np.where(live, phi_c, NEG), u)
        trace["gumbel_argmax"].append(np.where(live.any(-1), g.argmax(-1), -1))
        tok, bp, phi, G = select(phi_c, gt, K, end)
        prefixes = np.concatenate([np.take_along_axis(prefixes, bp[..., None], 1), tok[..., None]], -1)
        finished = tok == end
        for key, value in (("tokens", tok), ("backpointers", bp), ("scores", phi), ("perturbed", G)):
            trace[key].append(value)
    out = {"tokens": prefixes, "phi": phi, "G": G}
    out.update({"trace_" + k: np.stack(v, 1) for k, v in trace.items()})
    return out


def without_replacement_log_weights(phi, G):
    """fp64 statement of ``evaluators.without_replacement_weights`` by direct numerical integration (scipy): rows best first,
    kappa = G of the last slot, which gets -inf; kappa = -inf: log w_i = phi_i.  Otherwise the paper's p_i / q_i(kappa'),
    q_i(k) = 1 - exp(-exp(phi_i - k)), averaged over the root's free value -- the search conditions its G on the largest being
    0; with E ~ Exp(1) the unconditioned threshold is exp(-kappa') = E + exp(-kappa) - 1:

        w_i = p_i  int_0^inf exp(-x) / (1 - exp(-p_i (x + c))) dx,      c = exp(-kappa) - 1,  p_i = exp(phi_i)."""
    from scipy.integrate import quad

    phi, G = np.asarray(phi, dtype=np.float64), np.asarray(G, dtype=np.float64)
    out = np.full(phi.shape, NEG)
    for b in range(phi.shape[0]):
        kappa = G[b, -1]
        for i in range(phi.shape[1] - 1):
            if not np.isfinite(phi[b, i]):
                continue
            if kappa == NEG:
                out[b, i] = phi[b, i]
                continue
            p, c = np.exp(phi[b, i]), np.expm1(-kappa)
            value = sum(quad(lambda x: np.exp(-x) / -np.expm1(-p * (x + c)), lo, hi, epsabs=0.0, epsrel=1e-13, limit=400)[0]
                        for lo, hi in ((0.0, 1.0), (1.0, 8.0), (8.0, 40.0), (40.0, np.inf)))
            out[b, i] = phi[b, i] + np.log(value)
    return out


def chi_square_quantile(df, z=4.753424308822899):
    """The 1 - 1e-6 quantile of chi-square with ``df`` degrees of freedom (``z``: that quantile of the standard normal):
    scipy's when it is installed, else Wilson-Hilferty."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        return df * (1.0 - 2.0 / (9.0 * df) + z * np.sqrt(2.0 / (9.0 * df))) ** 3
