"""``pnmn_importance_bound_joint`` and what is built on it, on the MI355X: the kernel against the fp64 reference of
tests/helpers/importance_joint_reference.py over every sample count, vocabulary width and number of answers at which it takes
another path, with a sample that dominates through its ANSWER logit (the cancellation case of the leave-one-out terms),
questions a single row rules out -- by a token, by an answer that is no index, by a -inf answer logit, by an invalid program
-- and invalid programs that answer uniformly; guard words around every output; the bits it shares with
``pnmn_importance_bound``, between its two modes, between a question alone and in a batch and between ``valid`` NULL and all
ones; ``joint_importance_weighted_bound`` under autograd; one ``ImportanceWeightedJointStep`` and ``evaluate_joint_evidence``
on small models.

Tolerances -- derived as in tests/test_importance_bound_gpu.py, not measured.  The three sequence terms and ``log_pa``: rtol =
atol = 1e-5, the project's bar for log-softmax sums (``log_pa`` is one such term of one step).  log w combines the four sums
and inherits their ABSOLUTE errors: tol_g = 1e-5 (1 + max over the question's rows of |lx| + gamma |la| + beta (|lp| +
|lq|)), for ``log_weight`` and ``bound``; ``signal`` and ``share`` 2 tol_g, ``ess`` 4 tol_g relative, by the arguments given
there.  Gradients, coefficient x ce with |ce| <= 1 -- the answer's coefficient is gamma share, within 2 tol_g for gamma <= 1
--: |got - ref| <= 3 tol_g + 1e-5 |coefficient| per element.  -inf / finite patterns, ``support`` and ``row_predictions`` are
compared exactly; the latter on inputs whose every row holds its largest logit at least 1e-3 above the next (asserted on the
reference), so that the arg-max does not depend on rounding.

One launch has ONE ``invalid_log_answer``, so every case is launched in two configurations of the same x / p / q / answer
inputs.  RULED: ``invalid_log_answer`` = -inf and one invalid row among the marked questions g = 3 (mod 8), whose causes are, in
turn, a token that is no index (in x, p or q by the case), an answer that is no index, a -inf logit at the answer and that
invalid row: exactly these five questions are unsupported.  UNIFORM: the default -log A, the same invalid row and one more in
every question g = 5 (mod 8): those questions count, with a zero d_a row, and four of the five marked ones stay ruled out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from importance_joint_reference import importance_joint_reference  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)
GUARD = 64          # guard words on either side of every output buffer
SENTINEL = -777.0
G = 37
TX, TP, TQ = 5, 4, 3
PAD = 0
UNKNOWN = 1         # the prediction reported for an invalid row
MARKED = [g for g in range(G) if g % 8 == 3]
UNIFORM = [g for g in range(G) if g % 8 == 5]
LIFTED = [g for g in range(G) if g % 8 == 1]
CAUSES = ("token", "answer", "logit", "invalid", "token")
# (K, (Vx, Vq), A): every K of tests/test_importance_bound_gpu.py's SAMPLES, widths out of its WIDTHS that cover every register
# count of with_nper (1, 2, 4, 8, 16), every A of {2, 28, 64, 65, 257, 1024}; in the last four A alone is the widest vocabulary
CASES = [(1, (3, 2), 2), (2, (64, 45), 28), (3, (65, 64), 64), (8, (130, 129), 65), (9, (257, 256), 257), (64, (513, 512), 28),
         (3, (1024, 1023), 1024), (64, (65, 64), 2), (9, (3, 2), 1024), (8, (64, 45), 65), (2, (65, 64), 257), (1, (130, 129), 1024)]


def make_inputs(K, Vx, Vq, A, seed=0, Tx=TX):
    """37 questions of K rows in tests/test_importance_bound_gpu.py's scheme: logits x 3, a tenth of the rows x 8, a quarter of
    the tokens padding, some rows all padding; answer logits x 3 with a few -inf beside the answer.  Returns (x, q, p, (answer
    logits, answers), the marked rows' causes, valid per configuration).
    g = 1 (mod 8): the question's rows share one program (x / p / q of its first row), one of them holds the answer 40 above
    its other logits and the others hold it 25 below theirs: that sample's log w leads by 25 nats and more through the answer
    alone.  g = 3 (mod 8): one row ruled out, by CAUSES in turn.  g = 5 (mod 8): one row invalid in the UNIFORM configuration."""
    rng = np.random.default_rng(100000 * Vx + 1000 * K + 10 * Tx + A + seed)
    R = G * K

    def term(T, V):
        logits = (rng.standard_normal((R, T, V)) * 3).astype(np.float32)
        logits[rng.random(R) < 0.1] *= 8
        tokens = rng.integers(1, V, (R, T)).astype(np.int64)
        tokens[rng.random((R, T)) < 0.25] = PAD
        tokens[rng.random(R) < 0.06] = PAD
        return [logits, tokens, PAD]

    x, p, q = term(Tx, Vx), term(TP, Vq), term(TQ, Vq)
    x[1][R - 1], q[1][0] = PAD, PAD                      # (rows that are all padding, whatever the draw)
    a_logits = (rng.standard_normal((R, A)) * 3).astype(np.float32)
    answers = rng.integers(0, A, G).astype(np.int64)
    row_answers = np.repeat(answers, K)
    for r in range(0, R, 7):                             # a -inf beside the answer: probability 0, gradient exactly 0
        a_logits[r, (row_answers[r] + 1) % A] = -np.inf if A > 2 else a_logits[r, (row_answers[r] + 1) % A]
    for g in LIFTED:
        rows = slice(g * K, (g + 1) * K)
        for t in (x, p, q):
            t[0][rows], t[1][rows] = t[0][g * K], t[1][g * K]
        finite = np.where(np.isfinite(a_logits[rows]), a_logits[rows], 0.0)
        a_logits[rows, answers[g]] = finite.min(1) - 25.0
        lifted = g * K + int(rng.integers(0, K))
        a_logits[lifted, answers[g]] = np.abs(finite[lifted - g * K]).max() + 40.0
    causes = {}
    valid = {"ruled": np.ones(R, np.int32), "uniform": np.ones(R, np.int32)}
    for i, g in enumerate(MARKED):
        r = g * K + int(rng.integers(0, K))
        causes[g] = (CAUSES[i], r)
        if CAUSES[i] == "token":                         # x, p or q: by the case and the question
            logits, tokens, _ = (x, p, q)[(i + K + A) % 3]
            t = int(rng.integers(0, tokens.shape[1]))
            tokens[r, t] = logits.shape[2] + 3 if (i + K) % 2 else -2
        elif CAUSES[i] == "answer":                      # no index, and no padding value either: every row of the question
            answers[g] = (A, -1, -2, A + 5, 1 << 40)[(K + A) % 5]
        elif CAUSES[i] == "logit":
            a_logits[r, answers[g]] = -np.inf
        else:
            valid["ruled"][r] = valid["uniform"][r] = 0
            a_logits[r] = np.nan                         # (an invalid row's logits are not read)
    for g in UNIFORM:
        valid["uniform"][g * K + int(rng.integers(0, K))] = 0
    # every row's largest logit leads the next by 1 and more: the arg-max does not depend on rounding
    for r in range(R):
        if not np.isnan(a_logits[r]).any():
            a_logits[r, int(np.argmax(a_logits[r]))] += 1.0
    return tuple(x), tuple(q), tuple(p), (a_logits, answers), causes, valid


def launch(x, q, p, answer, beta, K, gamma=1.0, invalid=None, grad=(False, False, False, False), optional=True):
    """One ``pnmn_importance_bound_joint`` launch on numpy inputs; every output lies between GUARD sentinel words, which must
    come back untouched, and is itself filled with the sentinel first.  The token rows are handed over with a stride wider
    than T.  ``answer`` = (logits, answers, valid or None); ``grad`` = which of d_x / d_p / d_q / d_a are asked for;
    ``optional`` False: every optional output is left out.  Returns the outputs as numpy."""
    from probnmn import _hip, _hip_importance_joint

    dev = torch.device("cuda:0")
    R = len(x[0])
    n = R // K
    keep = []

    def term(t):
        if t is None:
            return [0, 0, 0, 0, 0, 0], 1
        logits, tokens, pad = t
        wide = torch.full((R, tokens.shape[1] + 2), 12345, dtype=torch.long)
        wide[:, :tokens.shape[1]] = torch.from_numpy(np.ascontiguousarray(tokens))
        d_logits, d_tokens = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev), wide.to(dev)
        keep.extend((d_logits, d_tokens))
        return [d_logits.data_ptr(), d_tokens.data_ptr(), wide.stride(0), pad, logits.shape[1], logits.shape[2]], logits[0].size

    (x_args, x_words), (p_args, p_words), (q_args, q_words) = term(x), term(p), term(q)
    a_logits, answers, valid = answer
    A = a_logits.shape[1]
    d_a_logits = torch.from_numpy(np.ascontiguousarray(a_logits, np.float32)).to(dev)
    d_answers = torch.from_numpy(np.ascontiguousarray(answers, np.int64)).to(dev)
    d_valid = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.int32)).to(dev)
    f32 = lambda size: torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
    bufs = {name: f32(R) for name in ("log_px", "log_pz", "log_q", "log_pa", "log_weight", "share", "signal")}
    bufs.update(bound=f32(n), ess=f32(n), support=torch.full((n + 2 * GUARD,), int(SENTINEL), dtype=torch.int32, device=dev),
                row_predictions=torch.full((R + 2 * GUARD,), int(SENTINEL), dtype=torch.long, device=dev))
    for name, want, words in zip(("d_x", "d_p", "d_q", "d_a"), grad, (x_words, p_words, q_words, A)):
        if want:
            bufs[name] = f32(R * words)
    ptr = lambda name: bufs[name][GUARD:].data_ptr() if name in bufs else 0  # noqa: E731
    opt = lambda name: ptr(name) if optional else 0  # noqa: E731
    rc = _hip_importance_joint.lib().pnmn_importance_bound_joint(
        *x_args, *p_args, *q_args, float(beta), n, K, opt("log_px"), opt("log_pz"), opt("log_q"), ptr("log_weight"), ptr("share"),
        ptr("signal"), ptr("bound"), opt("ess"), opt("support"), ptr("d_x"), ptr("d_p"), ptr("d_q"), d_a_logits.data_ptr(),
        0 if d_valid is None else d_valid.data_ptr(), d_answers.data_ptr(), A, float(gamma),
        float(-np.log(A) if invalid is None else invalid), UNKNOWN, opt("log_pa"), opt("row_predictions"), ptr("d_a"),
        _hip.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), name
        out[name] = host[GUARD:-GUARD]
    for name, shape in (("d_x", x[0].shape), ("d_p", None if p is None else p[0].shape), ("d_q", q[0].shape), ("d_a", a_logits.shape)):
        if name in out:
            out[name] = out[name].reshape(shape)
    return out


OPTIONAL = ("log_px", "log_pz", "log_q", "log_pa", "ess", "support", "row_predictions")


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b, names=None, rows=None):
    for name in names if names is not None else a:
        left, right = (a[name], b[name]) if rows is None else (a[name][rows[0]], b[name][rows[1]])
        assert np.array_equal(bits(np.ascontiguousarray(left)), bits(np.ascontiguousarray(right))), name


def check_against_reference(got, ref, x, q, p, answer, K, label=""):
    tol_g = 1e-5 * (1.0 + ref["scale"])
    tol_r = np.repeat(tol_g, K)
    counts = ref["support"] == K
    rows = np.repeat(counts, K)
    for name in ("log_px", "log_pz", "log_q", "log_pa"):
        if ref[name] is None:
            assert (got[name] == SENTINEL).all(), name          # (a term that is left out is not written)
            continue
        inf = np.isneginf(ref[name])
        assert np.array_equal(np.isneginf(got[name]), inf) and not np.isnan(got[name]).any(), name
        np.testing.assert_allclose(got[name][~inf], ref[name][~inf], err_msg=name, **TOL)
    assert np.array_equal(got["support"], ref["support"])
    assert np.array_equal(got["row_predictions"], ref["row_predictions"])
    fin = np.isfinite(ref["log_weight"])
    assert np.array_equal(np.isfinite(got["log_weight"]), fin) and np.isneginf(got["log_weight"][~fin]).all()
    worst = {"log_weight": (np.abs(got["log_weight"][fin] - ref["log_weight"][fin]) / tol_r[fin]).max(),
             "bound": (np.abs(got["bound"][counts] - ref["bound"][counts]) / tol_g[counts]).max(),
             "signal": (np.abs(got["signal"] - ref["signal"]) / (2 * tol_r)).max(),
             "share": (np.abs(got["share"] - ref["share"]) / (2 * tol_r)).max(),
             "ess": (np.abs(got["ess"][counts] - ref["ess"][counts]) / (4 * tol_g[counts] * ref["ess"][counts])).max()}
    assert np.isneginf(got["bound"][~counts]).all() and (got["ess"][~counts] == 0).all()
    assert (got["share"][~rows] == 0).all() and (got["signal"][~rows] == 0).all()
    a_logits, answers, valid = answer
    for name, term in (("d_x", x), ("d_p", p), ("d_q", q), ("d_a", None)):
        if name not in got:
            continue
        d, want, c = got[name], ref[name], np.abs(ref["coefficient_" + name[-1]])
        assert not (bits(d) == bits(np.float32(SENTINEL))).any(), name        # every word was written
        assert (d[~rows] == 0).all(), name                                     # unsupported questions: zeros
        if term is not None:
            scored = (term[1] != term[2]) & (term[1] >= 0) & (term[1] < term[0].shape[2])
            assert (d[~scored] == 0).all(), name                               # padding steps: zeros
            bar = (3 * tol_r + 1e-5 * c)[:, None, None]
        else:
            if valid is not None:
                assert (d[valid == 0] == 0).all()                              # invalid rows: zeros
            assert (d[np.isneginf(a_logits) & ~np.isnan(a_logits)] == 0).all()  # a logit of -inf gets exactly 0
            bar = (3 * tol_r + 1e-5 * c)[:, None]
        worst[name] = (np.abs(d - want) / bar).max()
    print("%s largest error / tolerance: %s" % (label, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def conditions(ref, a_logits, answers, valid, causes, K, ruled):
    """What the inputs are required to hold, on the fp64 reference alone: which questions are unsupported, the lead of the
    lifted sample, the margin of every arg-max."""
    out = [g for g in MARKED if ruled or causes[g][0] != "invalid"]
    assert len(MARKED) == 5 and sorted(c for c, _ in causes.values()) == sorted(CAUSES) and len(out) == (5 if ruled else 4)
    want = [K if g not in out else 0 if causes[g][0] == "answer" else K - 1 for g in range(G)]
    assert ref["support"].tolist() == want                                   # exactly the marked questions, and no other
    if K > 1:
        lw = np.sort(ref["log_weight"].reshape(G, K)[LIFTED], axis=1)
        print("lifted questions: the largest log w leads the next by %.1f .. %.1f nats" % ((lw[:, -1] - lw[:, -2]).min(), (lw[:, -1] - lw[:, -2]).max()))
        assert (lw[:, -1] - lw[:, -2] >= 25.0).all()    # one sample dominates, through its answer logit alone
        la = ref["log_pa"].reshape(G, K)[LIFTED]
        assert np.allclose(np.sort(la, 1)[:, -1] - np.sort(la, 1)[:, -2], lw[:, -1] - lw[:, -2], rtol=0, atol=1e-9)
    top = np.sort(np.where(np.isnan(a_logits), -np.inf, a_logits.astype(np.float64)), axis=1)
    read = valid != 0
    assert (top[read, -1] - top[read, -2] >= 1e-3).all() and np.isfinite(top[read, -1]).all()
    if not ruled:
        assert len(UNIFORM) == 4 and all((valid.reshape(G, K)[g] == 0).sum() == 1 for g in UNIFORM)


def run_case(K, Vx, Vq, A, beta=1.0, gamma=1.0, Tx=TX, prior=True):
    x, q, p, (a_logits, answers), causes, valids = make_inputs(K, Vx, Vq, A, Tx=Tx)
    p = p if prior else None
    assert all((t[1] == PAD).all(1).any() and (t[1] == PAD).mean() > 0.15 for t in (x, q))
    grads = (True, p is not None, True, True)
    results = {}
    for name, invalid in (("ruled", -np.inf), ("uniform", None)):
        answer = (a_logits, answers, valids[name])
        ref = importance_joint_reference(x, q, p, beta, K, answer, answer_weight=gamma, invalid_log_answer=invalid,
                                         unknown_index=UNKNOWN, gradients=True)
        if beta == 1.0 and prior and gamma == 1.0:
            conditions(ref, a_logits, answers, valids[name], causes, K, name == "ruled")
        got = launch(x, q, p, answer, beta, K, gamma=gamma, invalid=invalid, grad=grads)
        check_against_reference(got, ref, x, q, p, answer, K, "K = %d, V = (%d, %d), A = %d, %s:" % (K, Vx, Vq, A, name))
        # the plain launch: the outputs the two modes share are the same bits
        same_bits(launch(x, q, p, answer, beta, K, gamma=gamma, invalid=invalid), got, [n for n in got if not n.startswith("d_")])
        results[name] = (answer, got)
    return x, q, p, results


@pytest.mark.parametrize("K,V,A", CASES)
def test_kernel_against_fp64_reference(K, V, A):
    run_case(K, *V, A)


def test_second_block_of_steps():
    run_case(3, 3, 2, 28, Tx=70)  # (the tokens are read 64 at a time: steps 64 .. 69 are the second block)


@pytest.mark.parametrize("beta,gamma,prior", [(0.1, 0.5, True), (0.0, 1.0, True), (1.0, 0.25, False)])
def test_other_weights_and_terms_left_out(beta, gamma, prior):
    run_case(9, 65, 64, 28, beta=beta, gamma=gamma, prior=prior)


def test_zero_answer_weight_is_the_question_only_entry_point_bit_for_bit():
    """gamma = 0: the answer term is left out entirely -- no row is ruled out by it, no 0 x -inf is formed -- and every output
    the two entry points share, gradients included, is the same bits; log_pa and row_predictions are still reported."""
    from test_importance_bound_gpu import launch as bound_launch

    for K, V, A in ((9, (65, 64), 28), (2, (1024, 1023), 1024), (64, (3, 2), 257), (1, (130, 129), 2)):
        x, q, p, (a_logits, answers), causes, valids = make_inputs(K, *V, A)
        answer = (a_logits, answers, valids["ruled"])
        for beta, prior in ((1.0, p), (0.0, p), (0.5, None)):
            grads = (True, prior is not None, True)
            theirs = bound_launch(x, q, prior, beta, K, grad=grads)
            got = launch(x, q, prior, answer, beta, K, gamma=0.0, invalid=-np.inf, grad=grads + (True,))
            same_bits(theirs, got)
            assert (got["d_a"] == 0).all()
            ref = importance_joint_reference(x, q, prior, beta, K, answer, answer_weight=1.0, invalid_log_answer=-np.inf, unknown_index=UNKNOWN)
            assert np.array_equal(got["row_predictions"], ref["row_predictions"])
            assert np.array_equal(np.isneginf(got["log_pa"]), np.isneginf(ref["log_pa"])) and not np.isnan(got["log_pa"]).any()
            plain = launch(x, q, prior, answer, beta, K, gamma=0.0, invalid=-np.inf)
            same_bits(bound_launch(x, q, prior, beta, K), plain, [n for n in theirs if not n.startswith("d_")])
            same_bits(plain, got, ("log_pa", "row_predictions"))


def test_a_question_is_the_same_bits_alone_and_in_a_batch():
    for K, V, A in ((9, (65, 64), 28), (64, (130, 129), 65), (1, (64, 45), 1024)):
        x, q, p, (a_logits, answers), causes, valids = make_inputs(K, *V, A)
        valid = valids["uniform"]
        for grad in ((True, True, True, True), (False, False, False, False)):
            whole = launch(x, q, p, (a_logits, answers, valid), 1.0, K, grad=grad)
            same_bits(whole, launch(x, q, p, (a_logits, answers, valid), 1.0, K, grad=grad))
            for g in (0, 1, 3, 5, 9, 11, 19, 20, 27, 35, 36):
                lo, hi = g * K, (g + 1) * K
                cut = lambda t: (t[0][lo:hi], t[1][lo:hi], t[2])  # noqa: E731
                alone = launch(cut(x), cut(q), cut(p), (a_logits[lo:hi], answers[g:g + 1], valid[lo:hi]), 1.0, K, grad=grad)
                per_row = [n for n in alone if n not in ("bound", "ess", "support")]
                same_bits(alone, whole, per_row, rows=(slice(None), slice(lo, hi)))
                same_bits(alone, whole, ("bound", "ess", "support"), rows=(slice(0, 1), slice(g, g + 1)))


def test_valid_null_is_all_ones_and_left_out_outputs_change_nothing():
    K, V, A = 8, (257, 256), 64
    x, q, p, (a_logits, answers), causes, valids = make_inputs(K, *V, A)
    a_logits = np.where(np.isnan(a_logits), np.float32(0.5), a_logits)      # (every row is read now)
    ones = np.ones(G * K, np.int32)
    for grad in ((True, True, True, True), (False, False, False, False), (False, False, False, True)):
        with_ones = launch(x, q, p, (a_logits, answers, ones), 1.0, K, grad=grad)
        same_bits(with_ones, launch(x, q, p, (a_logits, answers, None), 1.0, K, grad=grad))
        bare = launch(x, q, p, (a_logits, answers, ones), 1.0, K, grad=grad, optional=False)
        assert all((bare[name] == int(SENTINEL)).all() for name in OPTIONAL)      # (left out: nothing written for them)
        same_bits(bare, with_ones, [n for n in bare if n not in OPTIONAL])
    # the answer's gradient alone is gradient mode: the other outputs are the plain launch's bits
    same_bits(launch(x, q, p, (a_logits, answers, ones), 1.0, K), with_ones, [n for n in with_ones if n != "d_a"])


def test_more_answers_than_the_widest_kernel_holds_returns_without_a_launch():
    from probnmn import _hip, _hip_importance_joint

    dev = torch.device("cuda:0")
    out = torch.full((2 * 3 * 1025,), SENTINEL, device=dev)
    a = out.data_ptr()
    for Vx, Vp, Vq, A in ((4, 4, 4, 1025), (4, 4, 4, 1 << 20), (1025, 4, 4, 4), (4, 1025, 4, 4), (4, 4, 1025, 4)):
        rc = _hip_importance_joint.lib().pnmn_importance_bound_joint(
            a, a, 3, 0, 3, Vx, a, a, 3, 0, 3, Vp, a, a, 3, 0, 3, Vq, 1.0, 1, 2, 0, 0, 0, a, a, a, a, 0, 0, 0, 0, 0,
            a, 0, a, A, 1.0, -1.0, 0, a, a, 0, _hip.stream_ptr(dev))
        assert rc == _hip.ESHAPE
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()  # nothing ran


# ---- under autograd ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modules_need_grad", [True, False])
def test_joint_importance_weighted_bound_under_autograd(modules_need_grad):
    from probnmn.models.nmn import INVALID_PROGRAM_LOSS
    from probnmn.modules.importance_weighted import joint_importance_weighted_bound

    dev = torch.device("cuda:0")
    K, beta, gamma, A = 3, 0.5, 0.75, 28
    x, q, p, (a_logits, answers), causes, valids = make_inputs(K, 65, 64, A)
    valid = valids["uniform"]
    ref = importance_joint_reference(x, q, p, beta, K, (a_logits, answers, valid), answer_weight=gamma, unknown_index=UNKNOWN, gradients=True)

    def on_device(t, needs_grad):
        return (torch.from_numpy(t[0]).to(dev).requires_grad_(needs_grad), torch.from_numpy(t[1]).to(dev), t[2])

    def answer_on_device(needs_grad):
        return (torch.from_numpy(a_logits).to(dev).requires_grad_(needs_grad), torch.from_numpy(answers).to(dev), torch.from_numpy(valid).to(dev))

    dx, dq, dp, da = on_device(x, True), on_device(q, True), on_device(p, False), answer_on_device(modules_need_grad)
    loss, stats = joint_importance_weighted_bound(dx, dq, dp, answer=da, samples=K, beta=beta, answer_weight=gamma, unknown_index=UNKNOWN)
    assert set(stats) == {"log_weight", "share", "signal", "ess", "support", "log_px", "log_pz", "log_q", "log_pa", "row_predictions"}
    assert not any(v.requires_grad for v in stats.values()) and loss.requires_grad and loss.shape == (G,)
    saved = loss.grad_fn.saved_tensors      # d_x, d_p, d_q, d_a: no buffer unasked
    assert saved[0] is not None and saved[1] is None and saved[2] is not None and (saved[3] is not None) == modules_need_grad
    counts = ref["support"] == K
    assert 0 < (~counts).sum() < G
    tol_g = 1e-5 * (1.0 + ref["scale"])
    host = loss.detach().cpu().numpy()
    assert (host[~counts] == np.float32(INVALID_PROGRAM_LOSS)).all()       # a question without full support pays the constant
    assert (np.abs(-host[counts] - ref["bound"][counts]) <= tol_g[counts]).all()
    assert np.array_equal(stats["support"].cpu().numpy(), ref["support"])
    assert np.array_equal(stats["row_predictions"].cpu().numpy(), ref["row_predictions"])
    # a dloss per question, not uniform
    weights = np.linspace(0.5, 2.0, G)
    (loss * torch.from_numpy(weights).to(dev, torch.float32)).sum().backward()
    tol_r, scale = np.repeat(tol_g, K), np.repeat(weights, K)
    for name, t in (("x", dx), ("q", dq), ("p", dp), ("a", da)):
        if t[0].grad is None:
            assert name == "p" or (name == "a" and not modules_need_grad)
            continue
        got = t[0].grad.cpu().numpy()
        shape = (-1,) + (1,) * (got.ndim - 1)
        bar = (scale * (3 * tol_r + 1e-5 * np.abs(ref["coefficient_" + name]))).reshape(shape)
        assert (np.abs(got - scale.reshape(shape) * ref["d_" + name]) <= bar).all(), name
        assert (got[np.repeat(~counts, K)] == 0).all()                     # ... and gets no gradient
    assert modules_need_grad == (da[0].grad is not None)
    if modules_need_grad:
        assert (da[0].grad[torch.from_numpy(valid == 0).to(dev)] == 0).all()
    # nothing requires a gradient: the plain launch, the same bits
    plain, plain_stats = joint_importance_weighted_bound(on_device(x, False), on_device(q, False), on_device(p, False),
                                                         answer=answer_on_device(False), samples=K, beta=beta, answer_weight=gamma,
                                                         unknown_index=UNKNOWN)
    assert not plain.requires_grad and torch.equal(plain, loss.detach())
    for name in stats:
        assert torch.equal(plain_stats[name], stats[name]), name


# ---- the models ------------------------------------------------------------------------------------------------------------

def _models(dev, seed=0):
    from probnmn.models import NeuralModuleNetwork, ProgramGenerator, ProgramPrior, QuestionReconstructor
    from probnmn.vocabulary import Vocabulary

    vocab = Vocabulary.clevr()
    torch.manual_seed(seed)
    pg, qr = ProgramGenerator(vocab).to(dev), QuestionReconstructor(vocab).to(dev)
    prior = ProgramPrior(vocab, hidden_size=256).to(dev)
    nmn = NeuralModuleNetwork(vocab, class_projection_channels=128, classifier_linear_size=32).to(dev)
    return vocab, pg, qr, prior, nmn


def _constraint(vocab, pg):
    from probnmn.runtime.program_compiler import ProgramCompiler

    compiler = ProgramCompiler(vocab.get_index_to_token_vocabulary("programs"))
    exclude = [getattr(pg, n) for n in ("_pad_index", "_unk_index", "_start_index", "_end_index")]
    return compiler, compiler.decoding_automaton(exclude=exclude)


def _parameters(*models):
    return [[p.detach().clone() for p in m.parameters()] for m in models]


def _moved(before, *models):
    return [any(not torch.equal(a, b) for a, b in zip(old, m.parameters())) for old, m in zip(before, models)]


@pytest.mark.parametrize("train_modules", [True, False])
def test_one_importance_weighted_joint_step(train_modules):
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.trainers import ImportanceWeightedJointStep

    dev = torch.device("cuda:0")
    vocab, pg, qr, prior, nmn = _models(dev, seed=1)
    compiler, automaton = _constraint(vocab, pg)
    batch = synthetic_batch(vocab, 8, seed=31)
    supervision = torch.tensor([1, 1, 0, 0, 0, 1, 0, 1])
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    dbatch["supervision"] = supervision
    before = _parameters(pg, qr, prior, nmn)
    K, alpha = 2, 100.0
    step = ImportanceWeightedJointStep(pg, qr, prior, nmn, num_samples=K, beta=1.0, answer_weight=1.0, alpha=alpha,
                                       constraint=automaton, train_modules=train_modules)
    torch.manual_seed(3)
    out = step.step(dbatch)
    torch.cuda.synchronize()
    for key in ("objective", "bound", "effective_sample_size", "signal_variance", "unsupported", "programs", "samples_per_question",
                "loss", "answer_accuracy", "posterior_answer_accuracy", "invalid_rows"):
        assert key in out, key
    assert out["samples_per_question"] == K and out["programs"].shape[0] == 4 * K
    assert int(out["unsupported"]) == 0 and int(out["invalid_rows"]) == 0
    assert all(c.valid for c in compiler.compile_batch(out["programs"].cpu().numpy()))
    values = [out[k] for k in ("objective", "bound", "effective_sample_size", "signal_variance", "answer_accuracy",
                               "posterior_answer_accuracy")] + list(out["loss"].values())
    assert all(torch.isfinite(v).all() for v in values)
    assert 1.0 <= float(out["effective_sample_size"]) <= K and float(out["signal_variance"]) >= 0.0
    assert 0.0 <= float(out["answer_accuracy"]) <= 1.0 and 0.0 <= float(out["posterior_answer_accuracy"]) <= 1.0 + 1e-6
    # the objective is the two terms it reports: alpha x the supervised cross entropies, minus the mean bound
    want = alpha * (float(out["loss"]["program_generation_gt"]) + float(out["loss"]["question_reconstruction_gt"])) - float(out["bound"])
    assert float(out["objective"]) == pytest.approx(want, rel=1e-5)
    step.settle()
    moved = _moved(before, pg, qr, prior, nmn)
    assert moved[0] and moved[1]                            # the generator and the reconstructor learn
    assert not moved[2] and not prior.training             # the prior is frozen, bit for bit
    assert all(p.grad is None for p in prior.parameters())
    assert moved[3] == train_modules                        # the modules learn when asked to, and only then
    step.close()


def test_evaluate_joint_evidence():
    from probnmn.data.synthetic import synthetic_batch
    from probnmn.evaluators import evaluate_joint_evidence
    from probnmn.trainers.marginal_training import candidate_targets

    dev = torch.device("cuda:0")
    vocab, pg, qr, prior, nmn = _models(dev)
    _, automaton = _constraint(vocab, pg)
    batch = {k: v.to(dev) for k, v in synthetic_batch(vocab, 8, seed=31).items()}
    batches = [{k: v[s] for k, v in batch.items()} for s in (slice(0, 4), slice(4, 8))]
    # metrics on record, the models in different modes
    qr.eval(), prior.eval(), nmn.eval()
    with torch.no_grad():
        qr(batch["program"], batch["question"])
        prior(batch["program"])
        nmn(batch["image"], batch["program"], batch["answer"])
    metrics = lambda: (qr.get_metrics(reset=False), nmn.get_metrics(reset=False), prior._log2_perplexity._count)  # noqa: E731
    metrics()                                        # (as tests/test_importance_bound_gpu.py reads them once before it records them)
    before = metrics()
    pg.train(), prior.train()
    params = _parameters(pg, qr, prior, nmn)

    torch.manual_seed(5)
    one = evaluate_joint_evidence(pg, qr, prior, nmn, batches, num_samples=1, constraint=automaton)
    assert one["questions"] == 8 and one["unsupported"] == 0 and one["bound"].shape == (8,) and one["log_weight"].shape == (8, 1)
    assert torch.equal(one["bound"], one["log_weight"][:, 0])                       # K = 1: the bound is log w
    assert one["log_joint_evidence_bound"] == pytest.approx(float(one["log_weight"].double().mean()), rel=1e-6)
    assert one["effective_sample_size"] == 1.0
    assert one["posterior_answer_accuracy"] == one["proposal_answer_accuracy"]       # one program: its answer either way

    K = 4
    torch.manual_seed(6)
    four = evaluate_joint_evidence(pg, qr, prior, nmn, batches, num_samples=K, constraint=automaton)
    assert four["questions"] == 8 and four["unsupported"] == 0 and four["log_weight"].shape == (8, K)
    assert four["log_answer_given_question"] == pytest.approx(four["log_joint_evidence_bound"] - four["log_evidence_bound"], abs=1e-9)
    assert 1.0 <= four["effective_sample_size"] <= K
    assert pg.training and prior.training and not qr.training and not nmn.training   # the modes are back
    assert metrics() == before                                                        # no metric moved
    assert not any(_moved(params, pg, qr, prior, nmn))

    # the fp64 reference fed the device's own logits: the same draw (the seed), the same passes, in eval() mode
    torch.manual_seed(6)
    for m in (pg, qr, prior, nmn):
        m.eval()
    bound, only_bound, log_weight, scale = [], [], [], []
    right, unsure = {"posterior": 0, "proposal": 0}, {"posterior": 0, "proposal": 0}
    with torch.no_grad():
        for b in batches:
            questions = b["question"].repeat_interleave(K, 0)
            programs = pg(questions, decoding_strategy="constrained_sampling", constraint=automaton)["predictions"]
            targets = candidate_targets(programs, pg)
            terms = (qr.teacher_forced_logits(targets, questions) + (qr._pad_index,),
                     pg.teacher_forced_logits(questions, targets, constraint=automaton) + (pg._pad_index,),
                     prior.teacher_forced_logits(targets) + (prior._pad_index,))
            answered = nmn.hypothesis_answer_logits(b["image"], programs, np.repeat(np.arange(4), K))
            host = [(t[0].cpu().numpy(), t[1].cpu().numpy(), t[2]) for t in terms]
            a_logits, valid = answered["answer_logits"].cpu().numpy(), answered["valid"].cpu().numpy()
            answers = b["answer"].cpu().numpy().astype(np.int64)
            assert (valid == 1).all()                                   # (under the grammar every sample is a program)
            ref = importance_joint_reference(*host, 1.0, K, (a_logits, answers, valid))
            only = importance_joint_reference(*host, 1.0, K, (a_logits, answers, valid), answer_weight=0.0)
            bound.append(ref["bound"]), only_bound.append(only["bound"]), scale.append(ref["scale"])
            log_weight.append(ref["log_weight"].reshape(4, K))
            z = a_logits.astype(np.float64)
            prob = np.exp(z - z.max(1, keepdims=True))
            prob = (prob / prob.sum(1, keepdims=True)).reshape(4, K, -1)
            # The answer of a mixture sum_k w_k p(c | z_k): the shares are within 2 tol_g of the reference's (the header's
            # tolerance) and both sets sum to 1, so sum_k dw_k p_k(c) = sum_k dw_k (p_k(c) - mean_k p_k(c)) moves the mixture
            # by at most 2 tol_g K max_k |p_k(c) - mean_k p_k(c)|; the softmax's own fp32 rounding adds 1e-6.  A question
            # whose two best answers lie closer than twice that (either may move) is UNSURE -- either may be the arg-max
            # -- the others must agree with the reference exactly.
            tol_only = 1e-5 * (1.0 + only["scale"])
            spread = np.abs(prob - prob.mean(1, keepdims=True)).max((1, 2))
            for name, w, bar in (("posterior", only["share"].reshape(4, K), 2 * (2 * tol_only * K * spread + 1e-6)),
                                 ("proposal", np.full((4, K), 1.0 / K), np.full(4, 2e-6))):
                mixture = (w[:, :, None] * prob).sum(1)
                top = np.sort(mixture, axis=1)
                sure = top[:, -1] - top[:, -2] > bar
                right[name] += int(((mixture.argmax(1) == answers) & sure).sum())
                unsure[name] += int((~sure).sum())
    bound, only_bound, log_weight = np.concatenate(bound), np.concatenate(only_bound), np.concatenate(log_weight)
    tol_g = 1e-5 * (1.0 + np.concatenate(scale))
    assert (np.abs(four["bound"].cpu().numpy() - bound) <= tol_g).all()
    assert (np.abs(four["log_weight"].cpu().numpy() - log_weight) <= tol_g[:, None]).all()
    assert abs(four["log_joint_evidence_bound"] - bound.mean()) <= tol_g.max()
    assert abs(four["log_evidence_bound"] - only_bound.mean()) <= tol_g.max()
    print("questions whose mixture's arg-max hangs on rounding: %s of 8" % unsure)
    for name in ("posterior", "proposal"):
        assert right[name] <= round(8 * four[name + "_answer_accuracy"]) <= right[name] + unsure[name], name
