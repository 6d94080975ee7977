"""The ragged inputs the ``pnmn_answer_posterior`` tests share (the reference test asserts on the CPU what the device test
relies on), and the seeds at which they hold."""
import numpy as np

FIXED_SIZES = [0, 1, 2, 3, 16, 17, 64, 65, 5, 1, 0, 7]
DEAD_GROUP = 5           # (the 17 rows: every weight is -inf)
BEYOND_GROUP = 8         # (the 5 rows: the given answer is A + 3)
NEGATIVE_GROUP = 11      # (the 7 rows: the given answer is -2)
# NPER 1, 2 and 4 and both sides of a lane boundary; 257 and 513, the first widths of the NPER 8 and 16 kernels (one live
# column in their register 4 and 8); 1024, the full width
ANSWERS = (1, 2, 28, 64, 65, 130, 257, 513, 1024)
# one seed per number of answers at which, on the reference alone, the two best scores of every supported group differ by
# 100 x the group's tolerance in every variant ``variants`` lists, and at least 28 groups are supported (searched on the CPU
# with ``ragged_inputs`` and the reference, seeds 0 .. 39: 38 and 32 of them do at A = 1 and 2, 13 to 23 from A = 28 to 130,
# 9, 13 and 18 at A = 257, 513 and 1024, where the first that does is taken)
SEEDS = {1: 0, 2: 0, 28: 0, 64: 0, 65: 2, 130: 0, 257: 4, 513: 0, 1024: 5}


def variants(A, log_weight):
    """(w_a, log_weight) pairs an A runs with: the weights given with w_a = 1 and 0.5, and -- from 28 answers on -- uniform
    weights.  With two answers the top scores of a 64-row uniform group cluster at log 1 within the margin; with one answer
    every uniform score ties exactly, which the tie test covers."""
    return [(1.0, log_weight), (0.5, log_weight)] + ([(1.0, None)] if A >= 28 else [])


def ragged_inputs(A: int, seed: int):
    """37 groups: FIXED_SIZES and 25 groups of 1 .. 8 rows.  Returns logits fp32 [R, A], valid int32 [R] (about one row in ten
    invalid), log_weight fp32 [R] (some -inf, all of DEAD_GROUP's), answers int64 [37] (one beyond the answers, one
    negative) and group_start int32 [38]; some rows hold -inf at their question's answer (A > 1), some are scaled by 8."""
    rng = np.random.default_rng(1000 * A + seed)
    sizes = np.array(FIXED_SIZES + rng.integers(1, 9, 25).tolist())
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    R = int(start[-1])
    logits = (rng.standard_normal((R, A)) * 3).astype(np.float32)
    logits[rng.random(R) < 0.1] *= 8                           # rows far out in the exponent range
    valid = (rng.random(R) >= 0.1).astype(np.int32)
    log_weight = (rng.standard_normal(R) * 4 - 20).astype(np.float32)
    log_weight[rng.random(R) < 0.08] = -np.inf
    log_weight[start[DEAD_GROUP]:start[DEAD_GROUP + 1]] = -np.inf
    answers = rng.integers(0, A, len(sizes)).astype(np.int64)
    answers[BEYOND_GROUP], answers[NEGATIVE_GROUP] = A + 3, -2
    if A > 1:
        group_of = np.repeat(np.arange(len(sizes)), sizes)
        for r in np.nonzero(rng.random(R) < 0.05)[0]:          # -inf at the target
            if 0 <= answers[group_of[r]] < A:
                logits[r, answers[group_of[r]]] = -np.inf
    return logits, valid, log_weight, answers, start
