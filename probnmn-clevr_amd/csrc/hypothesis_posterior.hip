// The posterior over a question's program hypotheses under the generative model, for gfx950:
//     p(z_r | x) ~ p(x | z_r)^w_x  p(z_r)^w_z  q(z_r | x)^w_q      over the rows r of the question's group
// from the teacher-forced logits of the reconstructor (x) and of the prior (z), the tokens they score and the generator's
// log-weight of every row: per row log p(x | z_r) and log p(z_r), per group the normalised log-posterior, the log-evidence
// and the MAP row.
//
// Not in the reference: it scores sampled programs with the three models in TRAINING only (probnmn/modules/elbo.py:130-161,
// through per-token mean losses) and answers from one sampled program (scripts/inference.py:76-91).
// include/probnmn_hip.h states the contract; tests/helpers/hypothesis_posterior_reference.py is the same in fp64 numpy.
//
//   workgroup   512 threads = eight wavefronts, one GROUP (one question's hypotheses) per workgroup; no LDS, no atomics, no
//               wait on another workgroup, every loop bounded by the clamped group bounds
//   rows        wave w takes the group's rows w, w + 8, ...: a row's two likelihood terms and its score come from exactly
//               one wave in a fixed order, so which wave took it cannot change the bits.  (The work is latency: a row is a
//               chain of dependent wave reductions.  Measured at 256 groups x 8 rows with the CLEVR shapes: four waves and one
//               step at a time 115 us, four steps at a time 64 us, eight waves and eight steps 38 us.)
//   lanes       run over the vocabulary (hypothesis_group.h: the column layout, the group bounds, the wave reductions), so
//               a step's logits are one coalesced segment
//   steps       a row's tokens are read 64 at a time, one per lane; the scored ones form a wave-uniform bit set, so padding
//               costs nothing, and the rest is taken U at a time (8 for V <= 128, 4 / 2 / 1 up to 256 / 512 / 1024): their butterflies
//               overlap, and the next U steps' logits are loaded before these are reduced
//   score       the wave's lane 0 writes score[r] into log_posterior[r]; ONE __syncthreads(); wave 0 then sweeps the group's
//               scores (64 at a time): the usable rows, the largest score and its first row; then score_normaliser()
//
// GRADIENT MODE (pnmn_hypothesis_posterior without best_row and with a log_px / log_pz pointer, which is then d_x_logits
// [n_rows][Tx][Vx] / d_z_logits [n_rows][Tz][Vz]): the same kernel body with GRAD set -- so the outputs the two modes share
// are the same bits -- and one more sweep.  The loss of a group is -log_evidence[g]; its gradient with respect to a row's
// logits of term k is the row's per-step cross-entropy gradient scaled by the row's posterior share:
//   barriers    NO wave returns before the second __syncthreads(): waves 1..7 skip wave 0's epilogue and wait at it, so the
//               posteriors wave 0 stored (a lane per row) are visible to every wave
//   sweep       every wave takes ITS OWN rows again (w, w + 8, ...; the logits are in L2): share_k = w_k exp(log_posterior[r]);
//               a row that is not usable, and every row of a term that does not enter the score, is one run of zeros; of a
//               usable row the scored steps go U at a time as in row_log_likelihood() -- the same maximum and sum, the next
//               U steps' logits loaded before these are reduced -- and d[t][v] = share_k (softmax_v - [v == token]) leaves as
//               one coalesced segment per register column, the target's column found by comparing v, never by indexing;
//               the padding steps leave as zeros the same way.  No word outside the group's clamped rows is touched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/probnmn_hip.h"
#include "hypothesis_group.h"
#include "sequence_term.h"  // Term, row_log_likelihood(), row_gradient(): shared with importance_bound.hip

namespace {

using namespace pnmn::hypothesis;

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / WAVE;

struct PosteriorArgs {
    Term x, z;
    const float* log_q;
    float w_q;  // (0 when log_q is null or the coefficient is 0: the term is left out)
    const int32_t* group_start;
    float* log_posterior;
    float* log_evidence;
    int32_t* best_row;
    int32_t* support;
    int n_groups, n_rows;
};

template <int NPER, bool GRAD>
__global__ __launch_bounds__(THREADS) void hypothesis_posterior_kernel(const PosteriorArgs p) {
    constexpr int U = NPER <= 2 ? 8 : 16 / NPER;  // steps in flight per wave: at most 16 registers of logits, twice
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const int g = blockIdx.x;
    const Rows rows = group_rows(p.group_start, g, p.n_rows);
    const int start = rows.start, end = rows.end;

    // ---- every wave: the likelihood terms and the score of its rows ----
    for (int r = start + wave; r < end; r += WAVES) {
        float score = 0.f;
        if (p.x.logits) {
            const float lp = row_log_likelihood<NPER, U>(p.x, r, lane);
            if (lane == 0 && p.x.out) p.x.out[r] = lp;
            if (p.x.scored) score += p.x.w * lp;
        }
        if (p.z.logits) {
            const float lp = row_log_likelihood<NPER, U>(p.z, r, lane);
            if (lane == 0 && p.z.out) p.z.out[r] = lp;
            if (p.z.scored) score += p.z.w * lp;
        }
        if (p.w_q != 0.f) score += p.w_q * p.log_q[r];
        if (lane == 0) p.log_posterior[r] = score;
    }
    __syncthreads();  // (workgroup scope: the scores the other waves stored are visible to wave 0)
    if constexpr (!GRAD) {
        if (wave != 0) return;
    }

    // ---- wave 0: the group's usable rows, the largest score and its first row ----
    if (!GRAD || wave == 0) {  // (gradient mode: the other waves go on to the second barrier, none returns before it)
        int count = 0, at = 0x7fffffff;
        float top = -INFINITY;
        for (int r = start + lane; r < end; r += WAVE) {
            const float s = p.log_posterior[r];
            if (finite(s)) {
                ++count;
                if (s > top || at == 0x7fffffff) top = s, at = r;  // (rows grow: the lane's first maximum)
            }
        }
        count = wave_sum(count);
        wave_argmax(top, at);  // (a lane without a usable row holds (-inf, int max) and never wins a tie)
        const float log_norm = score_normaliser(p.log_posterior, rows, lane, count, top);
        if (lane == 0) {
            p.log_evidence[g] = count > 0 ? top + log_norm : -INFINITY;
            if constexpr (!GRAD) p.best_row[g] = count > 0 ? at : -1;
            if (p.support) p.support[g] = count;
        }
    }

    // ---- gradient mode, every wave: d(-log_evidence[g]) / d logits of its rows ----
    if constexpr (GRAD) {
        __syncthreads();  // (the posteriors wave 0 stored, a lane per row, are visible to every wave; all 512 threads arrive)
        for (int r = start + wave; r < end; r += WAVES) {
            const float lp = p.log_posterior[r];
            const bool use = finite(lp);  // (wave-uniform; -inf for a row that is not usable, so for a group without support)
            const float weight = use ? expf(lp) : 0.f;
            if (p.x.d) row_gradient<NPER, U>(p.x, r, lane, use && p.x.scored, p.x.w * weight);
            if (p.z.d) row_gradient<NPER, U>(p.z, r, lane, use && p.z.scored, p.z.w * weight);
        }
    }
}

}  // namespace

extern "C" int pnmn_hypothesis_posterior(const float* x_logits, const int64_t* x_tokens, int64_t x_token_stride,
                                         const float* z_logits, const int64_t* z_tokens, int64_t z_token_stride,
                                         const float* log_q, const int32_t* group_start, float w_x, float w_z, float w_q,
                                         int pad_x, int pad_z, float* log_px, float* log_pz, float* log_posterior,
                                         float* log_evidence, int32_t* best_row, int32_t* support, int n_groups, int n_rows,
                                         int Tx, int Vx, int Tz, int Vz, void* stream) {
    if (n_groups < 0 || n_rows < 0) return PNMN_EINVAL;
    if (n_groups == 0) return 0;  // (nothing to read or to write)
    // gradient mode: no best_row, and log_px's / log_pz's place holds d_x_logits / d_z_logits (refused until this mode
    // existed: best_row was null)
    const bool grad = !best_row && (log_px || log_pz);
    if (!group_start || !log_posterior || !log_evidence || (!best_row && !grad)) return PNMN_EINVAL;
    if (grad && ((log_px && !x_logits) || (log_pz && !z_logits))) return PNMN_EINVAL;
    if ((x_logits && !x_tokens) || (z_logits && !z_tokens) || (!x_logits && !z_logits && !log_q)) return PNMN_EINVAL;
    if ((x_logits && (Tx < 1 || Vx < 1)) || (z_logits && (Tz < 1 || Vz < 1))) return PNMN_EINVAL;
    if (!(fabsf(w_x) < INFINITY) || !(fabsf(w_z) < INFINITY) || !(fabsf(w_q) < INFINITY)) return PNMN_EINVAL;
    if ((x_logits && Vx > MAX_COLUMNS) || (z_logits && Vz > MAX_COLUMNS)) return PNMN_ESHAPE;
    PosteriorArgs a;
    // (a term that neither enters the score nor is asked for is not computed)
    const bool score_x = x_logits && w_x != 0.f, score_z = z_logits && w_z != 0.f;
    if (grad) {  // (lp_x and lp_z are not reported; a term that does not enter the score is not read, its gradient is zeros)
        a.x = Term{score_x ? x_logits : nullptr, x_tokens, x_token_stride, nullptr, log_px, w_x, Tx, Vx, pad_x, score_x};
        a.z = Term{score_z ? z_logits : nullptr, z_tokens, z_token_stride, nullptr, log_pz, w_z, Tz, Vz, pad_z, score_z};
    } else {
        a.x = Term{score_x || log_px ? x_logits : nullptr, x_tokens, x_token_stride, log_px, nullptr, w_x, Tx, Vx, pad_x, score_x};
        a.z = Term{score_z || log_pz ? z_logits : nullptr, z_tokens, z_token_stride, log_pz, nullptr, w_z, Tz, Vz, pad_z, score_z};
    }
    a.log_q = log_q;
    a.w_q = log_q ? w_q : 0.f;
    a.group_start = group_start;
    a.log_posterior = log_posterior;
    a.log_evidence = log_evidence;
    a.best_row = best_row;
    a.support = support;
    a.n_groups = n_groups;
    a.n_rows = n_rows;
    return with_nper(std::max(a.x.logits ? Vx : 1, a.z.logits ? Vz : 1), [&](auto nper) {
        constexpr int NPER = decltype(nper)::value;
        const auto kernel = grad ? hypothesis_posterior_kernel<NPER, true> : hypothesis_posterior_kernel<NPER, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_groups), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
        return (int)hipGetLastError();
    });
}
