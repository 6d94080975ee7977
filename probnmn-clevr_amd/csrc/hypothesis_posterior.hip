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
//   lanes       run over the vocabulary: lane l holds columns l, l + 64, ... (NPER = ceil(V / 64) registers per step), so a
//               step's logits are one coalesced segment
//   steps       a row's tokens are read 64 at a time, one per lane; the scored ones form a wave-uniform bit set, so padding
//               costs nothing, and the rest is taken U at a time (8 for V <= 128, 4 / 2 / 1 up to 256 / 512 / 1024): their butterflies
//               overlap, and the next U steps' logits are loaded before these are reduced
//   score       the wave's lane 0 writes score[r] into log_posterior[r]; ONE __syncthreads(); wave 0 then sweeps the group's
//               scores (64 at a time): the usable rows, the largest score and its first row; the sum of exp(score - largest);
//               log_posterior[r] = (score[r] - largest) - log(sum) over the slots the scores were in
// Wave reductions are xor butterflies: every lane ends with the same bits, in an order that depends on nothing but the lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/probnmn_hip.h"

namespace {

constexpr int THREADS = 512;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int MAX_VOCAB = 1024;  // NPER <= 16 registers per step and lane

struct Term {  // one likelihood term: teacher-forced logits and the tokens they score
    const float* logits;    // [n_rows][T][V], null: the term is not computed
    const int64_t* tokens;  // row r at tokens + r * stride, T entries
    int64_t stride;
    float* out;             // [n_rows] or null
    float w;
    int T, V, pad;
    bool scored;            // the term enters the score (logits given and w != 0)
};

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

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// the largest value and the lowest index that holds it (the first maximum), in every lane
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const float ov = __shfl_xor(v, d, WAVE);
        const int oi = __shfl_xor(i, d, WAVE);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ bool finite(float x) { return fabsf(x) < INFINITY; }  // (false for a NaN)

template <int NPER>
__device__ __forceinline__ void load_step(const float* __restrict__ step, int V, int lane, float (&z)[NPER]) {
#pragma unroll
    for (int k = 0; k < NPER; ++k) {
        const int v = lane + WAVE * k;
        z[k] = v < V ? step[v] : -INFINITY;
    }
}

// Up to U scored steps taken off the (wave-uniform) set `steps` in ascending order, their logits requested: step[u] = the
// step's index within its block of 64 (-1: none), z[u] = its logits.
template <int NPER, int U>
__device__ __forceinline__ void take_steps(uint64_t& steps, const float* __restrict__ block, int V, int lane, int (&step)[U],
                                           float (&z)[U][NPER]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (steps) {
            step[u] = __ffsll((unsigned long long)steps) - 1;
            steps &= steps - 1;
            load_step<NPER>(block + (size_t)step[u] * V, V, lane, z[u]);
        } else {
            step[u] = -1;
#pragma unroll
            for (int j = 0; j < NPER; ++j) z[u][j] = -INFINITY;
        }
    }
}

// log p of row r's tokens under its teacher-forced logits: the sum over the steps whose token is not padding of
// (z[token] - max) - log sum exp(z - max), in ascending step order; -inf when a scored token is no index into the vocabulary
// (such a token is never used as one).  Every lane returns the same bits.
// The row's tokens are read 64 at a time, one per lane, and classified: the scored steps of a block are a wave-uniform bit
// set, so padding steps cost nothing and the rest is taken U at a time -- their 2 U butterflies are independent and
// overlap, and the next U steps' logits are on their way meanwhile.  A step's bits do not depend on U or on its neighbours.
template <int NPER, int U>
__device__ float row_log_likelihood(const Term& k, int r, int lane) {
    const int T = k.T, V = k.V;
    const float* row = k.logits + (size_t)r * T * V;
    const int64_t* tok = k.tokens + (int64_t)r * k.stride;
    float lp = 0.f;
    for (int t0 = 0; t0 < T; t0 += WAVE) {
        // this lane's step: its token (>= 0), -1 for padding or beyond T, -2 for a token that is no index
        int mine = -1;
        if (t0 + lane < T) {
            const int64_t t = tok[t0 + lane];
            mine = t == (int64_t)k.pad ? -1 : (t < 0 || t >= (int64_t)V) ? -2 : (int)t;
        }
        if (__ballot(mine == -2)) return -INFINITY;
        uint64_t steps = __ballot(mine >= 0);
        const float* block = row + (size_t)t0 * V;
        int step[U], ahead[U];
        float z[U][NPER], nxt[U][NPER];
        take_steps<NPER, U>(steps, block, V, lane, ahead, nxt);
        while (ahead[0] >= 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                step[u] = ahead[u];
#pragma unroll
                for (int j = 0; j < NPER; ++j) z[u][j] = nxt[u][j];
            }
            take_steps<NPER, U>(steps, block, V, lane, ahead, nxt);
            float top[U], se[U], at[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                top[u] = z[u][0];
#pragma unroll
                for (int j = 1; j < NPER; ++j) top[u] = fmaxf(top[u], z[u][j]);
            }
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1)
#pragma unroll
                for (int u = 0; u < U; ++u) top[u] = fmaxf(top[u], __shfl_xor(top[u], d, WAVE));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // (an empty slot: step 0's token stands in, its result is not used)
                const int token = __builtin_amdgcn_readlane(mine, step[u] >= 0 ? step[u] : 0);
                const int reg = token >> 6;
                float held = 0.f;
                se[u] = 0.f;
#pragma unroll
                for (int j = 0; j < NPER; ++j) {
                    se[u] += expf(z[u][j] - top[u]);  // (columns beyond V hold -inf: exp gives 0)
                    if (j == reg) held = z[u][j];
                }
                at[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(held), token & (WAVE - 1)));
            }
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1)
#pragma unroll
                for (int u = 0; u < U; ++u) se[u] += __shfl_xor(se[u], d, WAVE);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (step[u] >= 0) lp += (at[u] - top[u]) - logf(se[u]);
        }
    }
    return lp;
}

template <int NPER>
__global__ __launch_bounds__(THREADS) void hypothesis_posterior_kernel(const PosteriorArgs p) {
    constexpr int U = NPER <= 2 ? 8 : 16 / NPER;  // steps in flight per wave: at most 16 registers of logits, twice
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const int g = blockIdx.x;
    // the group's rows, clamped into the arrays whatever group_start says
    const int start = min(max(p.group_start[g], 0), p.n_rows);
    const int end = max(min(max(p.group_start[g + 1], 0), p.n_rows), start);

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
    if (wave != 0) return;

    // ---- wave 0: the group's usable rows, the largest score and its first row ----
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
    float log_norm = 0.f;
    if (count > 0) {
        float se = 0.f;
        for (int r = start + lane; r < end; r += WAVE) {
            const float s = p.log_posterior[r];
            if (finite(s)) se += expf(s - top);
        }
        log_norm = logf(wave_sum(se));
    }
    for (int r = start + lane; r < end; r += WAVE) {
        const float s = p.log_posterior[r];
        p.log_posterior[r] = finite(s) ? (s - top) - log_norm : -INFINITY;
    }
    if (lane == 0) {
        p.log_evidence[g] = count > 0 ? top + log_norm : -INFINITY;
        p.best_row[g] = count > 0 ? at : -1;
        if (p.support) p.support[g] = count;
    }
}

template <int NPER>
int launch(const PosteriorArgs& a, void* stream) {
    hipLaunchKernelGGL(hypothesis_posterior_kernel<NPER>, dim3((unsigned)a.n_groups), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
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
    if (!group_start || !log_posterior || !log_evidence || !best_row) return PNMN_EINVAL;
    if ((x_logits && !x_tokens) || (z_logits && !z_tokens) || (!x_logits && !z_logits && !log_q)) return PNMN_EINVAL;
    if ((x_logits && (Tx < 1 || Vx < 1)) || (z_logits && (Tz < 1 || Vz < 1))) return PNMN_EINVAL;
    if (!(fabsf(w_x) < INFINITY) || !(fabsf(w_z) < INFINITY) || !(fabsf(w_q) < INFINITY)) return PNMN_EINVAL;
    if ((x_logits && Vx > MAX_VOCAB) || (z_logits && Vz > MAX_VOCAB)) return PNMN_ESHAPE;
    PosteriorArgs a;
    // (a term that neither enters the score nor is asked for is not computed)
    const bool score_x = x_logits && w_x != 0.f, score_z = z_logits && w_z != 0.f;
    a.x = Term{score_x || log_px ? x_logits : nullptr, x_tokens, x_token_stride, log_px, w_x, Tx, Vx, pad_x, score_x};
    a.z = Term{score_z || log_pz ? z_logits : nullptr, z_tokens, z_token_stride, log_pz, w_z, Tz, Vz, pad_z, score_z};
    a.log_q = log_q;
    a.w_q = log_q ? w_q : 0.f;
    a.group_start = group_start;
    a.log_posterior = log_posterior;
    a.log_evidence = log_evidence;
    a.best_row = best_row;
    a.support = support;
    a.n_groups = n_groups;
    a.n_rows = n_rows;
    const int nper = (std::max(a.x.logits ? Vx : 1, a.z.logits ? Vz : 1) + WAVE - 1) / WAVE;
    if (nper <= 1) return launch<1>(a, stream);
    if (nper <= 2) return launch<2>(a, stream);
    if (nper <= 4) return launch<4>(a, stream);
    if (nper <= 8) return launch<8>(a, stream);
    return launch<16>(a, stream);
}
