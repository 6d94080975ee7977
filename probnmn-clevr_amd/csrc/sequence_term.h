// One likelihood term of the kernels that score token sequences under teacher-forced logits (hypothesis_posterior.hip,
// importance_bound.hip): the term's arguments, log p of a row's tokens and the row's cross-entropy gradient.  Every rule
// about padding, tokens that are no index (log p = -inf) and logits of -inf is stated here, once; the two kernels report the
// same bits for the same logits and tokens.
// (Internal linkage on purpose: each kernel file gets its own copies, inlined as when they were written in that file.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hypothesis_group.h"

namespace pnmn {
namespace hypothesis {
namespace {

struct Term {  // one likelihood term: teacher-forced logits and the tokens they score
    const float* logits;    // [n_rows][T][V], null: the term is not computed
    const int64_t* tokens;  // row r at tokens + r * stride, T entries
    int64_t stride;
    float* out;             // [n_rows] or null
    float* d;               // gradient mode: [n_rows][T][V] or null (it arrives in out's place)
    float w;
    int T, V, pad;
    bool scored;            // the term enters the score (logits given and w != 0)
};

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
            load_columns<NPER>(block + (size_t)step[u] * V, V, lane, z[u]);
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
                at[u] = lane_held<NPER>(z[u], token);
                se[u] = 0.f;
#pragma unroll
                for (int j = 0; j < NPER; ++j) se[u] += expf(z[u][j] - top[u]);  // (columns beyond V hold -inf: exp gives 0)
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

// Gradient mode: d(-log_evidence[g]) / d logits of row r's term k into k.d, every one of the row's T * V words written.
// `use`: the row is usable and the term enters the score (wave-uniform); share = w_k exp(log_posterior[r]).  A row that is
// not used is one run of zeros and its logits are not read.  Of a used row the scored steps are taken U at a time exactly as
// row_log_likelihood() takes them (the same maximum and the same sum of exponentials, so log softmax is the one the score was
// built from), and each leaves as one coalesced segment per register column; the target's column is found by comparing v.
// A logit of -inf gets exactly 0; the padding steps leave as zeros.
template <int NPER, int U>
__device__ void row_gradient(const Term& k, int r, int lane, bool use, float share) {
    const int T = k.T, V = k.V;
    float* __restrict__ d_row = k.d + (size_t)r * T * V;
    if (!use) {
        for (size_t i = lane; i < (size_t)T * V; i += WAVE) d_row[i] = 0.f;
        return;
    }
    const float* row = k.logits + (size_t)r * T * V;
    const int64_t* tok = k.tokens + (int64_t)r * k.stride;
    for (int t0 = 0; t0 < T; t0 += WAVE) {
        const bool inside = t0 + lane < T;
        int mine = -1;  // (as in row_log_likelihood)
        if (inside) {
            const int64_t t = tok[t0 + lane];
            mine = t == (int64_t)k.pad ? -1 : (t < 0 || t >= (int64_t)V) ? -2 : (int)t;
        }
        // (a usable row has no token that is no index; rows that malformed bounds let two groups share may: such a step is
        // written as zeros, and its token is never an index)
        uint64_t steps = __ballot(mine >= 0);
        uint64_t zeros = __ballot(inside && mine < 0);
        float* __restrict__ d_block = d_row + (size_t)t0 * V;
        while (zeros) {
            const int s = __ffsll((unsigned long long)zeros) - 1;
            zeros &= zeros - 1;
#pragma unroll
            for (int j = 0; j < NPER; ++j) {
                const int c = lane + WAVE * j;
                if (c < V) d_block[(size_t)s * V + c] = 0.f;
            }
        }
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
            float top[U], se[U];
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
                se[u] = 0.f;
#pragma unroll
                for (int j = 0; j < NPER; ++j) se[u] += expf(z[u][j] - top[u]);
            }
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1)
#pragma unroll
                for (int u = 0; u < U; ++u) se[u] += __shfl_xor(se[u], d, WAVE);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (step[u] < 0) continue;
                const int token = __builtin_amdgcn_readlane(mine, step[u]);
                const float log_z = logf(se[u]);
                float* __restrict__ d_step = d_block + (size_t)step[u] * V;
#pragma unroll
                for (int j = 0; j < NPER; ++j) {
                    const int c = lane + WAVE * j;
                    if (c < V) {
                        float g = 0.f;
                        if (z[u][j] > -INFINITY) {  // (a logit of -inf: probability 0, gradient 0)
                            const float prob = expf((z[u][j] - top[u]) - log_z);  // (<= 1: both terms are <= 0)
                            g = share * (prob - (c == token ? 1.f : 0.f));
                        }
                        d_step[c] = g;
                    }
                }
            }
        }
    }
}

}  // namespace
}  // namespace hypothesis
}  // namespace pnmn
