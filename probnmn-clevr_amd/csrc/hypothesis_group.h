// Building blocks of the kernels that reduce over one question's program hypotheses (answer_marginal.hip,
// hypothesis_posterior.hip, answer_posterior.hip): each rule exists once, here.  A GROUP is the rows
// group_start[g] .. group_start[g + 1] of one question; one wavefront works on it with its lanes over the columns (answers
// or vocabulary) of a row: lane l holds columns l, l + 64, ... in NPER = ceil(columns / 64) registers.
// Wave reductions are xor butterflies: every lane ends with the same bits, in an order that depends on nothing but the lane.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

namespace pnmn {
namespace hypothesis {

constexpr int WAVE = 64;
constexpr int MAX_COLUMNS = 1024;  // NPER <= 16 registers per row and lane

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v = fmaxf(v, __shfl_xor(v, d, WAVE));
    return v;
}

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

// One row of n columns: lane l gets columns l, l + 64, ...; a register beyond n holds -inf (exp gives 0, it wins no maximum).
template <int NPER>
__device__ __forceinline__ void load_columns(const float* __restrict__ row, int n, int lane, float (&z)[NPER]) {
#pragma unroll
    for (int k = 0; k < NPER; ++k) {
        const int c = lane + WAVE * k;
        z[k] = c < n ? row[c] : -INFINITY;
    }
}

// Column i of a row held as load_columns() left it (register i >> 6 of lane i & 63), in every lane; i is wave-uniform.
template <int NPER>
__device__ __forceinline__ float lane_held(const float (&z)[NPER], int i) {
    float held = 0.f;
#pragma unroll
    for (int k = 0; k < NPER; ++k)
        if (k == (i >> 6)) held = z[k];
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(held), i & (WAVE - 1)));
}

// the group's rows, clamped into the arrays whatever group_start says
struct Rows {
    int start, end;
};
__device__ __forceinline__ Rows group_rows(const int32_t* __restrict__ group_start, int g, int n_rows) {
    const int start = min(max(group_start[g], 0), n_rows);
    const int end = max(min(max(group_start[g + 1], 0), n_rows), start);
    return {start, end};
}

// Sweep 1 of the answer kernels, over the group's rows 64 at a time: a row is USABLE when it is valid (null: every row is)
// and its log-weight is finite (null: every row weighs the same).  count = the usable rows, lw_max = their largest
// log-weight, log_norm = log(sum exp(log-weight - largest)) -- so that log w_r = (lw_r - lw_max) - log_norm, every term
// rounded at its own size; log(count) for uniform weights, 0 for a group without a usable row.  The same in every lane.
struct WeightNorm {
    int count;
    float lw_max, log_norm;
};
__device__ __forceinline__ WeightNorm weight_normaliser(const int32_t* __restrict__ valid, const float* __restrict__ log_weight,
                                                        Rows rows, int lane) {
    auto usable = [&](int r) { return (valid == nullptr || valid[r] != 0) && (log_weight == nullptr || finite(log_weight[r])); };
    int count = 0;
    float lw_max = -INFINITY;
    for (int r = rows.start + lane; r < rows.end; r += WAVE)
        if (usable(r)) {
            ++count;
            lw_max = fmaxf(lw_max, log_weight ? log_weight[r] : 0.f);
        }
    count = wave_sum(count);
    lw_max = wave_max(lw_max);
    float log_norm = 0.f;
    if (count > 0) {
        if (log_weight) {
            float se = 0.f;
            for (int r = rows.start + lane; r < rows.end; r += WAVE)
                if (usable(r)) se += expf(log_weight[r] - lw_max);
            log_norm = logf(wave_sum(se));
        } else {
            log_norm = logf((float)count);
        }
    }
    return {count, lw_max, log_norm};
}

// The softmax statistics of one row held as load_columns() left it: its maximum, the first column that holds it, and the
// returned log(sum exp(z - maximum)); log softmax of column c is then (z_c - best) - log_z.  The same in every lane.
template <int NPER>
__device__ __forceinline__ float row_softmax_stats(const float (&z)[NPER], int lane, float& best, int& at) {
    best = z[0];
    at = lane;
#pragma unroll
    for (int k = 1; k < NPER; ++k)
        if (z[k] > best) best = z[k], at = lane + WAVE * k;  // (columns grow with k: the lane's first maximum)
    wave_argmax(best, at);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < NPER; ++k) se += expf(z[k] - best);  // (columns beyond n hold -inf: exp gives 0)
    return logf(wave_sum(se));
}

// Sweep 3 of the posterior kernels, by ONE wave, after the barrier that makes the scores visible to it: the group's scores
// are parked in log_posterior (a row that does not count holds a value that is not finite), `count` of them count and
// `top` is the largest.  Over those slots, 64 at a time: the returned log_norm = log(sum exp(score - top)) (0 for count
// == 0), and log_posterior[r] = (score[r] - top) - log_norm, -inf for a row that does not count.
__device__ __forceinline__ float score_normaliser(float* __restrict__ log_posterior, Rows rows, int lane, int count, float top) {
    float log_norm = 0.f;
    if (count > 0) {
        float se = 0.f;
        for (int r = rows.start + lane; r < rows.end; r += WAVE) {
            const float s = log_posterior[r];
            if (finite(s)) se += expf(s - top);
        }
        log_norm = logf(wave_sum(se));
    }
    for (int r = rows.start + lane; r < rows.end; r += WAVE) {
        const float s = log_posterior[r];
        log_posterior[r] = finite(s) ? (s - top) - log_norm : -INFINITY;
    }
    return log_norm;
}

// Host side: the kernel variant for `columns` (1 .. MAX_COLUMNS) columns -- f(std::integral_constant<int, NPER>) with the
// smallest NPER of 1, 2, 4, 8, 16 that holds them.
template <class F>
int with_nper(int columns, F&& f) {
    const int nper = (columns + WAVE - 1) / WAVE;
    if (nper <= 1) return f(std::integral_constant<int, 1>{});
    if (nper <= 2) return f(std::integral_constant<int, 2>{});
    if (nper <= 4) return f(std::integral_constant<int, 4>{});
    if (nper <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

}  // namespace hypothesis
}  // namespace pnmn
