// Grammar-masked logits for gfx950 (include/probnmn_grammar.h): every step's logits restricted to the allowed set of the
// token automaton the constrained decoders sample under, so that log_softmax of the result is log q_c -- the distribution
// those samples come from -- and the sequence losses can train the generator on them.  The sets are the decoders' own
// (pnmn::allowed_lanes / advance_row_state, sampling.h), rebuilt from each row's tokens.
//
// One wave per row walks the row's steps with the automaton state in a scalar register; lanes answer for columns lane and
// lane + 64 (V <= 128).  About 2 B T V 4 bytes move (10 MB at 1024 x 27 x 44): the launch and a row's chain of steps are
// what it costs, not the bytes (DESIGN 5 "Training under the grammar").
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_grammar.h"
#include "sampling.h"

namespace {

using pnmn::AutomatonLds;
using pnmn::LaneSet;
using pnmn::TokenAutomaton;
using pnmn::wmax;
using pnmn::wsum;

constexpr int ROWS_PER_GROUP = 8;  // 512 threads: what stage_automaton is written for

struct Specials {
    int pad, unk, start;
};

// S_t of one row at step t and the row's state behind the step's token (the rule: probnmn_grammar.h).  Wave-uniform in
// `state` and `tok` (-1: outside [0, V)); `unmasked` = the set ran empty and stands for all of [0, V); `out` = the step
// counts for `outside`.
__device__ __forceinline__ LaneSet step_set(const AutomatonLds& au, int& state, int tok, bool is_pad, int left, int V,
                                            const Specials& sp, bool& unmasked, bool& out) {
    const int lane = threadIdx.x & 63;
    LaneSet set = pnmn::allowed_lanes(au, state, left, V, sp.pad, sp.unk, sp.start);
    const bool mine_lo = tok == lane, mine_hi = tok == lane + 64;
    const bool inside = __ballot((mine_lo && set.lo) || (mine_hi && set.hi)) != 0;
    out = !(state & pnmn::ROW_FINISHED) && !is_pad && !inside;
    set.lo |= mine_lo;  // (tok < V, or -1: no lane's)
    set.hi |= mine_hi;
    unmasked = __ballot(set.lo || set.hi) == 0;
    if (unmasked) set = LaneSet{lane < V, lane + 64 < V};
    if (tok >= 0) state = pnmn::advance_row_state(au, state, tok);
    return set;
}

// BWD = false: x = logits, y = masked, log_mass and outside as given.  BWD = true: x = d_masked, y = d_logits.
template <bool BWD>
__global__ __launch_bounds__(64 * ROWS_PER_GROUP) void grammar_logits_kernel(
    const float* __restrict__ x, int64_t x_bstride, const int64_t* __restrict__ tokens, int64_t tok_bstride,
    float* __restrict__ y, int64_t y_bstride, float* __restrict__ log_mass, int32_t* __restrict__ outside, int B, int T, int V,
    int horizon, Specials sp, const TokenAutomaton automaton) {
    __shared__ unsigned char tables[pnmn::AUTOMATON_LDS_BYTES];
    const AutomatonLds au = pnmn::stage_automaton(tables, automaton);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * ROWS_PER_GROUP + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* xr = x + (size_t)b * x_bstride;
    float* yr = y + (size_t)b * y_bstride;
    const int64_t* tr = tokens + (size_t)b * tok_bstride;
    const float fill = BWD ? 0.f : -INFINITY;
    int state = 0, n_out = 0;
    // the steps are a serial chain through the state, but what they read is not: step t + 1's token and columns are
    // requested before step t is worked on, so their latency hides behind it
    int64_t next_tok = tr[0];
    float next_v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) next_v[k] = lane + 64 * k < V ? xr[lane + 64 * k] : fill;
    for (int t = 0; t < T; ++t) {
        const int64_t tok64 = next_tok;
        const float v[2] = {next_v[0], next_v[1]};
        if (t + 1 < T) {
            next_tok = tr[t + 1];
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (lane + 64 * k < V) next_v[k] = xr[(size_t)(t + 1) * V + lane + 64 * k];
        }
        const int tok = __builtin_amdgcn_readfirstlane((tok64 >= 0 && tok64 < V) ? (int)tok64 : -1);
        const bool is_pad = __builtin_amdgcn_readfirstlane((int)(tok64 == (int64_t)sp.pad)) != 0;
        bool unmasked, out;
        const LaneSet set = step_set(au, state, tok, is_pad, horizon - 1 - t, V, sp, unmasked, out);
        n_out += out ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = lane + 64 * k;
            if (j < V) yr[(size_t)t * V + j] = set.has(j) ? v[k] : fill;
        }
        if constexpr (!BWD) {
            if (log_mass != nullptr) {
                float mass = 0.f;
                if (!unmasked) {  // (wave-uniform)
                    float m_all = -INFINITY, m_set = -INFINITY;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        m_all = fmaxf(m_all, v[k]);  // (columns j >= V hold -inf)
                        if (set.has(lane + 64 * k)) m_set = fmaxf(m_set, v[k]);
                    }
                    m_all = wmax(m_all);
                    m_set = wmax(m_set);
                    float s_all = 0.f, s_set = 0.f;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int j = lane + 64 * k;
                        if (j < V) s_all += expf(v[k] - m_all);
                        if (set.has(j)) s_set += expf(v[k] - m_set);
                    }
                    // each lse relative to its own largest entry: a set far below the row's maximum keeps its digits
                    mass = fminf((m_set + logf(wsum(s_set))) - (m_all + logf(wsum(s_all))), 0.f);
                }
                if (lane == 0) log_mass[(size_t)b * T + t] = mass;
            }
        }
    }
    if constexpr (!BWD) {
        if (outside != nullptr && lane == 0) outside[b] = n_out;
    }
}

// what both entry points check before they launch: 0 and `au` filled, 1 = nothing to do, or a negative PNMN_E*
int check_arguments(TokenAutomaton& au, const void* x, const void* tokens, const void* y, int B, int T, int V, int horizon,
                    int end_index, const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left, int n_states,
                    int n_classes) {
    if (B < 0 || T < 0 || V < 0) return PNMN_EINVAL;
    if (B == 0 || T == 0) return 1;  // (an empty batch has no buffers to name)
    if (!x || !tokens || !y || horizon < 1 || V < 1) return PNMN_EINVAL;
    if (V > pnmn::AUTOMATON_TOKENS) return PNMN_ESHAPE;
    return pnmn::fill_automaton(au, token_class, next_state, min_left, n_states, n_classes, V, horizon, end_index);
}

}  // namespace

extern "C" {

int pnmn_grammar_logits(const float* logits, int64_t logits_bstride, const int64_t* tokens, int64_t tok_bstride, float* masked,
                        int64_t masked_bstride, float* log_mass, int32_t* outside, int B, int T, int V, int horizon,
                        int pad_index, int unk_index, int start_index, int end_index, const uint8_t* token_class,
                        const uint8_t* next_state, const uint8_t* min_left, int n_states, int n_classes, void* stream) {
    TokenAutomaton au;
    const int rc = check_arguments(au, logits, tokens, masked, B, T, V, horizon, end_index, token_class, next_state, min_left,
                                   n_states, n_classes);
    if (rc != 0) return rc < 0 ? rc : 0;
    hipLaunchKernelGGL(grammar_logits_kernel<false>, dim3((B + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP), dim3(64 * ROWS_PER_GROUP), 0,
                       static_cast<hipStream_t>(stream), logits, logits_bstride, tokens, tok_bstride, masked, masked_bstride,
                       log_mass, outside, B, T, V, horizon, Specials{pad_index, unk_index, start_index}, au);
    return (int)hipGetLastError();
}

int pnmn_grammar_logits_bwd(const float* d_masked, int64_t d_masked_bstride, const int64_t* tokens, int64_t tok_bstride,
                            float* d_logits, int64_t d_logits_bstride, int B, int T, int V, int horizon, int pad_index,
                            int unk_index, int start_index, int end_index, const uint8_t* token_class, const uint8_t* next_state,
                            const uint8_t* min_left, int n_states, int n_classes, void* stream) {
    TokenAutomaton au;
    const int rc = check_arguments(au, d_masked, tokens, d_logits, B, T, V, horizon, end_index, token_class, next_state, min_left,
                                   n_states, n_classes);
    if (rc != 0) return rc < 0 ? rc : 0;
    hipLaunchKernelGGL(grammar_logits_kernel<true>, dim3((B + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP), dim3(64 * ROWS_PER_GROUP), 0,
                       static_cast<hipStream_t>(stream), d_masked, d_masked_bstride, tokens, tok_bstride, d_logits,
                       d_logits_bstride, static_cast<float*>(nullptr), static_cast<int32_t*>(nullptr), B, T, V, horizon,
                       Specials{pad_index, unk_index, start_index}, au);
    return (int)hipGetLastError();
}

}  // extern "C"
