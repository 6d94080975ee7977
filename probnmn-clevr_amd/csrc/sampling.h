// Wave-level helpers shared by the decoder kernels: reductions, the Philox4x32-10 uniform that
// pnmn_sample_tokens also uses, and one row's token choice from a row of logits in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"

namespace pnmn {

// Wave-wide sum / max on the VALU's data-parallel primitives (DPP): four steps inside each row of 16 lanes
// (quad swaps, half-row and row mirrors), two row broadcasts, one v_readlane -- every lane gets the result.  The
// __shfl_xor butterfly these replace compiles to six ds_bpermute_b32, i.e. six dependent trips through the LDS
// crossbar (~60 cycles each) per reduction; the decoder kernels do ~25 reductions per time step.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float identity, float v) {  // lanes without a source keep `identity`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v),
                                                                  CTRL, ROW_MASK, 0xF, false));
}
template <typename Op>
__device__ __forceinline__ float wave_reduce(float v, float identity, Op op) {
    v = op(v, dpp_move<0xB1, 0xF>(identity, v));   // quad_perm [1,0,3,2]
    v = op(v, dpp_move<0x4E, 0xF>(identity, v));   // quad_perm [2,3,0,1]
    v = op(v, dpp_move<0x141, 0xF>(identity, v));  // row_half_mirror
    v = op(v, dpp_move<0x140, 0xF>(identity, v));  // row_mirror: every lane = its row of 16
    v = op(v, dpp_move<0x142, 0xA>(identity, v));  // row_bcast:15 into rows 1, 3
    v = op(v, dpp_move<0x143, 0xC>(identity, v));  // row_bcast:31 into rows 2, 3: lane 63 = the wave
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wsum(float v) {
    return wave_reduce(v, 0.f, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ float wmax(float v) {
    return wave_reduce(v, -INFINITY, [](float a, float b) { return fmaxf(a, b); });
}

__device__ __forceinline__ void philox_round(uint32_t (&ctr)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * ctr[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    ctr[0] = hi1 ^ ctr[1] ^ k0;
    ctr[1] = lo1;
    ctr[2] = hi0 ^ ctr[3] ^ k1;
    ctr[3] = lo0;
}
// word 0 of Philox4x32-10 for (seed, row, step): the one stream every draw of the library comes from
__device__ inline uint32_t philox_word0(uint64_t seed, uint64_t row, uint32_t step) {
    uint32_t ctr[4] = {(uint32_t)row, (uint32_t)(row >> 32), step, 0x9E3779B9u};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(ctr, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ctr[0];
}
__device__ inline float philox_uniform(uint64_t seed, uint64_t row, uint32_t step) {  // same stream as pnmn_sample_tokens
    return (float)(philox_word0(seed, row, step) >> 8) * (1.0f / 16777216.0f);
}
// the same word as an odd multiple of 2^-24: 0 < u < 1 exactly in fp32, so neither log u nor log(-log u) meets 0 or 1
__device__ inline float philox_uniform_open(uint64_t seed, uint64_t row, uint32_t step) {
    return (float)(2u * (philox_word0(seed, row, step) >> 9) + 1u) * (1.0f / 16777216.0f);
}

// Inverse-CDF scan of one row's weights `w` (chunk k of a lane = index lane + 64k, index order): the first index with
// w > 0 whose inclusive prefix sum exceeds `target`; the last index with w > 0 when round-off leaves the target past the
// end; -1 when no weight is > 0.  Wave-uniform.
template <int K>
__device__ __forceinline__ int inverse_cdf(const float (&w)[K], float target) {
    const int lane = threadIdx.x & 63;
    float before = 0.f;
    int choice = -1, last_ok = -1;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float inc = w[k];  // inclusive prefix sum over lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float tt = __shfl_up(inc, o);
            if (lane >= o) inc += tt;
        }
        const unsigned long long hit = __ballot((w[k] > 0.f) && (before + inc > target));
        if (choice < 0 && hit) choice = 64 * k + (int)__ffsll((long long)hit) - 1;
        const unsigned long long pos = __ballot(w[k] > 0.f);
        if (pos) last_ok = 64 * k + 63 - __clzll((long long)pos);
        before += __shfl(inc, 63);
    }
    return choice < 0 ? last_ok : choice;
}

// The allowed set of a token choice, beyond the rule's fixed "every index but pad / unk / start": WholeSet adds nothing (and,
// being empty, changes neither the code nor the arguments of the functions below); LaneSet is a set the caller worked out per
// lane -- each lane answers for its own indices lane and lane + 64 (rows of V <= 128), so a set costs no reduction.  It
// replaces the fixed set and also bounds the arg-max of mode 2: the constrained decoders' A_c (allowed_lanes below).
struct WholeSet {
    static constexpr bool whole = true;
};
struct LaneSet {
    static constexpr bool whole = false;
    bool lo, hi;
    __device__ __forceinline__ bool has(int j) const { return j < 64 ? lo : hi; }
};

// First index j < V with ok(j) of the largest v, a NaN counting as larger than any number (torch.argmax); -1 when no
// index is ok.  Wave-uniform.
template <int K, typename Ok>
__device__ inline int first_argmax(const float (&v)[K], Ok ok) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long nan = __ballot(ok(lane + 64 * k) && v[k] != v[k]);
        if (nan) return 64 * k + (int)__ffsll((long long)nan) - 1;
    }
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (ok(lane + 64 * k)) m = fmaxf(m, v[k]);
    m = wmax(m);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long hit = __ballot(ok(lane + 64 * k) && v[k] == m);
        if (hit) return 64 * k + (int)__ffsll((long long)hit) - 1;
    }
    return -1;
}

// The token of a row the common path cannot serve (the rule is documented beside pnmn_sample_tokens in
// include/probnmn_hip.h): greedy over a row with a NaN; sampling over a row with a NaN or +inf, or whose allowed weights
// sum to 0.  `v` holds the row (entries j >= V are -inf), `u` the row's uniform.  Reached only through a wave-uniform
// branch that a finite row with positive allowed mass never takes.  `set` (a LaneSet): the allowed set in the place of the
// fixed one; it then also holds the greedy choice of a row with a NaN, which is the arg-max of this rule inside the set.
template <int K, class Set = WholeSet>
__device__ inline int choose_token_fallback(const float (&v)[K], int V, bool greedy, int pad, int unk, int start, float u,
                                            const Set set = Set{}) {
    const int lane = threadIdx.x & 63;
    const auto in_row = [V](int j) { return j < V; };
    const auto allowed = [=](int j) {
        if constexpr (Set::whole) return j < V && j != pad && j != unk && j != start;
        else return set.has(j);
    };
    if constexpr (!Set::whole) {
        if (greedy) {
            const int c = first_argmax(v, allowed);
            if (c >= 0) return c;
        }
    }
    if (!greedy) {
        bool bad = false;  // a NaN or +inf in the row
        float m = -INFINITY;  // largest allowed logit
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = lane + 64 * k;
            if (j < V) bad |= !(v[k] < INFINITY);
            if (allowed(j)) m = fmaxf(m, v[k]);
        }
        m = wmax(m);
        if (!__ballot(bad) && m > -INFINITY) {
            // finite row whose allowed weights underflowed: the same distribution relative to its largest allowed logit
            float w[K], tot = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                w[k] = allowed(lane + 64 * k) ? expf(v[k] - m) : 0.f;
                tot += w[k];
            }
            return inverse_cdf(w, u * wsum(tot));
        }
        const int c = first_argmax(v, allowed);
        if (c >= 0) return c;
    }
    return first_argmax(v, in_row);  // greedy, or no allowed token at all
}

// A sampling filter (temperature, top-k, top-p): the rule is stated beside pnmn_sample_tokens in
// include/probnmn_hip.h.  It travels by value in the launch arguments of the filtered kernels only.
struct SamplingFilter {
    float temperature;
    int top_k;
    float top_p;
};
// what an entry point checks of a filter it is given before it launches anything, and which filters change nothing
inline bool filter_valid(const pnmn_sampling_filter* f) {
    return f && isfinite(f->temperature) && f->temperature > 0.f && f->top_k >= 0 && f->top_p > 0.f && f->top_p <= 1.f;
}
inline bool filter_is_identity(const pnmn_sampling_filter& f) { return f.temperature == 1.f && f.top_k == 0 && f.top_p == 1.f; }

// The filtered draw of one row that is all finite and has a positive allowed total (the caller has checked both: every
// other row keeps choose_token_fallback).  `v` holds the row (chunk k of a lane = index lane + 64k), `wl` 64 K floats of
// LDS this wave owns -- in the decoders the logit row itself, dead once it is in `v`.
//   w_j = exp(z_j / temperature - max over the allowed), -1 for an index that is not allowed: it ranks before nothing
//   every lane walks j = 0 .. V-1 in ascending order (all lanes read wl[j]: a broadcast) and accumulates, per entry of
//   its own, how many indices rank before it (w_j larger, or equal and j smaller) and their weight: its rank and the
//   mass before it, in one fixed summation order -- no sort, no atomics
//   top-k keeps rank < top_k, top-p of those the ones with mass before < top_p x (total kept by top-k) and rank 0;
//   the draw is the index-order inverse CDF over what is left, from the row's usual uniform `u`.
// A pure function of the row and the filter, wave-uniform: the eight members of a multi-CU tile agree.
// `set` (a LaneSet): the rule's A replaced by that set.
template <int K, class Set = WholeSet>
__device__ inline int filtered_draw(const float (&v)[K], float* wl, int V, int pad, int unk, int start,
                                    const SamplingFilter& f, float u, const Set set = Set{}) {
    const int lane = threadIdx.x & 63;
    float w[K], m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
        if constexpr (Set::whole) w[k] = (j < V && j != pad && j != unk && j != start) ? v[k] / f.temperature : -INFINITY;
        else w[k] = set.has(j) ? v[k] / f.temperature : -INFINITY;
        m = fmaxf(m, w[k]);
    }
    m = wmax(m);  // finite: some allowed weight of the unfiltered distribution is positive
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
        if constexpr (Set::whole) w[k] = (j < V && j != pad && j != unk && j != start) ? expf(w[k] - m) : -1.f;
        else w[k] = set.has(j) ? expf(w[k] - m) : -1.f;
        wl[j] = w[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // one wave: its LDS accesses complete in order
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int rank[K];
    float mass[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rank[k] = 0, mass[k] = 0.f;
    for (int j = 0; j < V; ++j) {
        const float wj = wl[j];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool before = wj > w[k] || (wj == w[k] && j < lane + 64 * k);
            rank[k] += before ? 1 : 0;
            mass[k] += before ? wj : 0.f;
        }
    }
    float kept[K], tot = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        kept[k] = (w[k] >= 0.f && (f.top_k <= 0 || rank[k] < f.top_k)) ? w[k] : 0.f;
        tot += kept[k];
    }
    tot = wsum(tot);  // (>= 1: the first-ranked index weighs exp(0))
    if (f.top_p < 1.f) {
        const float cut = f.top_p * tot;
        float left = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!(mass[k] < cut) && rank[k] > 0) kept[k] = 0.f;
            left += kept[k];
        }
        tot = wsum(left);
    }
    return inverse_cdf(kept, u * tot);
}

// One wave picks one row's token from `logits` (LDS, V <= 128 entries): mode 2 = first arg-max,
// mode 1 = inverse-CDF draw from softmax(logits) with pad / unk / start removed (reference
// seq2seq_base.py:203-220); rows that are not all finite follow choose_token_fallback.  The result is
// wave-uniform and always in [0, V).  FILT: mode 1 draws under the filter `f` instead (filtered_draw, which overwrites
// the 128 floats at `wl`); the rows the fallback serves, and mode 2, ignore it.
// `set` (a LaneSet): the draw, filtered or not, and the fallback are restricted to that set instead of "all but pad / unk /
// start", and so is the arg-max of mode 2; the softmax itself is always that of the whole row.
template <bool FILT = false, class Set = WholeSet>
__device__ inline int choose_row_token(const float* logits, int V, int mode, int pad, int unk, int start, uint64_t seed,
                                       uint64_t global_row, uint32_t t, float* wl = nullptr,
                                       const SamplingFilter& f = SamplingFilter{1.f, 0, 1.f}, const Set set = Set{}) {
    const int lane = threadIdx.x & 63;
    float v[2];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        v[k] = j < V ? logits[j] : -INFINITY;
        mx = fmaxf(mx, v[k]);
    }
    mx = wmax(mx);
    int choice;
    if (mode == 2) {
        int best = 0x7fffffff;
        if constexpr (Set::whole) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (lane + 64 * k < V && v[k] == mx && lane + 64 * k < best) best = lane + 64 * k;
        } else {
            float ms = -INFINITY;  // the largest logit inside the set
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (set.has(lane + 64 * k)) ms = fmaxf(ms, v[k]);
            ms = wmax(ms);
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (set.has(lane + 64 * k) && v[k] == ms && lane + 64 * k < best) best = lane + 64 * k;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        choice = best;
        if (__ballot(v[0] != v[0] || v[1] != v[1])) choice = choose_token_fallback(v, V, true, pad, unk, start, 0.f, set);
    } else {
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) se += (lane + 64 * k < V) ? expf(v[k] - mx) : 0.f;
        const float lse = mx + logf(wsum(se));
        float w[2], tot = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = lane + 64 * k;
            bool ok;
            if constexpr (Set::whole) ok = j < V && j != pad && j != unk && j != start;
            else ok = set.has(j);
            w[k] = ok ? expf(v[k] - lse) : 0.f;
            tot += w[k];
        }
        tot = wsum(tot);
        const float u = philox_uniform(seed, global_row, t);
        if (tot > 0.f) {  // (a NaN or +inf anywhere in the row makes the total NaN)
            if constexpr (FILT) choice = filtered_draw(v, wl, V, pad, unk, start, f, u, set);
            else choice = inverse_cdf(w, u * tot);
        } else {
            choice = choose_token_fallback(v, V, false, pad, unk, start, u, set);
        }
    }
    return min(max(choice, 0), V - 1);
}

// ---- the token automaton of the constrained decoders (the rule: include/probnmn_hip.h, beside pnmn_attn_lstm_fwd) ----
// The tables as the entry points check them and as they travel BY VALUE in the launch arguments; a workgroup stages them
// into LDS once (stage_automaton).  Unused entries are 0.
constexpr int AUTOMATON_STATES = PNMN_BEAM_MAX_STATES, AUTOMATON_CLASSES = PNMN_BEAM_MAX_CLASSES, AUTOMATON_TOKENS = 128;
struct TokenAutomaton {
    unsigned char token_class[AUTOMATON_TOKENS];                     // [V], < n_classes
    unsigned char next_state[AUTOMATON_STATES * AUTOMATON_CLASSES];  // [n_states][n_classes] packed, < n_states
    unsigned char min_left[AUTOMATON_STATES];                        // [n_states]; 255: no completion exists
    int n_classes, end;
};
constexpr int AUTOMATON_LDS_BYTES = AUTOMATON_TOKENS + AUTOMATON_STATES * AUTOMATON_CLASSES + AUTOMATON_STATES;  // 672
static_assert(AUTOMATON_STATES * AUTOMATON_CLASSES == 512 && AUTOMATON_TOKENS <= 512, "staged by 512 threads, one entry each");

// What an entry point checks of the tables it is given before it launches anything: 0 and `out` filled, or PNMN_EINVAL.  V, T: of the
// free-running passes the automaton applies to; V = 0 when there is none (a teacher-forced call: the tables are checked as far
// as they can be without a vocabulary, and ignored).
inline int fill_automaton(TokenAutomaton& out, const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left,
                          int n_states, int n_classes, int V, int T, int end_index) {
    out = TokenAutomaton{};
    if (!token_class || !next_state || !min_left) return PNMN_EINVAL;
    if (n_states < 1 || n_states > AUTOMATON_STATES || n_classes < 1 || n_classes > AUTOMATON_CLASSES) return PNMN_EINVAL;
    if (V != 0 && (V < 1 || V > AUTOMATON_TOKENS || end_index < 0 || end_index >= V)) return PNMN_EINVAL;
    for (int v = 0; v < V; ++v) {
        if (token_class[v] >= n_classes) return PNMN_EINVAL;
        out.token_class[v] = token_class[v];
    }
    for (int i = 0; i < n_states * n_classes; ++i) {
        if (next_state[i] >= n_states) return PNMN_EINVAL;
        out.next_state[i] = next_state[i];
    }
    for (int s = 0; s < n_states; ++s) out.min_left[s] = min_left[s];
    if (V != 0 && (int)min_left[0] > T) return PNMN_EINVAL;  // no accepted string fits the steps: A_c would run empty
    out.n_classes = n_classes;
    out.end = end_index;
    return 0;
}

// the staged tables: three byte arrays in `AUTOMATON_LDS_BYTES` of LDS
struct AutomatonLds {
    const unsigned char *cls, *next, *left;
    int ncls, end;
};
// all 512 threads of a workgroup, before a barrier of the caller's
__device__ __forceinline__ AutomatonLds stage_automaton(unsigned char* lds, const TokenAutomaton& au) {
    const int tid = threadIdx.x;
    unsigned char *cls = lds, *next = cls + AUTOMATON_TOKENS, *left = next + AUTOMATON_STATES * AUTOMATON_CLASSES;
    next[tid] = au.next_state[tid];
    if (tid < AUTOMATON_TOKENS) cls[tid] = au.token_class[tid];
    if (tid < AUTOMATON_STATES) left[tid] = au.min_left[tid];
    return AutomatonLds{cls, next, left, au.n_classes, au.end};
}
// A row's automaton state as the wave that chooses its tokens carries it: bits 0-7 the state, bit 8 = the row has finished.
constexpr int ROW_FINISHED = 256;
// A_c(s, t) of a row, each lane answering for its indices lane, lane + 64: `left` = T - 1 - t.  A finished row: end_index alone.
// All lanes of a wave read the same two state bytes (LDS broadcasts); the class and next-state bytes are per lane.
__device__ __forceinline__ LaneSet allowed_lanes(const AutomatonLds& au, int row_state, int left, int V, int pad, int unk, int start) {
    const int lane = threadIdx.x & 63;
    const bool finished = (row_state & ROW_FINISHED) != 0;
    const int s = row_state & 255;
    const int room = left < 254 ? left : 254;  // (255 marks a state without completion, however many steps remain)
    const bool may_end = finished || au.left[s] == 0;
    bool in[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        const bool token = !finished && j != pad && j != unk && j != start && (int)au.left[au.next[s * au.ncls + au.cls[j]]] <= room;
        in[k] = j < V && (j == au.end ? may_end : token);
    }
    return LaneSet{in[0], in[1]};
}
// the row's state behind its token (wave-uniform in, wave-uniform out)
__device__ __forceinline__ int advance_row_state(const AutomatonLds& au, int row_state, int token) {
    if (row_state & ROW_FINISHED) return row_state;
    if (token == au.end) return row_state | ROW_FINISHED;
    return __builtin_amdgcn_readfirstlane((int)au.next[row_state * au.ncls + au.cls[token]]);
}

}  // namespace pnmn
