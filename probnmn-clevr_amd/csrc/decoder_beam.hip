// Persistent beam-search decoder (inference only, hidden = 256) for gfx950.
//
// The free-running decoder of decoder.hip owns 16 INDEPENDENT rows per workgroup.  Beam search couples rows: the K
// hypotheses of a question compete every step and the survivors' h, c and last token are re-gathered by back-pointer.
// Here one workgroup owns one 16-row MFMA tile = 16/K questions x K hypotheses (row = question * K + slot) for all T
// steps, so a question's whole competition stays inside one workgroup: LDS and __syncthreads, no wait on any other
// workgroup.  Per step:
//     attention   as attn_lstm_fwd_kernel; wave w owns rows 2w, 2w+1, which for K >= 2 belong to ONE question, so
//                 each encoder row the wave fetches serves both hypotheses (enc / mask / h0 are per question)
//     gates, cell as attn_lstm_fwd_kernel (same packed-weight fragment order, 16x16x4 f32 MFMA)
//     logits      h W_p^T + b_p over the full vocabulary -> LDS
//     candidates  cand[k][v] = score[k] + log_softmax(logits[k])[v] with pad / unk / start removed; a finished
//                 hypothesis offers only @end@ at its own score; a non-finite candidate counts as -inf
//     selection   K rounds of (largest candidate, smallest flat index k*V+v among equals): every wave over its two rows,
//                 then one wave per question over the question's K/2 lists
//     gather      h (LDS -> LDS), c (registers -> LDS -> registers) and the last token by back-pointer; the step's
//                 (token, back-pointer) of every slot stays in LDS for the back-track after the last step
// The masked softmax of the attention, the gate product and the logits tile are the functions of decoder_stages.h that
// attn_lstm_fwd_kernel (decoder.hip) runs too; the loops over the encoder rows and the cell are restated here without that
// kernel's stores for the backward.
// Nothing is saved for a backward pass: the only global writes are tokens / scores and the optional per-step trace.
//
// Constrained variant (pnmn_attn_lstm_beam with tables, template parameter C): every slot also carries one byte, the state
// of a token automaton (class of every token, next state per class, fewest further tokens to an accepting state).  The
// three tables arrive by value in the launch arguments and are staged into LDS once; the candidate stage alone differs:
// a live hypothesis offers a token only if an accepting state stays reachable in the steps that remain, and @end@ only in
// an accepting state.  Selection, gather, early stop and back-track are the unconstrained ones; the survivors' states
// follow the back-pointers like their last tokens.
//
// Stochastic variant (pnmn_attn_lstm_beam_stochastic, template parameter ST, with or without C): every slot also carries G, its
// perturbed log-probability.  Again the candidate stage alone differs (stochastic_candidates): log-probabilities renormalised
// over the offered tokens, one Philox uniform per candidate, G~ conditioned on the parent's G; the selection ranks G~ and a
// survivor takes its candidate's phi from a second [16][128] array.  The K survivors are a sample without replacement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"
#include "decoder_stages.h"
#include "sampling.h"

using pnmn::f32x4;

namespace {

constexpr int H = 256;
constexpr int G4 = 4 * H;
constexpr int ROWS = 16;
constexpr int LD = H + 4;
constexpr int MAXS = 64;   // encoder positions
constexpr int MAXV = 128;  // target vocabulary
constexpr int MAXT = 64;   // decoding steps

using pnmn::sigm;
using pnmn::wmax;
using pnmn::wsum;

struct BeamArgs {
    const float* etable;    // [V][4H]  Emb W_e^T + b
    const float* enc;       // [B][S][H]   per QUESTION
    const float* mask;      // [B][S] 1/0
    const float* h0;        // [B][H]
    const float* w_c;       // [4H][H] fragment order
    const float* w_hh;      // [4H][H] fragment order
    const float* w_p;       // [V][H]
    const float* b_p;       // [V]
    int64_t* tokens;        // [B][K][T] best first
    float* scores;          // [B][K]
    int32_t* trace_tokens;  // [B][T][K] or nullptr
    int32_t* trace_backptr; // [B][T][K] or nullptr
    float* trace_scores;    // [B][T][K] or nullptr
    int B, T, S, V;
    int pad, unk, start, end;
};

constexpr int MAX_STATES = PNMN_BEAM_MAX_STATES;    // token automaton of the constrained search
constexpr int MAX_CLASSES = PNMN_BEAM_MAX_CLASSES;
constexpr int DEAD = 255;  // min_left: no completion exists
static_assert(MAX_STATES * MAX_CLASSES == 512 && MAXV <= 512 && (MAXV & (MAXV - 1)) == 0, "staged by 512 threads, one entry each");

struct ConstrainedBeamArgs : BeamArgs {
    unsigned char token_class[MAXV];                     // [V], < n_classes
    unsigned char next_state[MAX_STATES * MAX_CLASSES];  // [n_states][n_classes] packed, < n_states
    unsigned char min_left[MAX_STATES];                  // [n_states]
    int n_classes;
};

// stochastic beam search (pnmn_attn_lstm_beam_stochastic, template parameter ST): what it takes beyond the plain search's
template <class Base>
struct StochasticArgs : Base {
    float* perturbed;        // [B][K] G of every returned hypothesis, best first
    float* trace_perturbed;  // [B][T][K] or nullptr
    uint64_t seed;
    int64_t question_offset;
};

template <bool C, bool ST = false>
struct beam_args {
    using base = std::conditional_t<C, ConstrainedBeamArgs, BeamArgs>;
    using type = std::conditional_t<ST, StochasticArgs<base>, base>;
};

// Attention of NH hypotheses that share one question's encoder rows (`er` = enc row 0 of the question + 4 * lane):
// scores = enc . h, AllenNLP masked softmax, ctx = w . enc.  One wave; every encoder row is fetched once per pass for
// all NH hypotheses.
template <int NH>
__device__ __forceinline__ void attend(const float* er, const float* mrow, int S, const float (*h)[LD], float (*ctx)[LD]) {
    const int lane = threadIdx.x & 63;
    f32x4 hv[NH];
    float myscore[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        hv[n] = *reinterpret_cast<const f32x4*>(&h[n][4 * lane]);
        myscore[n] = 0.f;
    }
    for (int s0 = 0; s0 < S; s0 += 8) {
        f32x4 e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k < S ? s0 + k : S - 1;
            e[k] = *reinterpret_cast<const f32x4*>(er + (size_t)s * H);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int n = 0; n < NH; ++n) {
                const float p = wsum(e[k].x * hv[n].x + e[k].y * hv[n].y + e[k].z * hv[n].z + e[k].w * hv[n].w);
                if (lane == s0 + k) myscore[n] = p;
            }
    }
    const float m = lane < S ? mrow[lane] : 0.f;
    float wgt[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        float p;
        wgt[n] = pnmn::attention_weight(myscore[n], m, S, lane, p);
    }
    f32x4 c4[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) c4[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < S; s0 += 8) {
        f32x4 e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k < S ? s0 + k : S - 1;
            e[k] = *reinterpret_cast<const f32x4*>(er + (size_t)s * H);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int n = 0; n < NH; ++n) {
                const float ws = s0 + k < S ? __shfl(wgt[n], s0 + k) : 0.f;
                c4[n] += e[k] * ws;
            }
    }
#pragma unroll
    for (int n = 0; n < NH; ++n) *reinterpret_cast<f32x4*>(&ctx[n][4 * lane]) = c4[n];
}

// R rounds of (largest value; among equals the smallest index) over a wave's candidates, N (value, index) pairs per lane with
// index -1 where the value is -inf: lane j < R receives the j-th best, (-inf, -1) when nothing finite was left for it.
template <int N, int R>
__device__ __forceinline__ void wave_top(float (&val)[N], const int (&idx)[N], float& my_val, int& my_idx) {
    const int lane = threadIdx.x & 63;
    my_val = -INFINITY;
    my_idx = -1;
    for (int round = 0; round < R; ++round) {
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < N; ++i) m = fmaxf(m, val[i]);
        m = wmax(m);
        if (m == -INFINITY) break;  // wave-uniform: nothing finite is left
        float first = -INFINITY;    // the smallest index holding m, as a max over the negated index: < 2048, exact in fp32
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (val[i] == m) first = fmaxf(first, -(float)idx[i]);
        const int best = (int)(-wmax(first));
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (idx[i] == best) val[i] = -INFINITY;  // taken
        if (lane == round) {
            my_val = m;
            my_idx = best;
        }
    }
}

// The candidates of rows 2w, 2w+1 under stochastic beam search (Kool, van Hoof and Welling 2019; the rule: include/probnmn_hip.h,
// beside pnmn_attn_lstm_beam_stochastic), by wave w: logl[row] turns from logits into G~, the perturbed value the selection
// ranks by, and phil[row] receives phi, the log-probability renormalised over the offered tokens.  `offered(row, j)`: the
// plain search's test of a live hypothesis' token; `draw_row(row)`: (question_offset + question) * 16 + slot.  A lane
// answers for tokens lane and lane + 64 of both rows: four Philox draws per lane and step, no LDS traffic beyond the two
// stores, no barrier of its own.
template <class Offered, class DrawRow>
__device__ __forceinline__ void stochastic_candidates(float (*logl)[MAXV], float (*phil)[MAXV], const float* scorel, const float* gl,
                                                      const int* tokl, int end, uint64_t seed, uint32_t t, Offered offered,
                                                      DrawRow draw_row) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int rl = 2 * wave + rr;
        const float score = scorel[rl], G = gl[rl];
        const bool finished = tokl[rl] == end;
        float v[2], mx = -INFINITY;
        bool in[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = lane + 64 * k;
            v[k] = logl[rl][j];  // (-inf at and past V)
            in[k] = !finished && offered(rl, j) && v[k] > -INFINITY && v[k] < INFINITY;  // offered, with a finite logit
            if (in[k]) mx = fmaxf(mx, v[k]);
        }
        mx = wmax(mx);
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) se += in[k] ? expf(v[k] - mx) : 0.f;
        const float lse = mx + logf(wsum(se));
        float phi[2], gum[2], Z = -INFINITY;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            phi[k] = in[k] ? score + (v[k] - lse) : -INFINITY;
            if (!(phi[k] > -INFINITY && phi[k] < INFINITY)) phi[k] = -INFINITY;
            gum[k] = -INFINITY;
            if (phi[k] > -INFINITY) {
                const float u = pnmn::philox_uniform_open(seed, draw_row(rl) * MAXV + (lane + 64 * k), t);
                gum[k] = phi[k] - logf(-logf(u));
            }
            Z = fmaxf(Z, gum[k]);
        }
        Z = wmax(Z);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = lane + 64 * k;
            float key = -INFINITY;
            if (phi[k] > -INFINITY) {
                // G~ = -log(exp(-G) - exp(-Z) + exp(-g)) without its cancellation: w = G - g + log(1 - exp(g - Z)),
                // G~ = G - max(0, w) - log1p(exp(-|w|)); the arg-max child has w = -inf and keeps G
                const float d = gum[k] - Z;  // <= 0
                const float w = G - gum[k] + (d > -0.6931472f ? logf(-expm1f(d)) : log1pf(-expf(d)));
                key = G - fmaxf(0.f, w) - log1pf(expf(-fabsf(w)));
                if (!(key > -INFINITY && key < INFINITY)) key = phi[k] = -INFINITY;  // a non-finite candidate counts as -inf
            }
            if (finished && j == end && score > -INFINITY && G > -INFINITY && G < INFINITY) {
                phi[k] = score;  // a finished hypothesis offers only @end@, phi and G unchanged; no uniform is drawn for it
                key = G;
            }
            logl[rl][j] = key;
            phil[rl][j] = phi[k];
        }
    }
}

template <int K, bool C, bool ST = false>
__global__ __launch_bounds__(512) void attn_lstm_beam_kernel(const typename beam_args<C, ST>::type a) {
    constexpr int Q = ROWS / K;  // questions per workgroup
    __shared__ __attribute__((aligned(16))) float hl[2][ROWS][LD];  // [0]: h the step reads, [1]: h the cell wrote
    __shared__ __attribute__((aligned(16))) float cl[ROWS][LD];     // ctx; after the cell: c on its way through the gather
    __shared__ float logl[ROWS][MAXV];                              // logits, then candidates
    __shared__ float scorel[ROWS];
    __shared__ int tokl[ROWS];                                      // last token of every slot
    __shared__ int bpl[ROWS];                                       // back-pointer of the step (row inside the tile)
    __shared__ unsigned char tok_hist[MAXT][ROWS], bp_hist[MAXT][ROWS];
    __shared__ float top_val[8][ROWS];                              // selection: every wave's K best (value, candidate)
    __shared__ int top_idx[8][ROWS];
    // constrained search only: the automaton, and the state of every slot ([0]: the step reads, [1]: the survivors')
    __shared__ unsigned char clsl[C ? MAXV : 1], nextl[C ? MAX_STATES * MAX_CLASSES : 1], leftl[C ? MAX_STATES : 1];
    __shared__ unsigned char statel[2][C ? ROWS : 1];
    // stochastic search only: phi of every candidate beside its perturbed value in logl, and G of every slot
    __shared__ float phil[ST ? ROWS : 1][ST ? MAXV : 1];
    __shared__ float gl[ST ? ROWS : 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * Q;  // first question of this tile
    const int T = a.T, S = a.S, V = a.V;

    for (int i = tid; i < ROWS * H; i += 512) {
        const int r = i / H, k = i - r * H, q = q0 + r / K;
        hl[0][r][k] = q < a.B ? a.h0[(size_t)q * H + k] : 0.f;
    }
    if (tid < ROWS) {
        const bool live = q0 + tid / K < a.B;
        tokl[tid] = live ? a.start : a.end;  // (a tile row past the batch counts as finished)
        scorel[tid] = (tid % K == 0) ? 0.f : -INFINITY;  // step 0 expands ONE state per question
        if constexpr (ST) gl[tid] = (tid % K == 0) ? 0.f : -INFINITY;
    }
    int ncls = 1;
    if constexpr (C) {
        ncls = a.n_classes;
        clsl[tid & (MAXV - 1)] = a.token_class[tid & (MAXV - 1)];  // (512 threads: every entry, some four times over)
        nextl[tid] = a.next_state[tid];                            // (MAX_STATES * MAX_CLASSES = 512)
        if (tid < MAX_STATES) leftl[tid] = a.min_left[tid];
        if (tid < ROWS) statel[0][tid] = statel[1][tid] = 0;  // the start state
    }
    float creg[2][4];
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int r = 0; r < 4; ++r) creg[ut][r] = 0.f;
    __syncthreads();

    int done = T;  // steps decoded before every hypothesis of the tile had finished
    for (int t = 0; t < T; ++t) {
        // ---------------- attention: wave w owns rows 2w, 2w+1 ----------------
        if constexpr (K >= 2) {
            const int rl = 2 * wave, q = q0 + rl / K;  // both rows: the same question
            if (q < a.B) {                             // wave-uniform
                attend<2>(a.enc + (size_t)q * S * H + 4 * lane, a.mask + (size_t)q * S, S, &hl[0][rl], &cl[rl]);
            } else {
                *reinterpret_cast<f32x4*>(&cl[rl][4 * lane]) = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(&cl[rl + 1][4 * lane]) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int rl = 2 * wave + rr, q = q0 + rl;
                if (q < a.B)
                    attend<1>(a.enc + (size_t)q * S * H + 4 * lane, a.mask + (size_t)q * S, S, &hl[0][rl], &cl[rl]);
                else
                    *reinterpret_cast<f32x4*>(&cl[rl][4 * lane]) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();

        // ---------------- gates on the matrix cores ----------------
        f32x4 acc[4][2];
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = 4 * g + r;
                    const int n = gate * H + 32 * wave + 16 * ut + li;
                    acc[gate][ut][r] = (q0 + rl / K < a.B) ? a.etable[(size_t)tokl[rl] * G4 + n] : 0.f;
                }
        pnmn::gates_mfma<H, LD>(acc, cl, hl[0], a.w_c, a.w_hh, wave, lane);
        // ---------------- cell ----------------
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = 32 * wave + 16 * ut + li;
                const float ig = sigm(acc[0][ut][r]), fg = sigm(acc[1][ut][r]);
                const float gg = tanhf(acc[2][ut][r]), og = sigm(acc[3][ut][r]);
                const float c = fg * creg[ut][r] + ig * gg;
                creg[ut][r] = c;
                hl[1][4 * g + r][u] = og * tanhf(c);
            }
        __syncthreads();

        // ---------------- c into LDS for the gather (every wave is past its gates: cl is free); logits ----------------
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int r = 0; r < 4; ++r) cl[4 * g + r][32 * wave + 16 * ut + li] = creg[ut][r];
        {
            const int vn = 16 * wave + li;  // 16 rows x 16 vocabulary entries per wave
            const bool vok = vn < V;
            f32x4 lacc = f32x4{0.f, 0.f, 0.f, 0.f};
            if (16 * wave < V) lacc = pnmn::logits_tile<H, LD>(hl[1], a.w_p, V, wave, lane);
            const float bias = vok ? a.b_p[vn] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) logl[4 * g + r][vn] = vok ? lacc[r] + bias : -INFINITY;  // (vn < 128 = MAXV)
        }
        __syncthreads();

        // ---------------- candidates: wave w turns the logits of rows 2w, 2w+1 into score + log-probability ----------------
        if constexpr (ST) {
            const auto offered = [&](int rl, int j) {
                bool ok = j < V && j != a.pad && j != a.unk && j != a.start;
                if constexpr (C) {
                    if (ok) {  // the constrained search's test, below
                        const int st = statel[0][rl];
                        const int left = j == a.end ? (leftl[st] == 0 ? 0 : DEAD) : leftl[nextl[st * ncls + clsl[j]]];
                        ok = left <= T - 1 - t;
                    }
                }
                return ok;
            };
            const auto draw_row = [&](int rl) { return ((uint64_t)a.question_offset + (uint64_t)(q0 + rl / K)) * ROWS + rl % K; };
            stochastic_candidates(logl, phil, scorel, gl, tokl, a.end, a.seed, (uint32_t)t, offered, draw_row);
        } else {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int rl = 2 * wave + rr;
                float v[2], mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    v[k] = logl[rl][lane + 64 * k];  // (-inf at and past V)
                    mx = fmaxf(mx, v[k]);
                }
                mx = wmax(mx);
                float se = 0.f;
#pragma unroll
                for (int k = 0; k < 2; ++k) se += (lane + 64 * k < V) ? expf(v[k] - mx) : 0.f;
                const float lse = mx + logf(wsum(se));
                const float score = scorel[rl];
                const bool finished = tokl[rl] == a.end;
                int st = 0;
                if constexpr (C) st = statel[0][rl];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int j = lane + 64 * k;
                    float cand = -INFINITY;
                    if (finished) {
                        if (j == a.end) cand = score;  // a finished hypothesis keeps its score
                    } else if (j < V && j != a.pad && j != a.unk && j != a.start) {
                        cand = score + (v[k] - lse);
                        if constexpr (C) {
                            // @end@: only in an accepting state; any other token: an accepting state must stay reachable in
                            // the T - 1 - t steps after this one (DEAD = 255 > any step count)
                            const int left = j == a.end ? (leftl[st] == 0 ? 0 : DEAD) : leftl[nextl[st * ncls + clsl[j]]];
                            if (left > T - 1 - t) cand = -INFINITY;
                        }
                    }
                    if (!(cand > -INFINITY && cand < INFINITY)) cand = -INFINITY;  // a non-finite candidate counts as -inf
                    logl[rl][j] = cand;
                }
            }
        }
        __syncthreads();

        // ---------------- selection ----------------
        // Stage 1, all eight waves: wave w ranks the candidates of its rows 2w, 2w+1 (two hypotheses of one question; K = 1:
        // two questions, one after the other) and keeps their K best -- the question's K best are among these lists.
        // Stage 2 (K >= 4), one wave per question: the K best of the question's K/2 lists.  The order is the same in both.
        const auto commit = [&](int rl, float score, int flat) {  // slot rl of the tile takes candidate `flat` of its question
            const int bp = flat < 0 ? 0 : flat / V;               // (flat < 0: a slot left without a finite candidate)
            const int tok = flat < 0 ? a.end : flat - bp * V;
            if constexpr (ST) {  // ranked by G~: the survivor takes it, and its candidate's phi
                gl[rl] = score;
                score = flat < 0 ? -INFINITY : phil[(rl / K) * K + bp][tok];
            }
            scorel[rl] = score;
            bpl[rl] = (rl / K) * K + bp;
            tokl[rl] = tok;
            tok_hist[t][rl] = (unsigned char)tok;
            bp_hist[t][rl] = (unsigned char)bp;
            if constexpr (C) {  // the state reached from the parent's on the token; @end@ leaves it where it is
                const int ps = statel[0][(rl / K) * K + bp];
                statel[1][rl] = tok == a.end ? (unsigned char)ps : nextl[ps * ncls + clsl[tok]];
            }
            if (a.trace_tokens) {
                const size_t o = ((size_t)(q0 + rl / K) * T + t) * K + rl % K;
                a.trace_tokens[o] = tok;
                a.trace_backptr[o] = bp;
                a.trace_scores[o] = score;
                if constexpr (ST) a.trace_perturbed[o] = gl[rl];
            }
        };
#pragma unroll
        for (int grp = 0; grp < (K == 1 ? 2 : 1); ++grp) {
            constexpr int GR = K == 1 ? 1 : 2;  // rows ranked together
            const int r0 = 2 * wave + grp;
            if (q0 + r0 / K >= a.B) continue;  // wave-uniform
            float val[2 * GR];
            int idx[2 * GR];
#pragma unroll
            for (int rr = 0; rr < GR; ++rr)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int v = lane + 64 * j;
                    val[2 * rr + j] = logl[r0 + rr][v];  // (-inf at and past V)
                    idx[2 * rr + j] = v < V ? ((r0 + rr) % K) * V + v : -1;
                }
            float best;
            int flat;
            wave_top<2 * GR, K>(val, idx, best, flat);
            if (lane < K) {
                if (K <= 2) {
                    commit((r0 / K) * K + lane, best, flat);
                } else {
                    top_val[wave][lane] = best;
                    top_idx[wave][lane] = flat;
                }
            }
        }
        if constexpr (K >= 4) {
            __syncthreads();
            if (wave < Q && q0 + wave < a.B) {  // wave-uniform
                constexpr int E = K * K / 2, N2 = (E + 63) / 64;  // the question's K/2 lists of K entries
                float val[N2];
                int idx[N2];
#pragma unroll
                for (int n = 0; n < N2; ++n) {
                    const int e = lane + 64 * n;
                    val[n] = e < E ? top_val[wave * (K / 2) + e / K][e % K] : -INFINITY;
                    idx[n] = e < E ? top_idx[wave * (K / 2) + e / K][e % K] : -1;
                }
                float best;
                int flat;
                wave_top<N2, K>(val, idx, best, flat);
                if (lane < K) commit(wave * K + lane, best, flat);
            }
        }
        __syncthreads();

        // ---------------- gather the survivors' h and c by back-pointer ----------------
        for (int i = tid; i < ROWS * (H / 4); i += 512) {
            const int r = i / (H / 4), k4 = i - r * (H / 4);
            const int src = (q0 + r / K < a.B) ? bpl[r] : r;
            *reinterpret_cast<f32x4*>(&hl[0][r][4 * k4]) = *reinterpret_cast<const f32x4*>(&hl[1][src][4 * k4]);
        }
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = 4 * g + r;
                const int src = (q0 + rl / K < a.B) ? bpl[rl] : rl;
                creg[ut][r] = cl[src][32 * wave + 16 * ut + li];
            }
        if constexpr (C) {
            if (tid < ROWS) statel[0][tid] = statel[1][tid];  // (tile rows past the batch: never read)
        }
        // (also the barrier between this gather and the next step's writes to cl)
        if (__syncthreads_and(tid < ROWS ? tokl[tid] == a.end : 1)) {
            done = t + 1;
            break;
        }
    }

    // ---------------- every hypothesis finished early: the remaining steps only repeat @end@ ----------------
    // (the survivors are already best first, so each finite slot points at itself; a -inf slot has no finite candidate)
    if (tid < ROWS && q0 + tid / K < a.B) {
        const int q = q0 + tid / K, slot = tid % K;
        const float score = scorel[tid];
        const int bp = score > -INFINITY ? slot : 0;
        for (int t = done; t < T; ++t) {
            tok_hist[t][tid] = (unsigned char)a.end;
            bp_hist[t][tid] = (unsigned char)bp;
            if (a.trace_tokens) {
                const size_t o = ((size_t)q * T + t) * K + slot;
                a.trace_tokens[o] = a.end;
                a.trace_backptr[o] = bp;
                a.trace_scores[o] = score;
                if constexpr (ST) a.trace_perturbed[o] = gl[tid];
            }
        }
    }
    __syncthreads();
    // ---------------- back-track: hypothesis `slot` of the last step, best first ----------------
    if (tid < ROWS && q0 + tid / K < a.B) {
        const int q = q0 + tid / K, base = (tid / K) * K;
        int64_t* out = a.tokens + ((size_t)q * K + tid % K) * T;
        int cur = tid % K;
        for (int t = T - 1; t >= 0; --t) {
            out[t] = tok_hist[t][base + cur];
            cur = bp_hist[t][base + cur];
        }
        a.scores[(size_t)q * K + tid % K] = scorel[tid];
        if constexpr (ST) a.perturbed[(size_t)q * K + tid % K] = gl[tid];
    }
}

template <int K, bool C, bool ST>
int launch_beam(const typename beam_args<C, ST>::type& a, hipStream_t stream) {
    constexpr int Q = ROWS / K;
    hipLaunchKernelGGL((attn_lstm_beam_kernel<K, C, ST>), dim3((a.B + Q - 1) / Q), dim3(512), 0, stream, a);
    return (int)hipGetLastError();
}

template <bool C, bool ST>
int launch_beam_width(int beam, const typename beam_args<C, ST>::type& a, hipStream_t stream) {
    switch (beam) {
        case 1: return launch_beam<1, C, ST>(a, stream);
        case 2: return launch_beam<2, C, ST>(a, stream);
        case 4: return launch_beam<4, C, ST>(a, stream);
        case 8: return launch_beam<8, C, ST>(a, stream);
        case 16: return launch_beam<16, C, ST>(a, stream);
        default: return PNMN_EINVAL;
    }
}

// what pnmn_attn_lstm_beam_stochastic takes beyond pnmn_attn_lstm_beam
struct StochasticPart {
    float* perturbed;
    float* trace_perturbed;
    uint64_t seed;
    int64_t question_offset;
};

// the plain search (st == nullptr) or the stochastic one over the same arguments
template <bool C>
int launch_search(int beam, const typename beam_args<C>::type& a, const StochasticPart* st, hipStream_t stream) {
    if (!st) return launch_beam_width<C, false>(beam, a, stream);
    typename beam_args<C, true>::type sa{};
    static_cast<typename beam_args<C>::type&>(sa) = a;
    sa.perturbed = st->perturbed;
    sa.trace_perturbed = st->trace_perturbed;
    sa.seed = st->seed;
    sa.question_offset = st->question_offset;
    return launch_beam_width<C, true>(beam, sa, stream);
}

// the checks and the launch both entry points share
int beam_entry(const float* etable, const float* enc, const float* mask, const float* h0, const float* w_c, const float* w_hh,
               const float* w_p, const float* b_p, int64_t* tokens, float* scores, int32_t* trace_tokens, int32_t* trace_backptr,
               float* trace_scores, int B, int T, int S, int V, int hidden, int beam, int pad_index, int unk_index,
               int start_index, int end_index, const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left,
               int n_states, int n_classes, const StochasticPart* st, void* stream) {
    if (B < 0 || T < 0) return PNMN_EINVAL;
    if (!etable || !enc || !mask || !h0 || !w_c || !w_hh || !w_p || !b_p || !tokens || !scores) return PNMN_EINVAL;
    const int traced = (trace_tokens != nullptr) + (trace_backptr != nullptr) + (trace_scores != nullptr);
    if (traced != 0 && traced != 3) return PNMN_EINVAL;
    if (st && (!st->perturbed || st->question_offset < 0 || (st->trace_perturbed != nullptr) != (traced == 3))) return PNMN_EINVAL;
    if (hidden != H || S < 1 || S > MAXS || V < 1 || V > MAXV || T > MAXT) return PNMN_EINVAL;
    // every index the kernel looks a table row up by, or writes as a token, is inside the vocabulary
    if (start_index < 0 || start_index >= V || end_index < 0 || end_index >= V) return PNMN_EINVAL;
    if (beam != 1 && beam != 2 && beam != 4 && beam != 8 && beam != 16) return PNMN_EINVAL;
    const BeamArgs plain{etable, enc, mask, h0, w_c, w_hh, w_p, b_p, tokens, scores, trace_tokens, trace_backptr, trace_scores,
                         B, T, S, V, pad_index, unk_index, start_index, end_index};
    if (!token_class && !next_state && !min_left)
        return B == 0 || T == 0 ? 0 : launch_search<false>(beam, plain, st, static_cast<hipStream_t>(stream));
    if (!token_class || !next_state || !min_left) return PNMN_EINVAL;
    if (n_states < 1 || n_states > MAX_STATES || n_classes < 1 || n_classes > MAX_CLASSES) return PNMN_EINVAL;
    // every table entry the kernel indexes with stays inside the tables (min_left is only compared)
    ConstrainedBeamArgs a{};
    for (int v = 0; v < V; ++v) {
        if (token_class[v] >= n_classes) return PNMN_EINVAL;
        a.token_class[v] = token_class[v];
    }
    for (int i = 0; i < n_states * n_classes; ++i) {
        if (next_state[i] >= n_states) return PNMN_EINVAL;
        a.next_state[i] = next_state[i];
    }
    for (int s = 0; s < n_states; ++s) a.min_left[s] = min_left[s];
    if (B == 0 || T == 0) return 0;
    static_cast<BeamArgs&>(a) = plain;
    a.n_classes = n_classes;
    return launch_search<true>(beam, a, st, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" int pnmn_attn_lstm_beam(const float* etable, const float* enc, const float* mask, const float* h0,
                                   const float* w_c, const float* w_hh, const float* w_p, const float* b_p,
                                   int64_t* tokens, float* scores, int32_t* trace_tokens, int32_t* trace_backptr,
                                   float* trace_scores, int B, int T, int S, int V, int hidden, int beam, int pad_index,
                                   int unk_index, int start_index, int end_index, const uint8_t* token_class,
                                   const uint8_t* next_state, const uint8_t* min_left, int n_states, int n_classes,
                                   void* stream) {
    return beam_entry(etable, enc, mask, h0, w_c, w_hh, w_p, b_p, tokens, scores, trace_tokens, trace_backptr, trace_scores, B, T, S,
                      V, hidden, beam, pad_index, unk_index, start_index, end_index, token_class, next_state, min_left, n_states,
                      n_classes, nullptr, stream);
}

extern "C" int pnmn_attn_lstm_beam_stochastic(const float* etable, const float* enc, const float* mask, const float* h0,
                                              const float* w_c, const float* w_hh, const float* w_p, const float* b_p,
                                              int64_t* tokens, float* scores, int32_t* trace_tokens, int32_t* trace_backptr,
                                              float* trace_scores, int B, int T, int S, int V, int hidden, int beam,
                                              int pad_index, int unk_index, int start_index, int end_index,
                                              const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left,
                                              int n_states, int n_classes, float* perturbed, float* trace_perturbed,
                                              uint64_t seed, int64_t question_offset, void* stream) {
    const StochasticPart st{perturbed, trace_perturbed, seed, question_offset};
    return beam_entry(etable, enc, mask, h0, w_c, w_hh, w_p, b_p, tokens, scores, trace_tokens, trace_backptr, trace_scores, B, T, S,
                      V, hidden, beam, pad_index, unk_index, start_index, end_index, token_class, next_state, min_left, n_states,
                      n_classes, &st, stream);
}
