// Free-running samples from the program prior p(z) in one persistent launch (the contract: include/probnmn_hip.h, beside
// pnmn_prior_sample).  Per step a row runs two LSTM layers, the 256 x 256 projection, the tied output layer and the token
// choice, and feeds the token to its next step -- the torch loop this replaces issued about a dozen launches per step.
//
// One workgroup of 512 threads owns 16 rows for all T steps, with the wave / unit / accumulator layout of
// lstm_seq_fwd_kernel (seq2seq.hip): wave w owns hidden units [32w, 32w + 32) of all four gates, so both cell updates are
// lane-local, and c0 / c1 never leave registers.  W_hh0, W_ih1, W_hh1 and W_proj are streamed from L2 in MFMA fragment
// order; layer 1's two products accumulate into the same accumulators (gates_mfma, decoder_stages.h).  W_out ([V][256],
// V <= 128 and no multiple of 16 in general) is read row-major by logits_tile, as the decoders read their W_p.
//
// LDS: h0, h1 and the projection p at the LLD = 260 stride, SINGLE-buffered (3 x 16.25 KiB), the logits (8 KiB), the
// tokens and the staged automaton: 57.5 KiB, inside the 64 KiB static limit.  Double-buffering h0 and h1 beside p and the
// logits would take about 66 KiB and the opt-in of lds_optin.h; a single buffer costs one more barrier per layer and step
// (all waves have read h before any wave overwrites it), which is noise beside the 3.25 MiB of weights a step streams.
//
// Rows are independent: no inter-workgroup hand-off, no counters, no workspace, no need for co-residency -- a batch of
// any size is a plain grid of ceil(B / 16) workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/probnmn_hip.h"
#include "decoder_stages.h"
#include "sampling.h"

namespace {

using pnmn::sigm;
using pnmn::f32x4;
constexpr int H = 256;          // hidden = input size the kernel is built for
constexpr int ROWS = 16;        // batch rows per workgroup
constexpr int LD = H + 4;       // LDS row stride (floats), as LLD of the layer kernels
constexpr int G4 = 4 * H;
constexpr int MAXV = 128;

struct PriorArgs {
    const float* table0;    // [V][4H]  Emb W_ih0^T + b_ih0 + b_hh0
    const float* w_hh0;     // fragment order
    const float* w_ih1;     // fragment order
    const float* w_hh1;     // fragment order
    const float* b1;        // [4H]  b_ih1 + b_hh1
    const float* w_proj;    // fragment order
    const float* w_out;     // [V][H] row major
    int64_t* tokens;        // [B][T]
    float* logprob_vocab;   // [B][T]
    float* logprob_proj;    // [B][T]
    float* proj;            // [B][T][H] or null
    const int64_t* in_tokens;  // mode 0
    long in_stride;
    int B, T, V;
    int mode;               // 0: forced, 1: sample, 2: greedy
    int pad, unk, start;
    uint64_t seed, row_offset;
};
struct ConstrainedPriorArgs : PriorArgs {
    pnmn::TokenAutomaton automaton;
};
template <bool CONSTR>
struct prior_args {
    using type = PriorArgs;
};
template <>
struct prior_args<true> {
    using type = ConstrainedPriorArgs;
};

// the cell of one layer from its gate accumulators: c stays in `creg`, h goes to this layer's LDS rows
__device__ __forceinline__ void cell_update(const f32x4 (&acc)[4][2], float (&creg)[2][4], float (*hl)[LD], int wave, int li, int g) {
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ig = sigm(acc[0][ut][r]), fg = sigm(acc[1][ut][r]);
            const float gg = tanhf(acc[2][ut][r]), og = sigm(acc[3][ut][r]);
            const float c = fg * creg[ut][r] + ig * gg;
            creg[ut][r] = c;
            hl[4 * g + r][32 * wave + 16 * ut + li] = og * tanhf(c);
        }
}

// FILT: mode 1 draws under the filter `f` (sampling.h); its weights take the place of the row's logits in `logl`, which the
// wave has in registers by then.  CONSTR (modes 1 and 2): every choice is made within the automaton's allowed set A_c; a
// row's state and finished flag stay in registers of the wave that owns rows 2 wave, 2 wave + 1.
template <bool FILT, bool CONSTR>
__global__ __launch_bounds__(512) void prior_sample_kernel(const typename prior_args<CONSTR>::type a, const pnmn::SamplingFilter f) {
    __shared__ __attribute__((aligned(16))) float h0l[ROWS][LD];
    __shared__ __attribute__((aligned(16))) float h1l[ROWS][LD];
    __shared__ __attribute__((aligned(16))) float pl[ROWS][LD];
    __shared__ float logl[ROWS][MAXV];
    __shared__ int tokl[ROWS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * ROWS;
    const int T = a.T, V = a.V;

    for (int i = tid; i < ROWS * LD; i += 512) {
        (&h0l[0][0])[i] = 0.f;
        (&h1l[0][0])[i] = 0.f;
    }
    if (tid < ROWS) tokl[tid] = a.start;
    pnmn::AutomatonLds au{};
    int row_state[2] = {0, 0};  // (CONSTR) of rows 2 wave, 2 wave + 1: the start state, not finished
    if constexpr (CONSTR) {
        __shared__ unsigned char autl[pnmn::AUTOMATON_LDS_BYTES];
        au = pnmn::stage_automaton(autl, a.automaton);
    }
    float c0[2][4], c1[2][4];
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int r = 0; r < 4; ++r) c0[ut][r] = c1[ut][r] = 0.f;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        f32x4 acc[4][2];
        // ---------------- layer 0: table0[last] + h0 W_hh0^T ----------------
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* tr = a.table0 + (size_t)tokl[4 * g + r] * G4 + 32 * wave + li;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int ut = 0; ut < 2; ++ut) acc[gate][ut][r] = tr[gate * H + 16 * ut];
        }
#pragma unroll 4
        for (int kb = 0; kb < H / 16; ++kb) {
            const f32x4 ah = *reinterpret_cast<const f32x4*>(&h0l[li][kb * 16 + 4 * g]);
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int ut = 0; ut < 2; ++ut) {
                    const size_t fo = ((size_t)((gate * (H / 16) + 2 * wave + ut) * (H / 16) + kb) * 64 + lane) * 4;
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.w_hh0 + fo);
                    acc[gate][ut] = pnmn::mfma4(ah, b, acc[gate][ut]);
                }
        }
        __syncthreads();  // every wave has read h0 of step t - 1
        cell_update(acc, c0, h0l, wave, li, g);
        __syncthreads();

        // ---------------- layer 1: b1 + h0' W_ih1^T + h1 W_hh1^T ----------------
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int ut = 0; ut < 2; ++ut) {
                const float b = a.b1[gate * H + 32 * wave + 16 * ut + li];
                acc[gate][ut] = f32x4{b, b, b, b};
            }
        pnmn::gates_mfma<H, LD>(acc, h0l, h1l, a.w_ih1, a.w_hh1, wave, lane);
        __syncthreads();  // every wave has read h1 of step t - 1
        cell_update(acc, c1, h1l, wave, li, g);
        __syncthreads();

        // ---------------- projection p = h1' W_proj^T: wave w owns outputs [32w, 32w + 32) ----------------
        {
            f32x4 pacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
            for (int kb = 0; kb < H / 16; ++kb) {
                const f32x4 ah = *reinterpret_cast<const f32x4*>(&h1l[li][kb * 16 + 4 * g]);
#pragma unroll
                for (int ut = 0; ut < 2; ++ut) {
                    const size_t fo = ((size_t)((2 * wave + ut) * (H / 16) + kb) * 64 + lane) * 4;
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.w_proj + fo);
                    pacc[ut] = pnmn::mfma4(ah, b, pacc[ut]);
                }
            }
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = 4 * g + r, n = 32 * wave + 16 * ut + li;
                    pl[rl][n] = pacc[ut][r];
                    if (a.proj && row0 + rl < a.B) a.proj[((size_t)(row0 + rl) * T + t) * H + n] = pacc[ut][r];
                }
        }
        __syncthreads();

        // ---------------- logits z = p W_out^T: 16 rows x 16 vocabulary entries per wave ----------------
        if (16 * wave < V) {
            const int vn = 16 * wave + li;
            const f32x4 lacc = pnmn::logits_tile<H, LD>(pl, a.w_out, V, wave, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) logl[4 * g + r][vn] = vn < V ? lacc[r] : -INFINITY;
        }
        __syncthreads();

        // ---------------- token choice and the two log-probabilities: wave w owns rows 2w, 2w + 1 ----------------
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int rl = 2 * wave + rr;
            const int row = row0 + rl;
            if (row >= a.B) continue;  // wave-uniform
            float v[2], mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                v[k] = lane + 64 * k < V ? logl[rl][lane + 64 * k] : -INFINITY;
                mx = fmaxf(mx, v[k]);
            }
            mx = pnmn::wmax(mx);
            float se = 0.f;
#pragma unroll
            for (int k = 0; k < 2; ++k) se += (lane + 64 * k < V) ? expf(v[k] - mx) : 0.f;
            const float lse = mx + logf(pnmn::wsum(se));
            int choice;
            if (a.mode == 0) {
                const long forced = (long)a.in_tokens[(size_t)row * a.in_stride + t];
                choice = forced < 0 ? 0 : (forced >= V ? V - 1 : (int)forced);  // (it indexes table0 at the next step)
            } else if constexpr (CONSTR) {
                const auto set = pnmn::allowed_lanes(au, row_state[rr], T - 1 - t, V, a.pad, a.unk, a.start);
                choice = pnmn::choose_row_token<FILT>(logl[rl], V, a.mode, a.pad, a.unk, a.start, a.seed,
                                                      a.row_offset + (uint64_t)row, (uint32_t)t, logl[rl], f, set);
                row_state[rr] = pnmn::advance_row_state(au, row_state[rr], choice);
            } else {
                choice = pnmn::choose_row_token<FILT>(logl[rl], V, a.mode, a.pad, a.unk, a.start, a.seed,
                                                      a.row_offset + (uint64_t)row, (uint32_t)t, logl[rl], f);
            }
            choice = __builtin_amdgcn_readfirstlane(choice);
            const float zt = __shfl(choice < 64 ? v[0] : v[1], choice & 63);
            // log_softmax of the 256-wide projection at the token's index (the reference's quirk)
            float pv[4], pm = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pv[k] = pl[rl][lane + 64 * k];
                pm = fmaxf(pm, pv[k]);
            }
            pm = pnmn::wmax(pm);
            float ps = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) ps += expf(pv[k] - pm);
            const float plse = pm + logf(pnmn::wsum(ps));
            if (lane == 0) {
                const size_t o = (size_t)row * T + t;
                tokl[rl] = choice;
                a.tokens[o] = choice;
                a.logprob_vocab[o] = zt - lse;
                a.logprob_proj[o] = pl[rl][choice] - plse;
            }
        }
        __syncthreads();
    }
}

template <bool FILT, bool CONSTR>
void launch(const typename prior_args<CONSTR>::type& a, const pnmn::SamplingFilter& f, void* stream) {
    hipLaunchKernelGGL((prior_sample_kernel<FILT, CONSTR>), dim3((a.B + ROWS - 1) / ROWS), dim3(512), 0,
                       static_cast<hipStream_t>(stream), a, f);
}

}  // namespace

extern "C" {

int pnmn_prior_sample(const float* table0, const float* w_hh0, const float* w_ih1, const float* w_hh1, const float* b1,
                      const float* w_proj, const float* w_out, int64_t* tokens, float* logprob_vocab, float* logprob_proj,
                      float* proj, int B, int T, int V, int hidden, int mode, int pad_index, int unk_index, int start_index,
                      uint64_t seed, uint64_t row_offset, const int64_t* in_tokens, int64_t in_token_stride,
                      const struct pnmn_sampling_filter* filter, int end_index, const uint8_t* token_class,
                      const uint8_t* next_state, const uint8_t* min_left, int n_states, int n_classes, void* stream) {
    if (hidden != H || V < 1 || V > MAXV || T < 1 || B < 0 || mode < 0 || mode > 2) return PNMN_EINVAL;
    if (start_index < 0 || start_index >= V) return PNMN_EINVAL;  // (row of table0 every row reads at step 0)
    if (filter && !pnmn::filter_valid(filter)) return PNMN_EINVAL;
    const bool constrained = token_class || next_state || min_left;
    ConstrainedPriorArgs c{};
    if (constrained)
        if (const int e = pnmn::fill_automaton(c.automaton, token_class, next_state, min_left, n_states, n_classes, mode ? V : 0, T, end_index))
            return e;
    if (B == 0) return 0;
    if (!table0 || !w_hh0 || !w_ih1 || !w_hh1 || !b1 || !w_proj || !w_out || !tokens || !logprob_vocab || !logprob_proj)
        return PNMN_EINVAL;
    if (mode == 0 && !in_tokens) return PNMN_EINVAL;
    static_cast<PriorArgs&>(c) = PriorArgs{table0, w_hh0, w_ih1, w_hh1, b1, w_proj, w_out, tokens, logprob_vocab, logprob_proj, proj,
                                           mode == 0 ? in_tokens : nullptr, (long)in_token_stride, B, T, V, mode, pad_index,
                                           unk_index, start_index, seed, row_offset};
    const bool filtered = filter && mode == 1 && !pnmn::filter_is_identity(*filter);
    const pnmn::SamplingFilter f = filtered ? pnmn::SamplingFilter{filter->temperature, filter->top_k, filter->top_p}
                                            : pnmn::SamplingFilter{1.f, 0, 1.f};
    if (constrained && mode != 0) {
        if (filtered) launch<true, true>(c, f, stream);
        else launch<false, true>(c, f, stream);
    } else {
        if (filtered) launch<true, false>(static_cast<const PriorArgs&>(c), f, stream);
        else launch<false, false>(static_cast<const PriorArgs&>(c), f, stream);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
