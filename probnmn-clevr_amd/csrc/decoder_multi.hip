// Multi-CU attention-LSTM decoder for gfx950: eight workgroups per 16-row tile.
//
// decoder.hip gives one workgroup 16 rows for all steps; a step then costs ~27 us of fp32 MFMA on ONE
// CU plus ~40 us of attention (two rows per wave, encoder rows fetched from L2 twice), while the CUs
// that hold no tile idle -- 8 of 256 busy at 128 rows, 32 at 512.  Here a tile is shared by EIGHT
// workgroups that step in lockstep (cluster.h), member p owning
//     attention   rows 2p, 2p+1 of the tile: their encoder outputs (S x 256 floats each) stay in LDS
//                 for the whole sequence, four waves per row split the source positions
//     gates/cell  hidden units [32p, 32p+32) of all four gates: its slices of W_c and W_hh (2 x 16
//                 fragments = 128 VGPRs per lane) stay in registers for the whole sequence
// and two hand-offs per step: the context rows (all-gather through the saved `ctx` tensor), then the
// new hidden state (all-gather through the saved `hs` tensor) -- both tensors are outputs anyway, so
// the exchange costs no extra traffic.  In sampling mode every member computes the 16 x V logits tile
// from the gathered h_t and draws all 16 tokens itself (the Philox stream is keyed by the global row
// and step), so tokens need no exchange.
//
// Backward: member p owns the same units for the cell backward and produces, from its 128 gate
// columns, 16 x 256 PARTIAL sums of dctx = dgates W_c and dh = dgates W_hh (K split eight ways);
// hand-off A; the row owners add the eight partials of their two rows, run the attention backward
// against the LDS-resident encoder rows and publish the rows' complete dh_{t-1}; hand-off B.
// The encoder-output gradient is NOT accumulated here: the kernel emits dctx [B,T,H] and dscore
// [B,T,S] and the caller forms denc = w^T dctx + dscore^T h_prev as two batched GEMMs over time
// (the one-workgroup kernel's per-step read-modify-write of denc is the largest part of its step).
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/probnmn_hip.h"
#include "cluster.h"
#include "lds_optin.h"
#include "recurrent_tile.h"
#include "sampling.h"

using pnmn::f32x4;

namespace {

using pnmn::sigm;
using pnmn::wmax;
using pnmn::wsum;

constexpr int H = 256;
constexpr int G4 = 4 * H;
constexpr int ROWS = 16;
constexpr int MEMBERS = 8;
constexpr int RW = ROWS / MEMBERS;   // attention rows per member
constexpr int UW = H / MEMBERS;      // hidden units per member
constexpr int GLD = UW + 4;
constexpr int MAXS = 64;
constexpr int MAXV = 128;

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

struct MFwdArgs {
    const float* xe;
    const float* etable;
    const float* enc;
    const float* mask;
    const float* h0;
    const float* w_c;     // fragment-packed [4H/16][H/16][64][4]
    const float* w_hh;
    const float* w_p;     // [V][H] row major
    const float* b_p;
    float* hs;
    float* cs;
    float* act;
    float* ctx;
    float* probs;
    int64_t* tokens;
    const int64_t* in_tokens;  // teacher forcing without xe: step t's input is row in_tokens[row][t] of etable
    long in_stride;
    int* sync;
    int B, T, S, V, tiles;
    int sample;
    int pad, unk, start;
    uint64_t seed, row_offset;
};

// What a launch with its rows grouped by length (ORD) takes besides: an argument of its own, so that every other kernel keeps
// its arguments and its code.
struct OrdArgs {
    const int32_t* order;       // slot -> batch row of the pass, from the launch's first slot on
    const int32_t* tile_steps;  // steps of every tile of the launch
    int Bfull;                  // rows of the whole pass: what an entry of `order` may address
};

// What a free-running launch that stops its tiles (STOP) takes besides: an argument of its own, as OrdArgs is.
struct StopArgs {
    int32_t* steps_out;  // [rows of the launch] steps of every row: 1 + the step of its first `end`, T without one
    int end;
};

constexpr size_t FWD_FIXED_LDS = sizeof(float) * (4 * ROWS * GLD + RW * 4 * H + ROWS * MAXV + RW * MAXS) + sizeof(int) * ROWS;
constexpr size_t FWD_OVERLAP_LDS = sizeof(float) * (ROWS * H + 64);  // (OVERLAP) the staged h_{t-1} tile + a sink for predicated stores

// OVERLAP (the launch picks it when S leaves 16.6 KB of LDS free: S <= 59): the step's matrix work is two products,
// W_hh h_{t-1} and W_c ctx_t, and only the second needs the attention's result.  So h_{t-1} is staged into LDS at the TOP
// of the step and the 64 MFMAs of its product are issued in four groups of 16 inside the attention phase -- beside the
// scores' LDS reads and DPP reductions, the softmax and the context sums, which are latency, not issue slots -- and the
// gates phase behind the context hand-off stages and contracts the context alone: half the matrix time of a step leaves
// its critical path (cycle stamps before: gate MFMAs 42 % of a step, attention 23 %).  Each partial sum keeps its order
// (k-blocks ascending, x y z w); the two compilations still agree to round-off only (DESIGN, "Launches of the multi-CU
// decoder"), so a pass must not change sides between two runs that are compared bit for bit.  Without OVERLAP (S > 59): both
// products behind the hand-off, their A operands double buffered in the 16 KB that `cpart` and `logl` leave idle there.
// SAMPLE: the free-running modes (the kernel picks each step's token); a teacher-forced pass compiles without the token
// phase -- its logits tile, Philox draw and the pointers they keep live are what the register allocator spills.
// FILT (with SAMPLE): mode 1 draws under the filter `f` (sampling.h); the weights take the place of the row's logits in `logl`,
// dead by then.  Every member repeats the choice and gets the same token: it is a pure function of the row and the filter.
// CONSTR (with SAMPLE): every choice is made within the automaton's allowed set A_c (the rule: include/probnmn_hip.h).  The
// tables `aut` are staged once into AUTOMATON_LDS_BYTES of LDS behind everything else of the pass (the launch sizes its LDS,
// and picks OVERLAP, with them counted).  A row's state and finished flag stay in scalar registers of the wave that chooses the
// row's tokens -- wave w of EVERY member for rows 2w, 2w + 1, for all steps: a pure function of the row's own earlier tokens,
// which the members already agree on, so the state needs no hand-off either.
// ORD (teacher forced only): rows grouped by length, as in pnmn_lstm_seq_fwd_ordered.  Slot s of the tile is batch row
// order[16 tile + s] wherever a row of a tensor is addressed -- nothing is permuted in memory, and a row's arithmetic does not
// depend on its slot or its neighbours, so its bits are those of the unordered pass -- and the tile runs tile_steps[tile] steps.
// What a later call reads over all T steps (hs: the logits product; ctx: the cell's input weight gradient) is zero filled from
// there on; cs, act and probs, which only this pass's backward reads (over the same steps), stay unwritten.  Without ORD every
// expression below is the one it was.
// STOP (free running, no filter, no automaton): the tile leaves the step loop behind the step at which its last row has
// chosen `end`.  A row that has chosen `end` chooses `end` from then on (the finished row of the constrained kernels), and its
// steps -- 1 + the step of its first `end`, T without one -- go to steps_out.  Up to and including that step the row's tokens
// and saved tensors are the bits of the kernel without STOP: the Philox counter is (row, step), and a row's arithmetic does
// not depend on its neighbours.  From the tile's last step on its rows hold `end` in tokens and ZEROS in hs, ctx, cs, act
// and probs: hs and ctx feed products over all T (the logits, the cell's input weight gradient); cs, act and probs are what
// a backward with the rows grouped by their steps may read at a step the row's forward tile never ran (its tile there can be
// longer than its tile here) -- every gradient of such a step is 0 x these values, so they must be finite, and with probs = 0
// the softmax backward's renormalisation is 0 / 1e-13.
// WHY THE MEMBERS CANNOT DISAGREE about the step they leave at (one that left early would let the others wait for good):
// the decision is a function of the tile's 16 tokens per step alone.  Every member forms them itself, and forms the SAME
// tokens: each reads the same h_t (complete in memory behind the step's second hand-off), the same w_p and b_p, and runs the
// same instructions of the same code object over them, so the logits tile is bit-identical in all eight; the draw is a pure
// function of those logits and (seed, row, step).  The kernels without STOP rest on the same fact -- a member's gate columns
// take the token's table row, so members that disagreed would already compute a hidden state no single token sequence
// explains.  The finished flags sit in LDS per member, are written in the token phase and read behind the barrier that ends
// it: no exchange between workgroups is added, every member runs the same number of signal / wait pairs, and the counter
// arithmetic of cluster.h holds as it is.
template <bool OVERLAP, bool SAMPLE, bool FILT = false, bool CONSTR = false, bool ORD = false, bool STOP = false>
__device__ __forceinline__ void attn_lstm_fwd_multi_body(const MFwdArgs& a, const int tile, const int part,
                                                         const pnmn::SamplingFilter& f = pnmn::SamplingFilter{1.f, 0, 1.f},
                                                         const pnmn::TokenAutomaton* aut = nullptr,
                                                         const OrdArgs& ord = OrdArgs{nullptr, nullptr, 0},
                                                         const StopArgs& stop = StopArgs{nullptr, 0}) {
    static_assert(SAMPLE || !CONSTR, "the automaton constrains the free-running modes only");
    static_assert(!ORD || !SAMPLE, "a free-running pass knows its lengths only as it runs");
    static_assert(!STOP || (SAMPLE && !FILT && !CONSTR), "only the plain free-running modes stop");
    extern __shared__ __attribute__((aligned(16))) char raw[];
    const int T = a.T, S = a.S;
    float* encl = reinterpret_cast<float*>(raw);                                       // [RW][S][H]
    float (*gl)[ROWS][GLD] = reinterpret_cast<float (*)[ROWS][GLD]>(encl + RW * S * H);  // [4][16][36]
    float (*scl)[MAXS] = reinterpret_cast<float (*)[MAXS]>(&gl[4][0][0]);              // [RW][64]
    int* tokl = reinterpret_cast<int*>(&scl[RW][0]);                                   // [16]
    float (*cpart)[4][H] = reinterpret_cast<float (*)[4][H]>(tokl + ROWS);             // [RW][4][H]
    float (*logl)[MAXV] = reinterpret_cast<float (*)[MAXV]>(&cpart[RW][0][0]);         // [16][128]
    float* hst = &logl[ROWS][0];                                                       // (OVERLAP) [4 parts][16 rows][64]
    float* sink = hst + ROWS * H;                                                      // (OVERLAP) [64]
    int* rowl = reinterpret_cast<int*>(OVERLAP ? sink + 64 : hst);                     // (ORD) [16] batch row of every slot
    int* stepl = rowl;                                                                 // (STOP) [16] steps of every finished row, else 0

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int row0 = tile * ROWS, myrow0 = row0 + RW * part, u0 = UW * part;
    pnmn::Cluster cl;
    cl.start(a.sync + tile * pnmn::CLUSTER_COUNTER_STRIDE, MEMBERS);
    // (ORD) Every member of the tile reads this ONE word, which an earlier kernel on the stream wrote: all eight run the same
    // number of steps, so the same number of signal / wait pairs -- the counter arithmetic of cluster.h holds as it is.
    int steps = T;
    if constexpr (ORD) {
        steps = min(max(ord.tile_steps[tile], 1), T);
        // the tile's row indices, once (a slot past the launch's last repeats it, as the clamped rows below do; an index is
        // held inside the pass whatever the list holds)
        if (tid < ROWS) rowl[tid] = min(max(ord.order[min(row0 + tid, a.B - 1)], 0), ord.Bfull - 1);
        __syncthreads();
        // zero fill of my rows from the tile's last step on: the whole width of hs and ctx
        const int nz = (T - steps) * (H / 4);
        for (int rl = 0; rl < RW; ++rl) {
            if (myrow0 + rl >= a.B) continue;
            const size_t o = ((size_t)rowl[RW * part + rl] * T + steps) * H;
            for (int i = tid; i < nz; i += 512) {
                *reinterpret_cast<f32x4*>(a.hs + o + 4 * (size_t)i) = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(a.ctx + o + 4 * (size_t)i) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    // batch row of slot sl of the tile: of a slot inside the launch / clamped to the launch's last row
    auto grow = [&](const int sl) {
        if constexpr (ORD) return rowl[sl];
        else return row0 + sl;
    };
    auto crow = [&](const int sl) {
        if constexpr (ORD) return rowl[sl];
        else return min(row0 + sl, a.B - 1);
    };
    // ... of this member's attention row rl (the same rows, counted from the member's first: the expressions the kernels without
    // an order always had)
    auto mrow = [&](const int rl) {
        if constexpr (ORD) return rowl[RW * part + rl];
        else return myrow0 + rl;
    };

    for (int i = tid; i < RW * S * (H / 4); i += 512) {
        const int rl = i / (S * (H / 4)), rem = i - rl * S * (H / 4);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (myrow0 + rl < a.B) v = *reinterpret_cast<const f32x4*>(a.enc + (size_t)mrow(rl) * S * H + 4 * rem);
        *reinterpret_cast<f32x4*>(encl + (size_t)rl * S * H + 4 * rem) = v;
    }
    // this wave's gate tile: gate q = wave / 2, units u0 + 16 * (wave % 2) .. + 15
    const int gate = wave >> 1, ub = wave & 1;
    f32x4 wc[H / 16], wh[H / 16];
    {
        const int ntile = gate * (H / 16) + u0 / 16 + ub;
#pragma unroll
        for (int kb = 0; kb < H / 16; ++kb) {
            const size_t fo = ((size_t)(ntile * (H / 16) + kb) * 64 + lane) * 4;
            wc[kb] = *reinterpret_cast<const f32x4*>(a.w_c + fo);
            wh[kb] = *reinterpret_cast<const f32x4*>(a.w_hh + fo);
        }
    }
    if (tid < ROWS) tokl[tid] = a.start;
    if constexpr (STOP) {  // (a slot past the launch's last row counts as finished)
        if (tid < ROWS) stepl[tid] = row0 + tid < a.B ? 0 : T;
    }
    int ran = T;  // (STOP) steps the tile ran
    // source mask of the row this wave attends for (constant over the steps)
    const float row_mask = lane < S ? a.mask[(size_t)(ORD ? mrow(wave >> 2) : min(myrow0 + (wave >> 2), a.B - 1)) * S + lane] : 0.f;
    float creg = 0.f;                       // cell state of (row tid / 32, unit u0 + tid % 32)
    const int arow = min(row0 + li, a.B - 1);  // A-operand row (padding rows read a real row; results dropped)
    // teacher forcing from the table: tokl holds the step's input tokens as in the sampling modes; thread r < 16
    // fetches row r's next one a step ahead
    const int64_t* tf_row = (a.in_tokens && tid < ROWS) ? a.in_tokens + (size_t)crow(tid) * a.in_stride : nullptr;
    if (tf_row) tokl[tid] = (int)tf_row[0];

    // A-operand tiles (16 rows x 256 columns of h_{t-1} or ctx_t) in LDS: four parts of 64 columns, slot s (16 bytes) of
    // row r at slot s ^ r -- the 16 lanes of an MFMA operand read hit 16 bank groups.  A thread stages two pieces of a
    // row, 128 columns apart.
    constexpr int PARTF = ROWS * 64;  // floats of a part
    const int s_row = tid >> 5, s_q = tid & 31;
    const int s_rowc = crow(s_row);
    const int s_off = (s_q >> 4) * PARTF + s_row * 64 + 4 * ((s_q & 15) ^ s_row);
    // the four k-blocks of part p of a staged tile as this lane's MFMA fragments
    auto frags = [&](const float* tile_lds, const int p, f32x4 (&f)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = *reinterpret_cast<const f32x4*>(tile_lds + p * PARTF + li * 64 + 4 * ((4 * j + g) ^ li));
    };
    // 16 MFMAs: part p of a 256-long product into two partial sums (even / odd k-block), k-blocks ascending, x y z w
    auto mfma16 = [&](const f32x4 (&f)[4], const f32x4 (&w)[H / 16], const int p, f32x4& even, f32x4& odd) {
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const int kb = p * 4 + j;
            even = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j].x, w[kb].x, even, 0, 0, 0);
            odd = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j + 1].x, w[kb + 1].x, odd, 0, 0, 0);
            even = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j].y, w[kb].y, even, 0, 0, 0);
            odd = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j + 1].y, w[kb + 1].y, odd, 0, 0, 0);
            even = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j].z, w[kb].z, even, 0, 0, 0);
            odd = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j + 1].z, w[kb + 1].z, odd, 0, 0, 0);
            even = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j].w, w[kb].w, even, 0, 0, 0);
            odd = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j + 1].w, w[kb + 1].w, odd, 0, 0, 0);
        }
    };

    // (OVERLAP) the tile's recurrent vector into LDS: h_0 here, h_t right behind the hand-off that completes it
    auto stage_h = [&](const float* rows, const size_t row_stride) {
        const float* hsrc = rows + (size_t)s_rowc * row_stride + 4 * s_q;
        const f32x4 h_lo = *reinterpret_cast<const f32x4*>(hsrc), h_hi = *reinterpret_cast<const f32x4*>(hsrc + 128);
        *reinterpret_cast<f32x4*>(hst + s_off) = h_lo;
        *reinterpret_cast<f32x4*>(hst + s_off + 2 * PARTF) = h_hi;
    };
    if constexpr (OVERLAP) stage_h(a.h0, H);
    pnmn::AutomatonLds au{};
    int row_state[2] = {0, 0};  // (CONSTR) of rows 2 wave, 2 wave + 1: the start state, not finished
    if constexpr (CONSTR) au = pnmn::stage_automaton(reinterpret_cast<unsigned char*>(OVERLAP ? sink + 64 : hst), *aut);
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        // An opaque zero, added to the row indices below: the per-lane 64-bit addresses of a dozen tensors are then formed
        // where they are used (a few VALU each) instead of being hoisted out of the step loop, where they cost 2 VGPRs
        // each for the whole sequence -- beside the 128 weight registers that is what the allocator spilled.
        int zt = 0;
        asm volatile("" : "+v"(zt));
        f32x4 acc;                                             // the step's input projection rows of this wave's gate tile
        f32x4 ph0 = f32x4{0.f, 0.f, 0.f, 0.f}, ph1 = ph0;      // W_hh h_{t-1}, even / odd k-blocks
        auto load_inputs = [&] {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = 4 * g + r, slot = row0 + rl + zt, row = ORD ? grow(rl) + zt : slot;
                const int n = gate * H + u0 + 16 * ub + li;
                float v = 0.f;
                if (slot < a.B) v = a.xe ? a.xe[((size_t)row * T + t) * G4 + n] : a.etable[(size_t)tokl[rl] * G4 + n];
                acc[r] = v;
            }
        };
        // ---------------- attention for my rows: four waves per row split the source positions ----------------
        {
            const int rl = wave >> 2, q = wave & 3;
            const int slot = myrow0 + rl + zt, row = ORD ? mrow(rl) + zt : slot, rowc = ORD ? row : min(row, a.B - 1);
            f32x4 hv;
            if constexpr (OVERLAP) {
                const int r = RW * part + rl;  // my row within the tile; columns 4 lane .. + 3
                hv = *reinterpret_cast<const f32x4*>(hst + (lane >> 4) * PARTF + r * 64 + 4 * ((lane & 15) ^ r));
            } else {
                const float* hp = t > 0 ? a.hs + ((size_t)rowc * T + (t - 1)) * H : a.h0 + (size_t)rowc * H;
                hv = *reinterpret_cast<const f32x4*>(hp + 4 * lane);
            }
            const float* er = encl + (size_t)rl * S * H + 4 * lane;
            constexpr int NP = 4;  // (more in flight would spill beside the weight registers)
            int k_first = 0;
            if constexpr (OVERLAP) {
                // the first eight positions of this wave as straight-line code (positions past S re-read the last one;
                // their sums go to the sink), 16 MFMAs of W_hh h_{t-1} inside each batch of four
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    f32x4 ev[NP], hf[4];
                    float pk[NP];
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        const int s = q + 4 * (NP * b + k);
                        ev[k] = *reinterpret_cast<const f32x4*>(er + (size_t)(s < S ? s : S - 1) * H);
                    }
                    frags(hst, b, hf);
                    mfma16(hf, wh, b, ph0, ph1);
#pragma unroll
                    for (int k = 0; k < NP; ++k) pk[k] = dot4(ev[k], hv);
#pragma unroll
                    for (int k = 0; k < NP; ++k) pk[k] = wsum(pk[k]);
                    // (branch-free: lane 0 stores a sum that exists into its place, every other lane into the sink --
                    // a conditional store would cut the block the MFMAs are scheduled in)
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        const int s = q + 4 * (NP * b + k);
                        float* dst = (lane == 0 && s < S) ? &scl[rl][s] : sink + lane;
                        *dst = pk[k];
                    }
                }
                k_first = 2 * NP;
            }
            {   // this wave's (remaining) positions q + 4 k: all partial dot products first, then the six-step wave
                // reductions of all of them interleaved (one at a time they are 6 dependent shuffles each)
                for (int k0 = k_first; q + 4 * k0 < S; k0 += NP) {
                    float part[NP];
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        const int s = q + 4 * (k0 + k);
                        part[k] = s < S ? dot4(*reinterpret_cast<const f32x4*>(er + (size_t)s * H), hv) : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < NP; ++k) part[k] = wsum(part[k]);  // (DPP chains: independent, the scheduler interleaves them)
#pragma unroll
                    for (int k = 0; k < NP; ++k)
                        if (lane == 0 && q + 4 * (k0 + k) < S) scl[rl][q + 4 * (k0 + k)] = part[k];
                }
            }
            __syncthreads();
            auto softmax = [&] {
                const float m = row_mask;
                const float v = (lane < S ? scl[rl][lane] : 0.f) * m;  // allennlp masked_softmax: softmax(vector * mask) ...
                const float mx = wmax(lane < S ? v : -INFINITY);
                const float ex = lane < S ? expf(v - mx) : 0.f;
                const float p = ex / wsum(ex);
                const float qv = p * m;                                 // ... * mask, renormalised with 1e-13
                const float wgt = qv / (wsum(qv) + 1e-13f);
                if (lane < S) {
                    scl[rl][lane] = wgt;
                    if (slot < a.B) a.probs[((size_t)row * T + t) * S + lane] = p;
                }
            };
            if constexpr (OVERLAP) {
                f32x4 hf[4];
                frags(hst, 2, hf);
                if (q == 0) {  // (the MFMAs in both branches: beside the softmax's chain of reductions where there is one)
                    mfma16(hf, wh, 2, ph0, ph1);
                    softmax();
                } else {
                    mfma16(hf, wh, 2, ph0, ph1);
                }
            } else {
                if (q == 0) softmax();
            }
            __syncthreads();
            f32x4 c4 = f32x4{0.f, 0.f, 0.f, 0.f};
            int s_first = q;
            if constexpr (OVERLAP) {
                // the first four positions straight-line (weight 0 past S), the last 16 MFMAs among them
                constexpr int NC = 4;
                f32x4 ev[NC], hf[4];
                float wv[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int s = q + 4 * k, sc = s < S ? s : S - 1;
                    ev[k] = *reinterpret_cast<const f32x4*>(er + (size_t)sc * H);
                    const float w = scl[rl][sc];
                    wv[k] = s < S ? w : 0.f;
                }
                frags(hst, 3, hf);
                mfma16(hf, wh, 3, ph0, ph1);
#pragma unroll
                for (int k = 0; k < NC; ++k) c4 += ev[k] * wv[k];
                s_first = q + 4 * NC;
            }
            for (int s = s_first; s < S; s += 4) c4 += *reinterpret_cast<const f32x4*>(er + (size_t)s * H) * scl[rl][s];
            *reinterpret_cast<f32x4*>(&cpart[rl][q][4 * lane]) = c4;
            __syncthreads();
            const int rl2 = tid >> 8, k = tid & 255;
            const float cv = (cpart[rl2][0][k] + cpart[rl2][1][k]) + (cpart[rl2][2][k] + cpart[rl2][3][k]);
            if (myrow0 + rl2 < a.B) a.ctx[((size_t)(mrow(rl2) + zt) * T + t) * H + k] = cv;
        }
        cl.signal();
        cl.wait();

        // ---------------- gates of my units on the matrix cores ----------------
        const int tf_next = tf_row ? (int)tf_row[min(t + 1, T - 1)] : 0;  // (stored into tokl behind the cell phase)
        if constexpr (OVERLAP) {
            // the context tile through LDS (into the 16 KB of `cpart` + `logl`, idle here), then its 64 MFMAs
            float* cst = &cpart[0][0][0];
            const float* csrc = a.ctx + ((size_t)(s_rowc + zt) * T + t) * H + 4 * s_q;
            const f32x4 c_lo = *reinterpret_cast<const f32x4*>(csrc), c_hi = *reinterpret_cast<const f32x4*>(csrc + 128);
            load_inputs();  // (requested with the context: kept live across the attention they cost spills)
            *reinterpret_cast<f32x4*>(cst + s_off) = c_lo;
            *reinterpret_cast<f32x4*>(cst + s_off + 2 * PARTF) = c_hi;
            __syncthreads();
            f32x4 pc0 = f32x4{0.f, 0.f, 0.f, 0.f}, pc1 = pc0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f32x4 cf[4];
                frags(cst, p, cf);
                mfma16(cf, wc, p, pc0, pc1);
            }
            acc += (pc0 + pc1) + (ph0 + ph1);
        } else {
            load_inputs();
            // A operands (the tile's 16 x 256 context and hidden vectors) go through LDS in four parts of 64
            // columns, double buffered in the 16 KB that the attention phase's partial contexts and the token phase's
            // logits leave idle here: part p + 1 requested while part p's MFMAs run (holding all four in registers
            // instead spills -- kernels with scratch memory were seen to cost the HOST milliseconds per step once a
            // second stream runs beside them).  This wave owns ONE output tile, so a single accumulator would make its
            // 128 MFMAs one dependent chain: four partial sums -- context / hidden state, even / odd k-block -- keep
            // four chains in flight.
            constexpr int NB = 4, NPARTS = (H / 16) / NB, PART = 2 * ROWS * 64;
            float* stage = &cpart[0][0][0];  // [2 buffers][2 tensors][16 rows][64]
            const int s_tensor = tid >> 8, o_row = (tid >> 4) & 15, o_slot = tid & 15;
            const int o_rowc = crow(o_row);
            const float* s_src = (s_tensor == 0 ? a.ctx + ((size_t)o_rowc * T + t) * H
                                                : (t > 0 ? a.hs + ((size_t)o_rowc * T + (t - 1)) * H : a.h0 + (size_t)o_rowc * H)) + 4 * o_slot;
            float* s_dst = stage + (s_tensor * ROWS + o_row) * 64 + 4 * (o_slot ^ o_row);
            f32x4 sv = *reinterpret_cast<const f32x4*>(s_src);
            *reinterpret_cast<f32x4*>(s_dst) = sv;
            __syncthreads();
            f32x4 pc0 = f32x4{0.f, 0.f, 0.f, 0.f}, pc1 = pc0;
#pragma unroll
            for (int p = 0; p < NPARTS; ++p) {
                if (p + 1 < NPARTS) sv = *reinterpret_cast<const f32x4*>(s_src + (p + 1) * 64);
                const float* buf = stage + (p & 1) * PART;
                f32x4 ac[NB], ah[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int slot = (4 * j + g) ^ li;
                    ac[j] = *reinterpret_cast<const f32x4*>(buf + li * 64 + 4 * slot);
                    ah[j] = *reinterpret_cast<const f32x4*>(buf + (ROWS + li) * 64 + 4 * slot);
                }
                mfma16(ac, wc, p, pc0, pc1);
                mfma16(ah, wh, p, ph0, ph1);
                if (p + 1 < NPARTS) {
                    *reinterpret_cast<f32x4*>(s_dst + ((p + 1) & 1) * PART) = sv;
                    __syncthreads();
                }
            }
            acc += (pc0 + pc1) + (ph0 + ph1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) gl[gate][4 * g + r][16 * ub + li] = acc[r];
        __syncthreads();
        // ---------------- cell: thread -> (row, unit) ----------------
        {
            const int rl = tid >> 5, ul = tid & 31;
            const int slot = row0 + rl + zt, row = ORD ? grow(rl) + zt : slot, u = u0 + ul;
            const float ig = sigm(gl[0][rl][ul]), fg = sigm(gl[1][rl][ul]);
            const float gg = tanhf(gl[2][rl][ul]), og = sigm(gl[3][rl][ul]);
            const float c = fg * creg + ig * gg;
            const float h = og * tanhf(c);
            creg = c;
            if (slot < a.B) {
                const size_t o = ((size_t)row * T + t) * H + u;
                a.hs[o] = h;
                a.cs[o] = c;
                float* ar = a.act + ((size_t)row * T + t) * G4;
                ar[u] = ig;
                ar[H + u] = fg;
                ar[2 * H + u] = gg;
                ar[3 * H + u] = og;
            }
        }
        if (tf_row) tokl[tid] = tf_next;       // (read again behind the hand-off's barriers)
        if (t + 1 == steps && !SAMPLE) break;  // nobody needs the last h
        cl.signal();
        cl.wait();
        if constexpr (OVERLAP) {  // h_t of the whole tile: the next step's attention and W_hh product, the logits below
            stage_h(a.hs + ((size_t)zt * T + t) * H, (size_t)T * H);
            __syncthreads();
        }

        // ---------------- token choice for the next step (every member, all 16 rows) ----------------
        if constexpr (SAMPLE) {
            const int V = a.V;
            if (16 * wave < V) {
                f32x4 lacc = f32x4{0.f, 0.f, 0.f, 0.f}, lodd = lacc;
                const int vn = 16 * wave + li;
                const bool vok = vn < V;
                const float* hp = a.hs + ((size_t)arow * T + t) * H + 4 * g;
                constexpr int NB = 4;
#pragma unroll
                for (int part = 0; part < (H / 16) / NB; ++part) {
                    f32x4 ah[NB], bp[NB];
                    if constexpr (OVERLAP) frags(hst, part, ah);
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const int kb = part * NB + j;
                        if constexpr (!OVERLAP) ah[j] = *reinterpret_cast<const f32x4*>(hp + kb * 16);
                        bp[j] = vok ? *reinterpret_cast<const f32x4*>(a.w_p + (size_t)vn * H + kb * 16 + 4 * g)
                                    : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int j = 0; j < NB; j += 2) {  // two independent chains (even / odd k-block)
                        lacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j].x, bp[j].x, lacc, 0, 0, 0);
                        lodd = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j + 1].x, bp[j + 1].x, lodd, 0, 0, 0);
                        lacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j].y, bp[j].y, lacc, 0, 0, 0);
                        lodd = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j + 1].y, bp[j + 1].y, lodd, 0, 0, 0);
                        lacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j].z, bp[j].z, lacc, 0, 0, 0);
                        lodd = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j + 1].z, bp[j + 1].z, lodd, 0, 0, 0);
                        lacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j].w, bp[j].w, lacc, 0, 0, 0);
                        lodd = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j + 1].w, bp[j + 1].w, lodd, 0, 0, 0);
                    }
                }
                lacc += lodd;
                const float bias = vok ? a.b_p[vn] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) logl[4 * g + r][vn < MAXV ? vn : 0] = vok ? lacc[r] + bias : -INFINITY;
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int rl = 2 * wave + rr;
                const int row = row0 + rl;
                if (row >= a.B) continue;
                int choice;
                if constexpr (CONSTR) {
                    const auto set = pnmn::allowed_lanes(au, row_state[rr], T - 1 - t, V, a.pad, a.unk, a.start);
                    choice = pnmn::choose_row_token<FILT>(logl[rl], V, a.sample, a.pad, a.unk, a.start, a.seed,
                                                          a.row_offset + (uint64_t)row, (uint32_t)t, logl[rl], f, set);
                    row_state[rr] = pnmn::advance_row_state(au, row_state[rr], choice);
                } else {
                    choice = pnmn::choose_row_token<FILT>(logl[rl], V, a.sample, a.pad, a.unk, a.start, a.seed,
                                                          a.row_offset + (uint64_t)row, (uint32_t)t, logl[rl], f);
                }
                if constexpr (STOP) {  // (only this wave touches the row's flag inside the phase)
                    if (stepl[rl] != 0) choice = stop.end;
                    else if (choice == stop.end && lane == 0) stepl[rl] = t + 1;
                }
                if (lane == 0) {
                    tokl[rl] = choice;
                    if (part == 0) a.tokens[(size_t)row * T + t] = choice;
                }
            }
            __syncthreads();
            if constexpr (STOP) {  // every row of the tile has ended: the same answer in every thread of every member (above)
                int unfinished = 0;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) unfinished += stepl[r] == 0;
                if (unfinished == 0) {
                    ran = t + 1;
                    break;
                }
            }
        }
    }
    if constexpr (STOP) {
        // my rows from the tile's last step on: zeros in the saved tensors, `end` in the tokens; and their steps
        const int nz = T - ran;
        for (int rl = 0; rl < RW; ++rl) {
            const int row = myrow0 + rl;
            if (row >= a.B) continue;
            const size_t o = (size_t)row * T + ran;
            const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < nz * (H / 4); i += 512) {
                *reinterpret_cast<f32x4*>(a.hs + o * H + 4 * (size_t)i) = z4;
                *reinterpret_cast<f32x4*>(a.cs + o * H + 4 * (size_t)i) = z4;
                *reinterpret_cast<f32x4*>(a.ctx + o * H + 4 * (size_t)i) = z4;
            }
            for (int i = tid; i < nz * (G4 / 4); i += 512) *reinterpret_cast<f32x4*>(a.act + o * G4 + 4 * (size_t)i) = z4;
            for (int i = tid; i < nz * S; i += 512) a.probs[o * S + i] = 0.f;
            for (int i = tid; i < nz; i += 512) a.tokens[o + i] = stop.end;
            if (tid == 0) {
                const int st = stepl[RW * part + rl];
                stop.steps_out[row] = st != 0 ? st : T;
            }
        }
    }
    cl.finish();
}

template <bool OVERLAP, bool SAMPLE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_multi_kernel(const MFwdArgs a) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_fwd_multi_body<OVERLAP, SAMPLE>(a, tile, part);
}

// A teacher-forced pass with its rows grouped by length (ORD): a kernel of its own, so that the others keep their code.
template <bool OVERLAP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_multi_ordered_kernel(const MFwdArgs a,
                                                                                                                    const OrdArgs ord) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_fwd_multi_body<OVERLAP, false, false, false, true>(a, tile, part, pnmn::SamplingFilter{1.f, 0, 1.f}, nullptr, ord);
}

// A free-running pass whose tiles stop at their last row's `end` (STOP): a kernel of its own, so that the others keep their code.
template <bool OVERLAP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_multi_stop_kernel(const MFwdArgs a,
                                                                                                                 const StopArgs stop) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_fwd_multi_body<OVERLAP, true, false, false, false, true>(a, tile, part, pnmn::SamplingFilter{1.f, 0, 1.f}, nullptr,
                                                                       OrdArgs{nullptr, nullptr, 0}, stop);
}

// TWO independent decoder passes in one launch (the reconstructor's teacher-forced decode and the generator's
// supervised decode of a training iteration: different weights, step counts, source lengths): tiles [0, tiles0) run
// pass a0, the tiles behind them pass a1.  These kernels are bound by their per-step hand-off latency, not by the
// chip: at 128 questions per GPU a pass occupies 32-64 of the 256 CUs for 0.3-0.5 ms, and back to back the passes ADD
// their step counts on the iteration's critical chain; side by side the launch takes as long as the longer one.
// (Two launches on two streams would do the same but put two kernels that wait for their own workgroups on the chip
// next to a third -- DESIGN 6; one grid is resident as a whole or not at all.)
template <bool OVERLAP, bool SAMPLE0, bool SAMPLE1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_pair_kernel(const MFwdArgs a0,
                                                                                                           const MFwdArgs a1,
                                                                                                           const int tiles0) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile < tiles0) {
        if (tile >= a0.tiles) return;
        attn_lstm_fwd_multi_body<OVERLAP, SAMPLE0>(a0, tile, part);
    } else {
        tile -= tiles0;
        if (tile >= a1.tiles) return;
        attn_lstm_fwd_multi_body<OVERLAP, SAMPLE1>(a1, tile, part);
    }
}

// The same two kernels with a sampling filter per free-running pass.  M: 0 teacher forced, 1 free running, 2 sampling under
// its filter.  Kernels of their own, so that the unfiltered ones keep their arguments and their code.
template <bool OVERLAP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_multi_filtered_kernel(
    const MFwdArgs a, const pnmn::SamplingFilter f) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_fwd_multi_body<OVERLAP, true, true>(a, tile, part, f);
}

template <bool OVERLAP, int M0, int M1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_pair_filtered_kernel(
    const MFwdArgs a0, const MFwdArgs a1, const int tiles0, const pnmn::SamplingFilter f0, const pnmn::SamplingFilter f1) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile < tiles0) {
        if (tile >= a0.tiles) return;
        attn_lstm_fwd_multi_body<OVERLAP, M0 != 0, M0 == 2>(a0, tile, part, f0);
    } else {
        tile -= tiles0;
        if (tile >= a1.tiles) return;
        attn_lstm_fwd_multi_body<OVERLAP, M1 != 0, M1 == 2>(a1, tile, part, f1);
    }
}

// ... and under a token automaton (the tables of pnmn_attn_lstm_fwd_group): every free-running pass of the launch is constrained
// by the one automaton `au`.  M: 0 teacher forced, 1 constrained (sampling under the identity filter, or greedy), 2 constrained
// sampling under its filter.  The pair is instantiated for M0 <= M1 only: the host puts the passes in that order.
template <bool OVERLAP, bool FILT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_multi_constrained_kernel(
    const MFwdArgs a, const pnmn::SamplingFilter f, const pnmn::TokenAutomaton au) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_fwd_multi_body<OVERLAP, true, FILT, true>(a, tile, part, f, &au);
}

template <bool OVERLAP, int M0, int M1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_fwd_pair_constrained_kernel(
    const MFwdArgs a0, const MFwdArgs a1, const int tiles0, const pnmn::SamplingFilter f0, const pnmn::SamplingFilter f1,
    const pnmn::TokenAutomaton au) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile < tiles0) {
        if (tile >= a0.tiles) return;
        attn_lstm_fwd_multi_body<OVERLAP, M0 != 0, M0 == 2, M0 != 0>(a0, tile, part, f0, &au);
    } else {
        tile -= tiles0;
        if (tile >= a1.tiles) return;
        attn_lstm_fwd_multi_body<OVERLAP, M1 != 0, M1 == 2, M1 != 0>(a1, tile, part, f1, &au);
    }
}

struct MBwdArgs {
    const float* dhs;
    const float* act;
    const float* cs;
    const float* hs;
    const float* probs;
    const float* enc;
    const float* mask;
    const float* h0;
    const float* w_c_t;   // fragment-packed [H/16][4H/16][64][4]
    const float* w_hh_t;
    float* dgates;        // [B][T][4H]
    float* dctx;          // [B][T][H]
    float* dscore;        // [B][T][S]
    float* weights;       // [B][T][S]  masked, renormalised attention weights w (what the caller's dctx GEMM needs)
    float* dh0;           // [B][H]
    float* x1;            // [tiles][2][MEMBERS][2][16][H]   partial dctx / dh of every member
    float* x2;            // [tiles][2][16][H]               complete dh_{t-1} rows
    int* sync;
    int B, T, S, tiles;
};

constexpr int DLD = 4 * UW + 4;
constexpr size_t BWD_FIXED_LDS = sizeof(float) * (ROWS * DLD + 2 * RW * H + 2 * RW * MAXS + RW * 4 * H + 64);  // (+ a sink for predicated stores)
constexpr size_t ORDER_LDS = sizeof(int) * ROWS;  // (ORD, either direction) the tile's row indices, behind everything else

// ORD: the pass's rows grouped by length, as in the forward kernel: slot -> order[16 tile + slot] wherever a row of a tensor is
// addressed (the exchange buffers x1 / x2 are the TILE's: they stay indexed by slot), and the tile runs the steps
// tile_steps[tile] - 1 .. 0 from zero d h / d c carried in.  Contract, as for the LSTM layers: dhs[b][t] is not read for
// t >= tile_steps, and is exactly zero for t >= the row's own steps (the loss backward sees to that) -- so the skipped steps
// are the ones whose every gradient is an exact zero, and what the steps that run compute is what they computed.  The
// outputs that later calls read over all T (dgates, dctx, dscore, weights) are zero filled from tile_steps on.
template <bool ORD = false>
__device__ __forceinline__ void attn_lstm_bwd_multi_body(const MBwdArgs& a, const int tile, const int part,
                                                         const OrdArgs& ord = OrdArgs{nullptr, nullptr, 0}) {
    extern __shared__ __attribute__((aligned(16))) char raw[];
    const int T = a.T, S = a.S;
    float* encl = reinterpret_cast<float*>(raw);                                        // [RW][S][H]
    float (*dgl)[DLD] = reinterpret_cast<float (*)[DLD]>(encl + RW * S * H);             // [16][132]
    float (*dctxl)[H] = reinterpret_cast<float (*)[H]>(&dgl[ROWS][0]);                   // [RW][H]
    float (*dhl)[H] = dctxl + RW;                                                        // [RW][H] (unused since round 5)
    float (*dwl)[MAXS] = reinterpret_cast<float (*)[MAXS]>(&dhl[RW][0]);                 // [RW][64] d weights -> d scores
    float (*dhpart)[4][H] = reinterpret_cast<float (*)[4][H]>(&dwl[2 * RW][0]);          // [RW][4][H]
    float* sink = &dhpart[RW][0][0];                                                     // [64]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int row0 = tile * ROWS, myrow0 = row0 + RW * part, u0 = UW * part;
    pnmn::Cluster cl;
    cl.start(a.sync + tile * pnmn::CLUSTER_COUNTER_STRIDE, MEMBERS);
    float* x1t = a.x1 + (size_t)tile * 2 * MEMBERS * 2 * ROWS * H;
    float* x2t = a.x2 + (size_t)tile * 2 * ROWS * H;
    int* rowl = reinterpret_cast<int*>(sink + 64);                                       // (ORD) [16] batch row of every slot
    // (ORD) Every member of the tile reads this ONE word, which an earlier kernel on the stream wrote: all eight run the same
    // number of steps, so the same number of signal / wait pairs -- the counter arithmetic of cluster.h holds as it is.
    int steps = T;
    if constexpr (ORD) {
        steps = min(max(ord.tile_steps[tile], 1), T);
        if (tid < ROWS) rowl[tid] = min(max(ord.order[min(row0 + tid, a.B - 1)], 0), ord.Bfull - 1);
        __syncthreads();
        // zero fill of my rows from the tile's last step on
        for (int rl = 0; rl < RW; ++rl) {
            if (myrow0 + rl >= a.B) continue;
            const size_t o = (size_t)rowl[RW * part + rl] * T + steps;  // (row, step) the zeros begin at
            for (int i = tid; i < (T - steps) * (G4 / 4); i += 512)
                *reinterpret_cast<f32x4*>(a.dgates + o * G4 + 4 * (size_t)i) = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < (T - steps) * (H / 4); i += 512)
                *reinterpret_cast<f32x4*>(a.dctx + o * H + 4 * (size_t)i) = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < (T - steps) * S; i += 512) a.dscore[o * S + i] = 0.f, a.weights[o * S + i] = 0.f;
        }
    }
    auto grow = [&](const int sl) {  // batch row of slot sl of the tile: of a slot inside the launch ...
        if constexpr (ORD) return rowl[sl];
        else return row0 + sl;
    };
    auto crow = [&](const int sl) {  // ... / clamped to the launch's last row
        if constexpr (ORD) return rowl[sl];
        else return min(row0 + sl, a.B - 1);
    };

    for (int i = tid; i < RW * S * (H / 4); i += 512) {
        const int rl = i / (S * (H / 4)), rem = i - rl * S * (H / 4);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (myrow0 + rl < a.B) v = *reinterpret_cast<const f32x4*>(a.enc + (size_t)grow(RW * part + rl) * S * H + 4 * rem);
        *reinterpret_cast<f32x4*>(encl + (size_t)rl * S * H + 4 * rem) = v;
    }
    // this wave's output tiles (units 32 * wave .. + 31 of all 256) x my 128 gate columns, both matrices
    constexpr int KB = 4 * UW / 16;  // 8
    f32x4 wc[2][KB], wh[2][KB];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int kl = 0; kl < KB; ++kl) {
            const int q = kl / (UW / 16), jj = kl % (UW / 16);
            const int kb = (q * H + u0) / 16 + jj;
            const size_t fo = ((size_t)((2 * wave + nt) * (G4 / 16) + kb) * 64 + lane) * 4;
            wc[nt][kl] = *reinterpret_cast<const f32x4*>(a.w_c_t + fo);
            wh[nt][kl] = *reinterpret_cast<const f32x4*>(a.w_hh_t + fo);
        }
    float dc_rec = 0.f;
    const float row_mask = lane < S ? a.mask[(size_t)crow(RW * part + (wave >> 2)) * S + lane] : 0.f;
    __syncthreads();

    // What a step reads of the forward pass (activated gates, cell states, the incoming d h, the attention
    // probabilities) does not depend on the recurrence: step t - 1's values are requested before the last
    // hand-off of step t and arrive while it completes, instead of costing an HBM round trip at the top of
    // every step.
    struct Saved {
        float ig, fg, gg, og, c, cp, dhs, p;
    };
    const int c_rl = tid >> 5, c_ul = tid & 31;
    const int c_slot = row0 + c_rl, c_row = grow(c_rl), c_u = u0 + c_ul;
    const int p_row = crow(RW * part + (wave >> 2));
    auto load_saved = [&](int t) {
        Saved v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (c_slot < a.B) {
            const size_t o = ((size_t)c_row * T + t) * H + c_u;
            const float* ar = a.act + ((size_t)c_row * T + t) * G4;
            v.ig = ar[c_u], v.fg = ar[H + c_u], v.gg = ar[2 * H + c_u], v.og = ar[3 * H + c_u];
            v.c = a.cs[o];
            v.cp = t > 0 ? a.cs[o - H] : 0.f;
            v.dhs = a.dhs[o];
        }
        if ((wave & 3) == 0 && lane < S) v.p = a.probs[((size_t)p_row * T + t) * S + lane];
        return v;
    };
    Saved sv = load_saved(steps - 1);

    // this wave's A fragments of the step's gate gradients (16 rows x my 128 gate columns, K block kl)
    auto dg_frag = [&](const int kl) { return *reinterpret_cast<const f32x4*>(&dgl[li][kl * 16 + 4 * g]); };
    // 16 MFMAs of one product (weights as the A operand: the product comes out transposed, each lane holding FOUR
    // CONSECUTIVE UNITS of one row -- one 16-byte store per tile instead of four 4-byte ones): K blocks kl0, kl0 + 1 of both
    // output tiles; every accumulator sees its K blocks ascending, x y z w
    auto mfma16 = [&](const f32x4 (&w)[2][KB], const int kl0, f32x4 (&acc)[2]) {
#pragma unroll
        for (int kl = kl0; kl < kl0 + 2; ++kl) {
            const f32x4 av = dg_frag(kl);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[nt] = pnmn::mfma4(w[nt][kl], av, acc[nt]);
        }
    };

    // The two products of a step's gate gradients are not equally urgent: the partial dctx = dgates W_c is what the
    // attention backward waits for (hand-off A), the partial dh = dgates W_hh only enters dh_{t-1}, which nobody reads
    // before the NEXT step's cell backward.  So only the dctx product runs in front of hand-off A; the 64 MFMAs of the dh
    // product are issued inside the attention backward (its scores, softmax backward and d h sums are latency, not issue
    // slots -- as in the forward kernel), every member publishes its partial with hand-off B, and the next step's cell
    // backward adds the eight partials (same order as the row owners added them before) to the row owner's attention part.
    for (int t = steps - 1; t >= 0; --t) {
        const Saved cur = sv;
        int zt = 0;  // (an opaque zero in the row indices: addresses formed where they are used, see the forward kernel)
        asm volatile("" : "+v"(zt));
        // ---------------- cell backward of my units: thread -> (row, unit) ----------------
        {
            const int rl = c_rl, ul = c_ul;
            const int row = c_row + zt, u = c_u;
            float di = 0.f, df = 0.f, dg = 0.f, dout = 0.f, dcp = 0.f;
            if (c_slot + zt < a.B) {
                const float ig = cur.ig, fg = cur.fg, gg = cur.gg, og = cur.og;
                const float c = cur.c;
                const float cp = cur.cp;
                const float tc = tanhf(c);
                float dhp = 0.f;
                if (t < steps - 1) {
                    // d h_t from step t + 1: the members' partial products, then the row owner's attention part
                    const float* ph = x1t + (((size_t)((t + 1) & 1) * MEMBERS) * 2 + 1) * ROWS * H + (size_t)(rl + zt) * H + u;
                    float pv[MEMBERS];
#pragma unroll
                    for (int m = 0; m < MEMBERS; ++m) pv[m] = ph[(size_t)(2 * m) * ROWS * H];
                    const float att = x2t[((size_t)((t + 1) & 1) * ROWS + rl) * H + u];
                    float sh = 0.f;
#pragma unroll
                    for (int m = 0; m < MEMBERS; ++m) sh += pv[m];
                    dhp = sh + att;
                }
                const float dh = cur.dhs + dhp;
                const float dc = dc_rec + dh * og * (1.f - tc * tc);
                di = dc * gg * ig * (1.f - ig);
                df = dc * cp * fg * (1.f - fg);
                dg = dc * ig * (1.f - gg * gg);
                dout = dh * tc * og * (1.f - og);
                dcp = dc * fg;
                float* dr = a.dgates + ((size_t)row * T + t) * G4;
                dr[u] = di;
                dr[H + u] = df;
                dr[2 * H + u] = dg;
                dr[3 * H + u] = dout;
            }
            dc_rec = dcp;
            dgl[rl][ul] = di;
            dgl[rl][UW + ul] = df;
            dgl[rl][2 * UW + ul] = dg;
            dgl[rl][3 * UW + ul] = dout;
        }
        __syncthreads();
        // ---------------- partial dctx from my gate columns ----------------
        float* const pc = x1t + (((size_t)(t & 1) * MEMBERS + part) * 2 + 0) * ROWS * H;
        float* const ph = pc + ROWS * H;
        {
            f32x4 accc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int kl = 0; kl < KB; kl += 2) mfma16(wc, kl, accc);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const size_t o = (size_t)(li + zt) * H + 16 * (2 * wave + nt) + 4 * g;  // row li, units 16 (2 wave + nt) + 4 g ..
                *reinterpret_cast<f32x4*>(pc + o) = accc[nt];
            }
        }
        cl.signal();
        cl.wait();

        // ---------------- my rows: gather the dctx partials, attention backward (+ the dh product) ----------------
        f32x4 acch[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        {
            const int rl2 = tid >> 8, k = tid & 255;
            const float* src = x1t + (size_t)(t & 1) * MEMBERS * 2 * ROWS * H + (size_t)(RW * part + rl2 + zt) * H + k;
            float pv[MEMBERS];
#pragma unroll
            for (int s = 0; s < MEMBERS; ++s) pv[s] = src[(size_t)(2 * s) * ROWS * H];
            float sc = 0.f;
#pragma unroll
            for (int s = 0; s < MEMBERS; ++s) sc += pv[s];
            dctxl[rl2][k] = sc;
            if (myrow0 + rl2 < a.B) a.dctx[((size_t)(grow(RW * part + rl2) + zt) * T + t) * H + k] = sc;
        }
        __syncthreads();
        {
            const int rl = wave >> 2, q = wave & 3;
            const int slot = myrow0 + rl + zt, row = ORD ? grow(RW * part + rl) + zt : slot;
            const float* er = encl + (size_t)rl * S * H + 4 * lane;
            const f32x4 dc4 = *reinterpret_cast<const f32x4*>(&dctxl[rl][4 * lane]);
            constexpr int NP = 4;  // (more in flight would spill beside the weight registers)
            // the first eight positions of this wave as straight-line code (positions past S re-read the last one; their
            // sums go to the sink), 16 MFMAs of the dh product inside each batch of four
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                f32x4 ev[NP];
                float pk[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int s = q + 4 * (NP * b + k);
                    ev[k] = *reinterpret_cast<const f32x4*>(er + (size_t)(s < S ? s : S - 1) * H);
                }
                mfma16(wh, 2 * b, acch);
#pragma unroll
                for (int k = 0; k < NP; ++k) pk[k] = dot4(ev[k], dc4);
#pragma unroll
                for (int k = 0; k < NP; ++k) pk[k] = wsum(pk[k]);
#pragma unroll
                for (int k = 0; k < NP; ++k) {  // (branch-free: lane 0 stores a sum that exists, every other lane into the sink)
                    const int s = q + 4 * (NP * b + k);
                    float* dst = (lane == 0 && s < S) ? &dwl[rl][s] : sink + lane;
                    *dst = pk[k];
                }
            }
            for (int k0 = 2 * NP; q + 4 * k0 < S; k0 += NP) {  // (the remaining positions, S > 32)
                float part[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int s = q + 4 * (k0 + k);
                    part[k] = s < S ? dot4(*reinterpret_cast<const f32x4*>(er + (size_t)s * H), dc4) : 0.f;
                }
#pragma unroll
                for (int k = 0; k < NP; ++k) part[k] = wsum(part[k]);  // (DPP chains: independent, the scheduler interleaves them)
#pragma unroll
                for (int k = 0; k < NP; ++k)
                    if (lane == 0 && q + 4 * (k0 + k) < S) dwl[rl][q + 4 * (k0 + k)] = part[k];
            }
            __syncthreads();
            auto softmax_bwd = [&] {
                // forward quantities of this (row, step): p (softmax before masking), mask, q, Z
                const float m = row_mask;
                const float p = lane < S ? cur.p : 0.f;
                const float qv = p * m;
                const float Z = wsum(qv) + 1e-13f;
                const float dw = lane < S ? dwl[rl][lane] : 0.f;
                // w = q / Z ; q = p * mask ; p = softmax(score * mask)
                const float dq = dw / Z - wsum(dw * qv) / (Z * Z);
                const float dp = dq * m;
                const float dv = p * (dp - wsum(dp * p));
                const float dscore = dv * m;
                if (lane < S) {
                    dwl[rl][lane] = dscore;
                    if (slot < a.B) {
                        a.dscore[((size_t)row * T + t) * S + lane] = dscore;
                        a.weights[((size_t)row * T + t) * S + lane] = qv / Z;
                    }
                }
            };
            if (q == 0) {  // (the MFMAs in both branches: beside the chain of reductions where there is one)
                mfma16(wh, 4, acch);
                softmax_bwd();
            } else {
                mfma16(wh, 4, acch);
            }
            __syncthreads();
            f32x4 dh4 = f32x4{0.f, 0.f, 0.f, 0.f};
            {
                // the first four positions straight-line (weight 0 past S), the last 16 MFMAs among them
                constexpr int NC = 4;
                f32x4 ev[NC];
                float wv[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int s = q + 4 * k, sc = s < S ? s : S - 1;
                    ev[k] = *reinterpret_cast<const f32x4*>(er + (size_t)sc * H);
                    const float w = dwl[rl][sc];
                    wv[k] = s < S ? w : 0.f;
                }
                mfma16(wh, 6, acch);
#pragma unroll
                for (int k = 0; k < NC; ++k) dh4 += ev[k] * wv[k];
            }
            for (int s = q + 16; s < S; s += 4) dh4 += *reinterpret_cast<const f32x4*>(er + (size_t)s * H) * dwl[rl][s];
            *reinterpret_cast<f32x4*>(&dhpart[rl][q][4 * lane]) = dh4;
        }
        // this member's partial dh: published by hand-off B (the final step's: by the one after the loop)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const size_t o = (size_t)(li + zt) * H + 16 * (2 * wave + nt) + 4 * g;
            *reinterpret_cast<f32x4*>(ph + o) = acch[nt];
        }
        __syncthreads();
        {
            // the attention's part of d h_{t-1} for my rows
            const int rl2 = tid >> 8, k = tid & 255;
            const float v = (dhpart[rl2][0][k] + dhpart[rl2][1][k]) + (dhpart[rl2][2][k] + dhpart[rl2][3][k]);
            x2t[((size_t)(t & 1) * ROWS + RW * part + rl2 + zt) * H + k] = v;
        }
        if (t > 0) sv = load_saved(t - 1);
        cl.signal();
        cl.wait();
    }
    {   // d h_0 of my rows: the members' partials of the last step (t = 0), then the attention part (as the cell backward adds them)
        const int rl2 = tid >> 8, k = tid & 255;
        const float* ph0 = x1t + (size_t)1 * ROWS * H + (size_t)(RW * part + rl2) * H + k;  // buffer 0 (t = 0), tensor 1
        float pv[MEMBERS];
#pragma unroll
        for (int m = 0; m < MEMBERS; ++m) pv[m] = ph0[(size_t)(2 * m) * ROWS * H];
        const float att = x2t[((size_t)0 * ROWS + RW * part + rl2) * H + k];
        float sh = 0.f;
#pragma unroll
        for (int m = 0; m < MEMBERS; ++m) sh += pv[m];
        if (myrow0 + rl2 < a.B) a.dh0[(size_t)grow(RW * part + rl2) * H + k] = sh + att;
    }
    cl.finish();
}

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_bwd_multi_kernel(const MBwdArgs a) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_bwd_multi_body(a, tile, part);
}

// a pass with its rows grouped by length (ORD): a kernel of its own, as in the forward direction
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_bwd_multi_ordered_kernel(const MBwdArgs a,
                                                                                                                    const OrdArgs ord) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile >= a.tiles) return;
    attn_lstm_bwd_multi_body<true>(a, tile, part, ord);
}

// the backward passes of two decoders in one launch (see attn_lstm_fwd_pair_kernel)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_bwd_pair_kernel(const MBwdArgs a0,
                                                                                                           const MBwdArgs a1,
                                                                                                           const int tiles0) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile < tiles0) {
        if (tile >= a0.tiles) return;
        attn_lstm_bwd_multi_body(a0, tile, part);
    } else {
        tile -= tiles0;
        if (tile >= a1.tiles) return;
        attn_lstm_bwd_multi_body(a1, tile, part);
    }
}

// ... of THREE (round 5): the generator's two decodes and the reconstructor's.  In the backward pass of a training iteration
// the three are independent (the samples are discrete: nothing flows from the reconstructor into the generator), and on one
// stream they would add their step counts on the iteration's critical chain -- at 128 questions per GPU the seq2seq backward
// is that chain (scripts/step_timeline.py).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_lstm_bwd_group3_kernel(const MBwdArgs a0,
                                                                                                             const MBwdArgs a1,
                                                                                                             const MBwdArgs a2,
                                                                                                             const int tiles0,
                                                                                                             const int tiles01) {
    int tile, part;
    pnmn::cluster_coords<MEMBERS>(tile, part);
    if (tile < tiles0) {
        if (tile >= a0.tiles) return;
        attn_lstm_bwd_multi_body(a0, tile, part);
    } else if (tile < tiles01) {
        tile -= tiles0;
        if (tile >= a1.tiles) return;
        attn_lstm_bwd_multi_body(a1, tile, part);
    } else {
        tile -= tiles01;
        if (tile >= a2.tiles) return;
        attn_lstm_bwd_multi_body(a2, tile, part);
    }
}

// ---- the compiled kernels: every __global__ instantiation of this file, named once -----------------------------------
// A launch finds its kernel by key.  Forward: passes side by side (1 or 2), OVERLAP, the kernel's M of either pass (0 teacher
// forced, 1 free running, 2 sampling under a filter; m1 = 0 for a lone pass), under the automaton, rows grouped by length.
// Backward: the passes (1 to 3) and the order.  `stop`: a lone free-running pass whose tiles stop (last, so that the rows above
// read as they did).  `optin` is the row's own: the kernel's LDS opt-in per device (lds_optin.h).
struct VariantKey {
    int backward, passes, overlap, m0, m1, constrained, ordered, stop;
};
struct Variant {
    VariantKey key;
    const void* kernel;
    std::atomic<uint64_t> optin{0};
};
template <class... Args>
const void* kernel_of(void (*kernel)(Args...)) {
    return reinterpret_cast<const void*>(kernel);
}
Variant VARIANTS[] = {
    // bwd n ov m0 m1 con ord
    {{0, 1, 1, 1, 0, 0, 0}, kernel_of(attn_lstm_fwd_multi_kernel<true, true>)},
    {{0, 1, 1, 0, 0, 0, 0}, kernel_of(attn_lstm_fwd_multi_kernel<true, false>)},
    {{0, 1, 0, 1, 0, 0, 0}, kernel_of(attn_lstm_fwd_multi_kernel<false, true>)},
    {{0, 1, 0, 0, 0, 0, 0}, kernel_of(attn_lstm_fwd_multi_kernel<false, false>)},
    {{0, 2, 1, 1, 1, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<true, true, true>)},
    {{0, 2, 1, 1, 0, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<true, true, false>)},
    {{0, 2, 1, 0, 1, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<true, false, true>)},
    {{0, 2, 1, 0, 0, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<true, false, false>)},
    {{0, 2, 0, 1, 1, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<false, true, true>)},
    {{0, 2, 0, 1, 0, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<false, true, false>)},
    {{0, 2, 0, 0, 1, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<false, false, true>)},
    {{0, 2, 0, 0, 0, 0, 0}, kernel_of(attn_lstm_fwd_pair_kernel<false, false, false>)},
    // with a filter: at least one M is 2
    {{0, 1, 1, 2, 0, 0, 0}, kernel_of(attn_lstm_fwd_multi_filtered_kernel<true>)},
    {{0, 1, 0, 2, 0, 0, 0}, kernel_of(attn_lstm_fwd_multi_filtered_kernel<false>)},
    {{0, 2, 1, 2, 2, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<true, 2, 2>)},
    {{0, 2, 1, 2, 1, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<true, 2, 1>)},
    {{0, 2, 1, 2, 0, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<true, 2, 0>)},
    {{0, 2, 1, 1, 2, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<true, 1, 2>)},
    {{0, 2, 1, 0, 2, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<true, 0, 2>)},
    {{0, 2, 0, 2, 2, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<false, 2, 2>)},
    {{0, 2, 0, 2, 1, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<false, 2, 1>)},
    {{0, 2, 0, 2, 0, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<false, 2, 0>)},
    {{0, 2, 0, 1, 2, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<false, 1, 2>)},
    {{0, 2, 0, 0, 2, 0, 0}, kernel_of(attn_lstm_fwd_pair_filtered_kernel<false, 0, 2>)},
    // under the automaton: at least one M is not 0, and m0 <= m1 in a pair (launch_fwd puts the passes in that order)
    {{0, 1, 1, 2, 0, 1, 0}, kernel_of(attn_lstm_fwd_multi_constrained_kernel<true, true>)},
    {{0, 1, 1, 1, 0, 1, 0}, kernel_of(attn_lstm_fwd_multi_constrained_kernel<true, false>)},
    {{0, 1, 0, 2, 0, 1, 0}, kernel_of(attn_lstm_fwd_multi_constrained_kernel<false, true>)},
    {{0, 1, 0, 1, 0, 1, 0}, kernel_of(attn_lstm_fwd_multi_constrained_kernel<false, false>)},
    {{0, 2, 1, 0, 2, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<true, 0, 2>)},
    {{0, 2, 1, 0, 1, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<true, 0, 1>)},
    {{0, 2, 1, 1, 2, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<true, 1, 2>)},
    {{0, 2, 1, 1, 1, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<true, 1, 1>)},
    {{0, 2, 1, 2, 2, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<true, 2, 2>)},
    {{0, 2, 0, 0, 2, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<false, 0, 2>)},
    {{0, 2, 0, 0, 1, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<false, 0, 1>)},
    {{0, 2, 0, 1, 2, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<false, 1, 2>)},
    {{0, 2, 0, 1, 1, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<false, 1, 1>)},
    {{0, 2, 0, 2, 2, 1, 0}, kernel_of(attn_lstm_fwd_pair_constrained_kernel<false, 2, 2>)},
    // rows grouped by length: a lone teacher-forced pass
    {{0, 1, 1, 0, 0, 0, 1}, kernel_of(attn_lstm_fwd_multi_ordered_kernel<true>)},
    {{0, 1, 0, 0, 0, 0, 1}, kernel_of(attn_lstm_fwd_multi_ordered_kernel<false>)},
    // tiles that stop at their last row's end: a lone free-running pass (bwd n ov m0 m1 con ord stop)
    {{0, 1, 1, 1, 0, 0, 0, 1}, kernel_of(attn_lstm_fwd_multi_stop_kernel<true>)},
    {{0, 1, 0, 1, 0, 0, 0, 1}, kernel_of(attn_lstm_fwd_multi_stop_kernel<false>)},
    // backward
    {{1, 1, 0, 0, 0, 0, 0}, kernel_of(attn_lstm_bwd_multi_kernel)},
    {{1, 1, 0, 0, 0, 0, 1}, kernel_of(attn_lstm_bwd_multi_ordered_kernel)},
    {{1, 2, 0, 0, 0, 0, 0}, kernel_of(attn_lstm_bwd_pair_kernel)},
    {{1, 3, 0, 0, 0, 0, 0}, kernel_of(attn_lstm_bwd_group3_kernel)},
};

// rows one launch can take: all tiles x 8 members resident, one workgroup per CU
int rows_per_launch() {
    const int cus = pnmn::device_cus();
    return cus >= 8 * MEMBERS ? (cus / (8 * MEMBERS)) * 8 * ROWS : 0;
}


// ---- host side: one to three independent passes per launch ---------------------------------------------------------
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int MAX_JOBS = 3;

inline int padded_tiles(int B) { return 8 * ((((B + ROWS - 1) / ROWS) + 7) / 8); }  // (whole groups of 8 tiles)

// all n passes in one launch?  (their tile groups must be resident together)
bool fits(const int* rows, int n) {
    const int chunk = rows_per_launch();
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        if (rows[i] <= 0) return false;
        tiles += padded_tiles(rows[i]);
    }
    return chunk > 0 && tiles * ROWS <= chunk && tiles <= 128;
}
template <class Job>
bool jobs_fit(const Job* j, int n) {
    int rows[MAX_JOBS];
    for (int i = 0; i < n; ++i) {
        if (j[i].T <= 0) return false;
        rows[i] = j[i].B;
    }
    return fits(rows, n);
}

// tiles of exchange buffers behind the counters: a lone pass takes its own tiles (of one row chunk), passes side by
// side whole groups of 8 tiles each
int exchange_tiles(const int* rows, int n, int chunk) {
    if (n == 1) return ((rows[0] < chunk ? rows[0] : chunk) + ROWS - 1) / ROWS;
    int tiles = 0;
    for (int i = 0; i < n; ++i) tiles += padded_tiles(rows[i]);
    return tiles;
}

// passes that do not fit one launch together: the first n - 1 by the same rule, then the last alone
int64_t workspace_bytes(const int* rows, int n, bool backward) {
    if (n > 1 && !fits(rows, n)) {
        const int64_t a = workspace_bytes(rows, n - 1, backward), b = workspace_bytes(rows + n - 1, 1, backward);
        return a > b ? a : b;
    }
    const int chunk = rows_per_launch();
    if (chunk <= 0 || rows[0] <= 0) return 0;
    int64_t bytes = (int64_t)pnmn::CLUSTER_SYNC_BYTES;
    if (backward) bytes += (int64_t)exchange_tiles(rows, n, chunk) * (2 * MEMBERS * 2 + 2) * ROWS * H * sizeof(float);
    return bytes;
}

int check_job(const pnmn_decoder_fwd_job& j, int hidden) {
    if (!j.enc || !j.mask || !j.h0 || !j.w_c || !j.w_hh || !j.hs || !j.cs || !j.act || !j.ctx || !j.probs) return PNMN_EINVAL;
    if (j.sample ? (!j.etable || !j.w_p || !j.b_p || !j.tokens) : (!j.xe && !(j.etable && j.in_tokens))) return PNMN_EINVAL;
    if (hidden != H || j.S < 1 || j.S > MAXS || (j.sample && (j.V < 1 || j.V > MAXV))) return PNMN_ESHAPE;
    return 0;
}
int check_job(const pnmn_decoder_bwd_job& j, int hidden) {
    if (!j.dhs || !j.act || !j.cs || !j.hs || !j.probs || !j.enc || !j.mask || !j.h0 || !j.w_c_t || !j.w_hh_t || !j.dgates ||
        !j.dctx || !j.dscore || !j.weights || !j.dh0)
        return PNMN_EINVAL;
    if (hidden != H || j.S < 1 || j.S > MAXS) return PNMN_ESHAPE;
    return 0;
}

// the kernel's arguments for `rows` rows of a pass from row r on; tile0 = the pass's first tile in the launch (its
// counters and exchange buffers)
MFwdArgs kernel_args(const pnmn_decoder_fwd_job& j, size_t r, int rows, int* sync, int tile0) {
    const int T = j.T, S = j.S;
    return MFwdArgs{j.xe ? j.xe + r * T * G4 : nullptr, j.etable, j.enc + r * S * H, j.mask + r * S, j.h0 + r * H, j.w_c, j.w_hh,
                    j.w_p, j.b_p, j.hs + r * T * H, j.cs + r * T * H, j.act + r * T * G4, j.ctx + r * T * H, j.probs + r * T * S,
                    j.tokens ? j.tokens + r * T : nullptr, (!j.sample && !j.xe) ? j.in_tokens + r * j.in_token_stride : nullptr,
                    (long)j.in_token_stride, sync + tile0 * pnmn::CLUSTER_COUNTER_STRIDE, rows, T, S, j.V, (rows + ROWS - 1) / ROWS,
                    j.sample, j.pad_index, j.unk_index, j.start_index, j.seed, j.row_offset + r};
}
MBwdArgs kernel_args(const pnmn_decoder_bwd_job& j, size_t r, int rows, int* sync, int tile0, float* x1, float* x2) {
    const int T = j.T, S = j.S;
    return MBwdArgs{j.dhs + r * T * H, j.act + r * T * G4, j.cs + r * T * H, j.hs + r * T * H, j.probs + r * T * S,
                    j.enc + r * S * H, j.mask + r * S, j.h0 + r * H, j.w_c_t, j.w_hh_t, j.dgates + r * T * G4, j.dctx + r * T * H,
                    j.dscore + r * T * S, j.weights + r * T * S, j.dh0 + r * H, x1 + (size_t)tile0 * 2 * MEMBERS * 2 * ROWS * H,
                    x2 + (size_t)tile0 * 2 * ROWS * H, sync + tile0 * pnmn::CLUSTER_COUNTER_STRIDE, rows, T, S,
                    (rows + ROWS - 1) / ROWS};
}

// The range of slots from r0 on (a multiple of 16) of a pass whose rows are grouped by length: its part of `order` and
// `tile_steps`; the kernel's other arguments are those of the range's ROWS (kernel_args at r = 0 with the range's row count):
// the pass's own base pointers -- a slot's row may lie anywhere in the pass
OrdArgs ordered_range(size_t r0, int pass_rows, const int32_t* order, const int32_t* tile_steps) {
    return OrdArgs{order + r0, tile_steps + r0 / ROWS, pass_rows};
}

// Orders of a group call: null, or n entries of which entry i (may be null) belongs to job i
inline bool any_order(const int32_t* const* order, int n) {
    for (int i = 0; order && i < n; ++i)
        if (order[i]) return true;
    return false;
}
inline const int32_t* const* from(const int32_t* const* lists, int i) { return lists ? lists + i : nullptr; }

// What a group of passes needs before its launch, the same in both directions: every job checked, the longest source
// (the LDS size follows it), every pass's first tile (tile0[n] = all tiles).
template <class Job>
int plan_group(const Job* j, int n, int hidden, int& smax, int& chunk, int* rows, int* tile0) {
    smax = 0;
    tile0[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (const int e = check_job(j[i], hidden)) return e;
        smax = j[i].S > smax ? j[i].S : smax;
        rows[i] = j[i].B;
        tile0[i + 1] = tile0[i] + padded_tiles(rows[i]);
    }
    chunk = rows_per_launch();
    return chunk > 0 ? 0 : PNMN_ESHAPE;
}

// The table's row of `key`, its kernel opted in to the LDS limit on this device (the limit itself, whatever the launch
// uses).  A key without a row is PNMN_EINVAL: the launchers below form none.
int find_variant(const VariantKey& key, const Variant*& out) {
    for (Variant& v : VARIANTS) {
        const VariantKey& k = v.key;
        if (k.backward == key.backward && k.passes == key.passes && k.overlap == key.overlap && k.m0 == key.m0 && k.m1 == key.m1 &&
            k.constrained == key.constrained && k.ordered == key.ordered && k.stop == key.stop) {
            out = &v;
            return pnmn::opt_in_lds(v.kernel, LDS_LIMIT, v.optin);
        }
    }
    return PNMN_EINVAL;
}

// One launch of a row's kernel over `tiles` tiles.  `args`: the kernel's arguments in the order every signature follows -- the
// pass records; with more than one pass tiles0 (and tiles01); a filter per pass (the filtered and the constrained kernels); the
// automaton (constrained); OrdArgs (ordered); StopArgs (stop) -- each null where the kernel takes none.
int launch(const Variant& v, int tiles, size_t lds, hipStream_t st, std::initializer_list<const void*> args) {
    void* argv[8];
    int n = 0;
    for (const void* a : args)
        if (a) argv[n++] = const_cast<void*>(a);
    (void)hipLaunchKernel(v.kernel, dim3(MEMBERS * tiles), dim3(512), argv, lds, st);
    return (int)hipGetLastError();
}

// A lone pass runs in row ranges of at most `chunk` rows, each a launch behind the stream's counter block: issue(r0, rows, sync)
template <class Issue>
int for_row_ranges(int rows, int chunk, void* workspace, hipStream_t st, Issue issue) {
    int* sync = nullptr;
    for (int r0 = 0; r0 < rows; r0 += chunk) {
        const hipError_t e = pnmn::cluster_sync_block(workspace, st, &sync);
        if (e != hipSuccess) return (int)e;
        if (const int rc = issue(r0, rows - r0 < chunk ? rows - r0 : chunk, sync)) return rc;
    }
    return 0;
}

// Passes that fit the chip together go out as ONE launch; otherwise the first n - 1 by the same rule and then the last
// alone.  A pass with an order goes out alone too -- the kernels for passes side by side take none -- so a group that holds
// one falls back as a group that does not fit.  A lone pass beyond one launch runs in row ranges.
// `f`: one filter per job (checked by the caller), or null: none.  A job runs under its filter when it samples (mode 1) and
// the filter is not the identity.  `au`: the checked automaton of a constrained call, or null.  It applies to every
// free-running job, and a launch with such a job takes the constrained kernels.  Those pairs exist for M0 <= M1, so the passes
// go out in that order (a pass's result does not depend on where its tiles sit in the grid).  `order` / `tile_steps`: see
// any_order; the caller has checked the lists, and that a job with an order is teacher forced.  `steps_out`: as `order`, one
// entry per job; a job with one is free running without a filter or an automaton (checked by the caller), goes out alone as a
// job with an order does, and takes the kernels that stop (`end`: their end token).  A range from row r0 takes steps_out + r0.
// The LDS of a launch is the passes' own for the longest source plus what its family puts behind it -- the automaton's tables, or
// the tile's row indices -- and OVERLAP is picked with that counted: S <= 59, under the automaton S <= 58.
int launch_fwd(const pnmn_decoder_fwd_job* j, const pnmn_sampling_filter* f, int n, int hidden, void* workspace, hipStream_t st,
               const pnmn::TokenAutomaton* au, const int32_t* const* order, const int32_t* const* tile_steps,
               int32_t* const* steps_out = nullptr, int end = 0) {
    if (n > 1 && (!jobs_fit(j, n) || any_order(order, n) || any_order(steps_out, n))) {
        const int rc = launch_fwd(j, f, n - 1, hidden, workspace, st, au, order, tile_steps, steps_out, end);
        return rc != 0 ? rc : launch_fwd(j + n - 1, f ? f + n - 1 : nullptr, 1, hidden, workspace, st, au, from(order, n - 1),
                                         from(tile_steps, n - 1), steps_out ? steps_out + n - 1 : nullptr, end);
    }
    if (j[0].B <= 0 || j[0].T <= 0) return 0;  // (a lone pass only: passes side by side have rows and steps, see jobs_fit)
    int smax, chunk, rows[MAX_JOBS], tile0[MAX_JOBS + 1];
    if (const int e = plan_group(j, n, hidden, smax, chunk, rows, tile0)) return e;
    int m[2] = {0, 0};  // the kernels' M per pass
    pnmn::SamplingFilter ff[2] = {{1.f, 0, 1.f}, {1.f, 0, 1.f}};
    for (int i = 0; i < n; ++i) {
        m[i] = j[i].sample == 0 ? 0 : (f && j[i].sample == 1 && !pnmn::filter_is_identity(f[i])) ? 2 : 1;
        if (m[i] == 2) ff[i] = pnmn::SamplingFilter{f[i].temperature, f[i].top_k, f[i].top_p};
    }
    const bool ordered = any_order(order, 1);  // (n == 1 then)
    const bool stop = any_order(steps_out, 1);  // (n == 1, m[0] == 1 and no automaton then)
    const bool constrained = au && (m[0] != 0 || m[1] != 0);
    const bool filters = constrained || m[0] == 2 || m[1] == 2;  // (does the kernel take them?)
    const int lo = n > 1 && constrained && m[0] > m[1] ? 1 : 0, hi = 1 - lo;  // the order the passes go out in
    const size_t extras = constrained ? pnmn::AUTOMATON_LDS_BYTES : ordered || stop ? ORDER_LDS : 0;  // (S <= 59 still: 192 bytes are left there)
    const size_t base = FWD_FIXED_LDS + sizeof(float) * RW * smax * H + extras;
    // A teacher-forced launch of a call with an automaton stages no tables, but takes OVERLAP where the call's constrained
    // launches do: the two compilations of the body differ in the last bits, and a pass must compute the same bits alone
    // (a group that does not fit) and beside a free-running pass.
    const size_t as_pair = au && !constrained && !ordered ? pnmn::AUTOMATON_LDS_BYTES : 0;
    const bool overlap = base + as_pair + FWD_OVERLAP_LDS <= LDS_LIMIT;
    const size_t lds = base + (overlap ? FWD_OVERLAP_LDS : 0);
    const Variant* v = nullptr;
    if (const int e = find_variant({0, n, overlap, m[lo], n > 1 ? m[hi] : 0, constrained, ordered, stop}, v)) return e;
    const void* const f0 = filters ? &ff[lo] : nullptr;
    if (n > 1) {
        int* sync = nullptr;
        const hipError_t e = pnmn::cluster_sync_block(workspace, st, &sync);
        if (e != hipSuccess) return (int)e;
        const int tiles0 = padded_tiles(rows[lo]);
        const MFwdArgs a0 = kernel_args(j[lo], 0, rows[lo], sync, 0), a1 = kernel_args(j[hi], 0, rows[hi], sync, tiles0);
        return launch(*v, tile0[2], lds, st, {&a0, &a1, &tiles0, f0, filters ? &ff[hi] : nullptr, constrained ? au : nullptr});
    }
    return for_row_ranges(rows[0], chunk, workspace, st, [&](int r0, int part, int* sync) {
        // (an ordered range is addressed from the pass's base pointers: ordered_range)
        const MFwdArgs a = kernel_args(j[0], ordered ? 0 : (size_t)r0, part, sync, 0);
        const OrdArgs ord = ordered ? ordered_range((size_t)r0, rows[0], order[0], tile_steps[0]) : OrdArgs{};
        const StopArgs sa = stop ? StopArgs{steps_out[0] + r0, end} : StopArgs{};
        return launch(*v, padded_tiles(part), lds, st, {&a, f0, constrained ? au : nullptr, ordered ? &ord : nullptr, stop ? &sa : nullptr});
    });
}

int launch_bwd(const pnmn_decoder_bwd_job* j, int n, int hidden, void* workspace, hipStream_t st, const int32_t* const* order,
               const int32_t* const* tile_steps) {
    if (n > 1 && (!jobs_fit(j, n) || any_order(order, n))) {  // (as launch_fwd)
        const int rc = launch_bwd(j, n - 1, hidden, workspace, st, order, tile_steps);
        return rc != 0 ? rc : launch_bwd(j + n - 1, 1, hidden, workspace, st, from(order, n - 1), from(tile_steps, n - 1));
    }
    if (j[0].B <= 0 || j[0].T <= 0) return 0;  // (a lone pass only: passes side by side have rows and steps, see jobs_fit)
    int smax, chunk, rows[MAX_JOBS], tile0[MAX_JOBS + 1];
    if (const int e = plan_group(j, n, hidden, smax, chunk, rows, tile0)) return e;
    const bool ordered = any_order(order, 1);  // (n == 1 then)
    const size_t lds = BWD_FIXED_LDS + sizeof(float) * RW * smax * H + (ordered ? ORDER_LDS : 0);
    const Variant* v = nullptr;
    if (const int e = find_variant({1, n, 0, 0, 0, 0, ordered, 0}, v)) return e;
    float* x1 = reinterpret_cast<float*>(static_cast<char*>(workspace) + pnmn::CLUSTER_SYNC_BYTES);
    float* x2 = x1 + (size_t)exchange_tiles(rows, n, chunk) * 2 * MEMBERS * 2 * ROWS * H;
    if (n > 1) {
        int* sync = nullptr;
        const hipError_t e = pnmn::cluster_sync_block(workspace, st, &sync);
        if (e != hipSuccess) return (int)e;
        MBwdArgs a[MAX_JOBS];
        for (int i = 0; i < n; ++i) a[i] = kernel_args(j[i], 0, rows[i], sync, tile0[i], x1, x2);
        return launch(*v, tile0[n], lds, st, {&a[0], &a[1], n > 2 ? &a[2] : nullptr, &tile0[1], n > 2 ? &tile0[2] : nullptr});
    }
    return for_row_ranges(rows[0], chunk, workspace, st, [&](int r0, int part, int* sync) {
        const MBwdArgs a = kernel_args(j[0], ordered ? 0 : (size_t)r0, part, sync, 0, x1, x2);
        const OrdArgs ord = ordered ? ordered_range((size_t)r0, rows[0], order[0], tile_steps[0]) : OrdArgs{};
        return launch(*v, padded_tiles(part), lds, st, {&a, ordered ? &ord : nullptr});
    });
}

}  // namespace

extern "C" {

int64_t pnmn_attn_lstm_group_workspace_bytes(const int32_t* rows, int n, int backward) {
    if (!rows || n < 1 || n > MAX_JOBS) return 0;
    return workspace_bytes(rows, n, backward != 0);
}

// a job with an order: both lists, a teacher-forced pass, shapes inside the kernels' limits
static bool orders_valid(const int32_t* const* order, const int32_t* const* tile_steps, int n, int hidden, const int* S,
                         const int* sample) {
    if (!order != !tile_steps) return false;
    for (int i = 0; order && i < n; ++i) {
        if (!order[i] != !tile_steps[i]) return false;
        if (order[i] && (sample[i] != 0 || hidden != H || S[i] < 1 || S[i] > MAXS)) return false;
    }
    return true;
}

int pnmn_attn_lstm_fwd_group_stop(const pnmn_decoder_fwd_job* jobs, const pnmn_sampling_filter* filters, int end_index,
                                  const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left, int n_states,
                                  int n_classes, int n, int hidden, const int32_t* const* order, const int32_t* const* tile_steps,
                                  int32_t* const* steps_out, void* workspace, void* stream) {
    if (!jobs || !workspace || n < 1 || n > 2) return PNMN_EINVAL;
    for (int i = 0; filters && i < n; ++i)
        if (!pnmn::filter_valid(filters + i)) return PNMN_EINVAL;
    // a job with steps_out: free running, its end token inside the vocabulary, no filter of its own and no automaton
    for (int i = 0; steps_out && i < n; ++i) {
        if (!steps_out[i]) continue;
        if (jobs[i].sample == 0 || end_index < 0 || end_index >= jobs[i].V) return PNMN_EINVAL;
        if (token_class || next_state || min_left) return PNMN_EINVAL;
        if (filters && jobs[i].sample == 1 && !pnmn::filter_is_identity(filters[i])) return PNMN_EINVAL;
    }
    {
        const int S[2] = {jobs[0].S, n > 1 ? jobs[1].S : 0}, sample[2] = {jobs[0].sample, n > 1 ? jobs[1].sample : 0};
        if (!orders_valid(order, tile_steps, n, hidden, S, sample)) return PNMN_EINVAL;
    }
    if (!token_class && !next_state && !min_left)
        return launch_fwd(jobs, filters, n, hidden, workspace, static_cast<hipStream_t>(stream), nullptr, order, tile_steps,
                          steps_out, end_index);
    int V = 0, T = INT_MAX;  // of the free-running jobs: one automaton, one vocabulary; the fewest steps
    for (int i = 0; i < n; ++i) {
        if (jobs[i].sample == 0) continue;
        if (V != 0 && jobs[i].V != V) return PNMN_EINVAL;
        V = jobs[i].V;
        T = jobs[i].T < T ? jobs[i].T : T;
    }
    pnmn::TokenAutomaton au;
    if (const int e = pnmn::fill_automaton(au, token_class, next_state, min_left, n_states, n_classes, V, T, end_index)) return e;
    return launch_fwd(jobs, filters, n, hidden, workspace, static_cast<hipStream_t>(stream), &au, order, tile_steps);
}

int pnmn_attn_lstm_fwd_group_ordered(const pnmn_decoder_fwd_job* jobs, const pnmn_sampling_filter* filters, int end_index,
                                     const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left, int n_states,
                                     int n_classes, int n, int hidden, const int32_t* const* order,
                                     const int32_t* const* tile_steps, void* workspace, void* stream) {
    return pnmn_attn_lstm_fwd_group_stop(jobs, filters, end_index, token_class, next_state, min_left, n_states, n_classes, n, hidden,
                                         order, tile_steps, nullptr, workspace, stream);
}

int pnmn_attn_lstm_fwd_group(const pnmn_decoder_fwd_job* jobs, const pnmn_sampling_filter* filters, int end_index,
                             const uint8_t* token_class, const uint8_t* next_state, const uint8_t* min_left, int n_states,
                             int n_classes, int n, int hidden, void* workspace, void* stream) {
    return pnmn_attn_lstm_fwd_group_ordered(jobs, filters, end_index, token_class, next_state, min_left, n_states, n_classes, n,
                                            hidden, nullptr, nullptr, workspace, stream);
}

int pnmn_attn_lstm_bwd_group_ordered(const pnmn_decoder_bwd_job* jobs, int n, int hidden, const int32_t* const* order,
                                     const int32_t* const* tile_steps, void* workspace, void* stream) {
    if (!jobs || !workspace || n < 1 || n > MAX_JOBS) return PNMN_EINVAL;
    {
        int S[MAX_JOBS], sample[MAX_JOBS];
        for (int i = 0; i < n; ++i) S[i] = jobs[i].S, sample[i] = 0;
        if (!orders_valid(order, tile_steps, n, hidden, S, sample)) return PNMN_EINVAL;
    }
    return launch_bwd(jobs, n, hidden, workspace, static_cast<hipStream_t>(stream), order, tile_steps);
}

int pnmn_attn_lstm_bwd_group(const pnmn_decoder_bwd_job* jobs, int n, int hidden, void* workspace, void* stream) {
    return pnmn_attn_lstm_bwd_group_ordered(jobs, n, hidden, nullptr, nullptr, workspace, stream);
}

}  // extern "C"
