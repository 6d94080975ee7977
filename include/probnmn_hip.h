/*
 * probnmn_hip.h -- C ABI of libprobnmn_hip.so, the MI355X (gfx950) kernels behind the
 * probnmn.models / probnmn.modules class surface.
 *
 * The reference (kdexd/probnmn-clevr) has no FFI of its own: its hot path is torch ops called
 * from Python.  Each entry point below therefore cites the reference torch call
 * site(s) it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer into caller-owned, contiguous fp32 / int64 / int32 memory;
 *     the library allocates nothing and keeps no state -> re-entrant per device;
 *   - activations are NHWC ("channels last"): a feature map is [H*W][C] floats; conv weights are
 *     [Cout][KH*KW][Cin] (what torch calls channels_last for a [Cout,Cin,KH,KW] tensor);
 *   - work is described by arrays of fixed-size "item" records living in device memory, so one
 *     launch executes the same op for many (example, module) pairs with different weights --
 *     this is how the per-example dynamic program composition of nmn.py:197-238 is batched;
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*), never synchronise;
 *   - return 0 on success, a negative PNMN_E* for argument errors, a positive hipError_t
 *     otherwise.
 * No torch types appear anywhere in this interface.
 *
 * Declaration conventions.  The Python binding (probnmn/_hip.py) is derived from this file when it is imported: an
 * entry point, record or constant is added HERE (and defined in csrc), nowhere else.  Its reader relies on:
 *   - a prototype starts its line with the return type, `int` or `int64_t`, and ends with `);`
 *   - a record is one `typedef struct [tag] { ... } pnmn_x;` of pointers, fixed-width scalars (int32_t, uint32_t,
 *     int64_t, uint64_t, float, double) and arrays of them -- no nested records, unions or bit fields
 *   - scalar parameters are int, int32_t, uint32_t, int64_t, uint64_t, float or double; anything with a `*` is a pointer
 *   - a host argument block -- a few scalars the caller fills in HOST memory and an entry point reads before it returns,
 *     never an element of a device work list -- is a plain `struct pnmn_x { ... };` of the same field kinds, named
 *     `struct pnmn_x` in prototypes; the binding derives its dtype too, beside the records, not among them
 *   - a constant is `#define PNMN_NAME <integer>` or `(<negative integer>)`
 * A pnmn_ declaration written any other way makes the import fail with its text (tests/test_abi.py).
 *
 * Options.  An option is a nullable trailing argument of the entry point it modifies, never a second entry point.  For the
 * decoders (pnmn_sample_tokens, pnmn_attn_lstm_fwd, _fwd_group, _beam, pnmn_prior_sample):
 *   - filter == NULL (group: filters == NULL) means the identity filter;
 *   - token_class, next_state and min_left all NULL means unconstrained: end_index, n_states and n_classes are then ignored
 *     (but for pnmn_attn_lstm_beam's end_index, which the search itself uses); some but not all of the three given returns PNMN_EINVAL.
 */
#ifndef PROBNMN_HIP_H
#define PROBNMN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNMN_EINVAL (-1)   /* bad argument                                   */
#define PNMN_ESHAPE (-2)   /* shape not supported by the gfx950 kernels      */

#define PNMN_CHANNELS 128  /* module_channels the LDS tiling is built for    */

/* ---------------------------------------------------------------------------------------------
 * Grouped convolution, forward and data-gradient.
 * Replaces: F.relu(conv3x3(feats * attn.repeat(...)))   nmn_modules.py:83-85,120-122,161-166
 *           stem convs                                   nmn.py:67-72,183
 *           ComparisonModule.projection on cat(in1,in2)  nmn_modules.py:241
 *           classifier conv1x1                           nmn.py:76
 *           and, with transposed weights + `gate`, the autograd dgrad of all of them.
 * One item = one example's feature map through one convolution:
 *   x[p][c]   = in[p*in_stride + c]            (chunk k of 128 input channels at in + 128k,
 *                                               or taken from in2 for k>=1 when in2 != NULL)
 *   x        *= mask[p]                        if mask  (single-channel attention, broadcast)
 *   x         = gate[p*in_stride+c] > 0 ? x:0  if gate  (ReLU backward fused into the load)
 *   out[p*out_stride + n] = act(bias[n] + sum_{tap,c} x[shift(p,tap,dil)][c] * W[n][tap][c])
 *   (added to the previous contents of out when flags & PNMN_CONV_ACCUMULATE)
 * Shapes: H x W = 14 x 14 (one workgroup stages the whole map) and 28 x 28 (NMN.IMAGE_FEATURE_SIZE
 * [1024,28,28], nmn.py:46-53: four row bands per item, each staging the rows its taps touch);
 * anything else returns PNMN_ESHAPE.
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_conv_item {
    const float* in;
    const float* in2;
    const float* mask;
    const float* gate;
    const float* weight;   /* [cout_total][ntaps][cin_chunks*128] */
    const float* bias;     /* [cout_total] or NULL                */
    float*       out;
    int32_t      dilation;
    int32_t      flags;    /* PNMN_CONV_ACCUMULATE: out += result (plain read-modify-write) */
    /* fused backward of `feats * attn` (flags & PNMN_CONV_MASKBWD; data-gradient of a conv whose
     * forward input was the masked stem output): instead of storing the result dx to `out`,
     *   mb_dfeats[p][c] += dx[p][c] * mb_attn[p];   mb_dattn[p] += sum_c dx[p][c] * mb_feats[p][c]
     * with fp32 atomics; mb_attn == NULL means the all-ones attention (no mb_dattn). */
    const float* mb_feats;
    const float* mb_attn;
    float*       mb_dfeats;
    float*       mb_dattn;
} pnmn_conv_item;          /* 96 bytes */
#define PNMN_CONV_ACCUMULATE 1
#define PNMN_CONV_ATOMIC     2   /* with ACCUMULATE: add with fp32 atomics (concurrent writers) */
#define PNMN_CONV_MASKBWD    4   /* fused mask backward epilogue (see the mb_* fields) */
#define PNMN_CONV_DATTN     16   /* dx is STORED to `out` as usual and only mb_dattn[p] += sum_c dx[p][c] * mb_feats[p][c] is
                                    fused (the d(feats) half of the mask backward is left to pnmn_feat_grad_gather) */
#define PNMN_CONV_MB_SOLE     8   /* with MASKBWD: no other item of this launch adds into the same
                                     mb_dfeats map -> plain read-modify-write instead of atomics */

int pnmn_conv_nhwc(const pnmn_conv_item* items, int n_items, int H, int W, int cin_chunks,
                   int ntaps /* 9 or 1 */, int in_stride, int out_stride,
                   int cout_blocks /* cout_total / 128 */, int relu, void* stream);
/* The same with the number of CUs the launch may count on (0 = all of them): the launch planner cuts the items into
 * rounds of that many workgroups.  For launches that share the chip with other streams' kernels (the joint step's trunk
 * beside the seq2seq passes).  In a pnmn_launch entry the `c` field of a CONV carries it. */
int pnmn_conv_nhwc_cus(const pnmn_conv_item* items, int n_items, int H, int W, int cin_chunks, int ntaps, int in_stride,
                       int out_stride, int cout_blocks, int relu, int cus, void* stream);
/* Kernel launches one pnmn_conv_nhwc call with these sizes makes (1 since round 3: the segments of different splits
 * go out as one launch; 0 for an empty call or an unsupported map size) -- for per-launch accounting. */
int pnmn_conv_nhwc_launches(int n_items, int H, int W, int cin_chunks, int ntaps, int cout_blocks);
/* Tuning / test hook: every later convolution launch of this process uses ONE split -- 1, 2, 4, 6, 8, 14 or 26 workgroups
 * per (item, 128-channel output block), which share its 128 output channels (and from 4 on its pixel tiles); 6, 14 and 26
 * exist for 3x3 launches only: a 1x1 launch under one of them is planned as if none were forced.  The results do not
 * depend on it (every output sums all its input channels in one wave, in one order).  0 = the launch planner decides
 * again; any other value returns PNMN_EINVAL and changes nothing.  Also settable as PNMN_CONV_KSPLIT before the first
 * launch. */
int pnmn_conv_force_split(int split);

/* ---------------------------------------------------------------------------------------------
 * Grouped convolution weight-gradient (autograd wgrad of the convs above).
 *   dW[n][tap][c] += sum_items sum_p dy[p][n] * (gate[p][n] > 0) * x[shift(p,tap,dil)][c]
 * A job = a run of items sharing one weight; the kernel accumulates a job's items in registers
 * and adds the result into dw with fp32 atomics (dw must be zeroed by the caller beforehand).
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_wgrad_item {
    const float* x;        /* [HW][x_stride]  forward input of the conv               */
    const float* x2;       /* second source for input-channel blocks >= 1, or NULL    */
    const float* xmask;    /* [HW] attention multiplied onto x in the forward, or NULL */
    const float* dy;       /* [HW][dy_stride] gradient wrt the conv output            */
    const float* gate;     /* [HW][dy_stride] forward output (ReLU gate), or NULL     */
    int32_t      dilation;
    int32_t      reserved;
} pnmn_wgrad_item;         /* 48 bytes */

typedef struct pnmn_wgrad_job {
    float*  dw;            /* [cout_total][ntaps][cin_total] accumulated into        */
    float*  dbias;         /* [cout_total] accumulated into, or NULL                 */
    int32_t item_begin;
    int32_t item_end;
} pnmn_wgrad_job;          /* 24 bytes */

int pnmn_conv_wgrad(const pnmn_wgrad_item* items, const pnmn_wgrad_job* jobs, int n_jobs, int H,
                    int W, int ntaps, int cin_blocks, int cout_blocks, int x_stride,
                    int dy_stride, void* stream);
/* The same with a CU budget (0 = none; 14x14 maps): at most `cus` workgroups, each walking several (job, slab) units --
 * for launches that share the chip with other streams' kernels.  In a pnmn_launch entry p[7] of a WGRAD carries it.
 * The budget only changes how the work is cut, never the sums.  What a value means, path by path:
 *   3x3 at 14x14 and classifier-shaped 1x1 (one input block, even cout_blocks, at most 512 jobs; either map size):
 *     1..256 is the budget; anything else (0, negative, larger) sizes the launch for the whole chip;
 *   other 1x1 at 14x14: any cus >= 1 below the number of (job, slab) units is the number of workgroups, which walk the
 *     units (values above 256 included); anything else gives one workgroup per unit;
 *   the banded 28x28 kernels (3x3, and every 1x1 launch that is not classifier-shaped) ignore it.
 * A job may be empty (item_begin == item_end: nothing is added), and every item carries its own dilation -- the items of
 * one job need not share it. */
int pnmn_conv_wgrad_cus(const pnmn_wgrad_item* items, const pnmn_wgrad_job* jobs, int n_jobs, int H, int W, int ntaps,
                        int cin_blocks, int cout_blocks, int x_stride, int dy_stride, int cus, void* stream);

/* [Cout][taps][Cin] -> [Cin][taps reversed][Cout] for a list of weights (dgrad operand). */
typedef struct pnmn_wtrans_item {
    const float* src;
    float*       dst;
    int32_t      cout, cin, ntaps, reserved;
} pnmn_wtrans_item;        /* 32 bytes */
int pnmn_transpose_weights(const pnmn_wtrans_item* items, int n_items, void* stream);

/* ---------------------------------------------------------------------------------------------
 * conv1x1(128 -> 1) + sigmoid                       nmn_modules.py:86,167
 *   out[p] = sigmoid(b + sum_c in[p][c] * w[c])
 * backward: dz = dout*out*(1-out); din[p][c] = dz[p]*w[c]; dw[c] += sum_p dz[p]*in[p][c];
 *           db += sum_p dz[p]      (dw/db via fp32 atomics; din written, not accumulated)
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_dot1_item {
    const float* in;    /* [HW][128]                 */
    const float* w;     /* [128]                     */
    const float* b;     /* [1]                       */
    float*       out;   /* [HW]    fwd: written; bwd: read */
    const float* dout;  /* [HW]    bwd only          */
    float*       din;   /* [HW][128] bwd only        */
    float*       dw;    /* [128]   bwd only          */
    float*       db;    /* [1]     bwd only          */
} pnmn_dot1_item;       /* 64 bytes */
int pnmn_dot1_sigmoid_fwd(const pnmn_dot1_item* items, int n_items, int HW, void* stream);
int pnmn_dot1_sigmoid_bwd(const pnmn_dot1_item* items, int n_items, int HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SameModule                                         nmn_modules.py:200-208
 *   j = argmax_p attn[p] (first maximum, as max_pool2d); v[c] = feats[j][c]
 *   out[p] = sigmoid(b + sum_c w[c]*feats[p][c]*v[c] + w[128]*attn[p])
 * backward accumulates dfeats (+=) and dattn (+=; may be NULL), accumulates dw[129]/db with atomics.
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_same_item {
    const float* feats;  /* [HW][128] */
    const float* attn;   /* [HW]      */
    const float* w;      /* [129]     */
    const float* b;      /* [1]       */
    float*       out;    /* [HW]      */
    const float* dout;   /* bwd */
    float*       dfeats; /* bwd, += */
    float*       dattn;  /* bwd, += (may be NULL) */
    float*       dw;     /* bwd, atomics */
    float*       db;     /* bwd, atomics */
} pnmn_same_item;        /* 80 bytes */
int pnmn_same_fwd(const pnmn_same_item* items, int n_items, int HW, void* stream);
int pnmn_same_bwd(const pnmn_same_item* items, int n_items, int HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * And / Or: elementwise min / max with 1 <-> C channel broadcast    nmn_modules.py:25-27,43-45
 * backward routes the gradient to the selected operand (ties: half each, as torch.minimum),
 * summing over channels for a broadcast operand; da / db are accumulated (+=).
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_minmax_item {
    const float* a;
    const float* b;
    float*       out;     /* fwd: written */
    const float* dout;    /* bwd */
    float*       da;      /* bwd, += (may be NULL) */
    float*       db;      /* bwd, += (may be NULL) */
    int32_t      a_channels, b_channels;   /* 1 or C */
    int32_t      is_max, reserved;
} pnmn_minmax_item;       /* 64 bytes */
int pnmn_minmax_fwd(const pnmn_minmax_item* items, int n_items, int HW, int C, void* stream);
int pnmn_minmax_bwd(const pnmn_minmax_item* items, int n_items, int HW, int C, void* stream);

/* Backward of `feats * attn.repeat(1,C,1,1)` (nmn_modules.py:83,120,161):
 *   dattn[p] += sum_c dx[p][c]*feats[p][c];  dfeats[p][c] += dx[p][c]*attn[p]   (both with atomics: items may share maps)
 * attn == NULL means the all-ones attention `scene` produces: dfeats += dx, no dattn. */
typedef struct pnmn_maskbwd_item {
    const float* dx;
    const float* feats;
    const float* attn;
    float*       dfeats;
    float*       dattn;
} pnmn_maskbwd_item;      /* 40 bytes */
int pnmn_mask_bwd(const pnmn_maskbwd_item* items, int n_items, int HW, void* stream);
/* The d(feats) half of the backward of `feats * attn`, deferred to the end of the module programs' backward pass:
 * for every example e of the batch, gfeat[e][p][c] += sum over the items i whose `dfeats` is gfeat[e] of
 * items[i].dx[p][c] * items[i].attn[p] (attn == NULL: all ones).  `items` is sorted by `dfeats`; one workgroup per
 * (example, pixel range) finds its items by bisection, reads every dx map once and writes its range of gfeat[e] once
 * (no atomics, no read-modify-write per item: the fused epilogue this replaces re-read and re-wrote the 100 KB map
 * of d(feats) once per masked convolution).  Only `dx`, `attn`, `dfeats` of the items are read. */
int pnmn_feat_grad_gather(const pnmn_maskbwd_item* items, float* gfeat, int n_items, int n_examples, int HW, void* stream);

/* dst[p][c] += src[p][c] for a list of [HW][128] maps (fan-in of value gradients). */
typedef struct pnmn_axpy_item {
    const float* src;
    float*       dst;
    int64_t      n;
} pnmn_axpy_item;         /* 24 bytes */
int pnmn_accumulate(const pnmn_axpy_item* items, int n_items, void* stream);
/* dst[0..n) = src[0..n), or zeros where src is NULL: the classifier-input rows of programs whose result is the stem's
 * feature map itself (nmn.py:227-233: `output` stays feat_input) and of invalid programs (nmn.py:236-238:
 * zeros_like(feat_input)) -- one launch instead of an index_fill_ and an index_copy_ between the grouped launches. */
int pnmn_set_rows(const pnmn_axpy_item* items, int n_items, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Layout changes at the boundary: the reference hands NCHW features (datasets.py:137-142).
 * ------------------------------------------------------------------------------------------- */
int pnmn_nchw_to_nhwc(const float* src, float* dst, int n, int C, int HW, void* stream);
/* the same for a subset of a batch: example i of dst is example rows[i] of src (no gathered copy of the 0.8 MB maps) */
int pnmn_nchw_to_nhwc_rows(const float* src, float* dst, const int64_t* rows, int n, int C, int HW, void* stream);
int pnmn_nhwc_to_nchw(const float* src, float* dst, int n, int C, int HW, void* stream);

/* Feature ingest: replaces the per-item h5 read + float cast + collate + .to(device) of
 * probnmn/data/readers.py:63-108, datasets.py:137-142, trainers/_trainer.py:272-287 AND the layout change
 * above.  `store` is a DEVICE-VISIBLE pointer to page-locked HOST memory holding [n_store][C][HW] fp32
 * (hipHostMalloc / a torch pinned tensor); `indices` [n] int64 on the device; dst [n][HW][C] on the
 * device.  The kernel reads the selected rows over PCIe.  (= pnmn_gather_features_typed with F32, F32.) */
int pnmn_gather_features(const float* store, const int64_t* indices, float* dst, int n, int64_t n_store,
                         int C, int HW, void* stream);
/* Element types of a feature store.  The networks compute in fp32; a store may keep its rows in half or a quarter of
 * the bytes.  (3 is no element type.) */
#define PNMN_ELEM_F32  0
#define PNMN_ELEM_F16  1   /* IEEE binary16 */
#define PNMN_ELEM_BF16 2   /* bfloat16: the upper half of a binary32 */
#define PNMN_ELEM_F8E4M3 4 /* OCP e4m3fn (torch.float8_e4m3fn): no infinities, 0x7f / 0xff are NaN, largest finite 448 */
#define PNMN_ELEM_F8E5M2 5 /* e5m2 (torch.float8_e5m2): IEEE-like, infinities exist, largest finite 57344 */
/* pnmn_gather_features with the element types as parameters: `store` [n_store][C][HW] of `src_elem` (page-locked host
 * memory or device memory), dst [n][HW][C] of `dst_elem`.  Supported: F16 | BF16 | F8E4M3 | F8E5M2 -> F32 (a narrow
 * store feeding a batch; widening is exact for every code, NaN to NaN), F32 -> F16 | BF16 | F8E4M3 | F8E5M2 (filling a
 * narrow device store from the fp32 staging buffer: round to nearest even, subnormals kept, overflow to infinity --
 * to NaN for F8E4M3, which has no infinity: |x| > 464 -- what torch's Tensor.to(dtype) does on the host) and F32 ->
 * F32 (what pnmn_gather_features runs).  Any other pair returns PNMN_EINVAL.  The same fixed grid of at most 12
 * workgroups and the same 26 KB LDS bound for every pair; an index outside [0, n_store) reads row 0. */
int pnmn_gather_features_typed(const void* store, int src_elem, const int64_t* indices, void* dst, int dst_elem, int n,
                               int64_t n_store, int C, int HW, void* stream);
/* Rows of a narrow store that lives in device memory, widened: rows [n_store][row_elems] F16, BF16, F8E4M3 or F8E5M2
 * (already NHWC), indices [n] int64 on the device, dst [n][row_elems] fp32; dst row i = rows[indices[i]] (an index
 * outside [0, n_store) reads row 0).  No transpose.  16-byte loads when row_elems is a multiple of the 8 or 16 elements
 * in them and both bases are 16-byte aligned (every row then starts aligned), element by element otherwise.  Runs in
 * front of the stem on the step's own stream and uses the whole chip.  Any other src_elem returns PNMN_EINVAL. */
int pnmn_expand_rows(const void* rows, int src_elem, const int64_t* indices, void* dst, int n, int64_t n_store,
                     int64_t row_elems, void* stream);
/* An fp32 chunk that is already in device memory, in the store's own order, rounded into an 8-bit store: src [n_elems]
 * fp32, dst [n_elems] of `dst_elem` (F8E4M3 or F8E5M2; anything else returns PNMN_EINVAL), the rounding of
 * pnmn_gather_features_typed.  `overflowed` (device) is incremented by the number of elements that were finite in fp32
 * and are not after narrowing: the caller's running count, which a stream-ordered fill cannot turn into an error. */
int pnmn_narrow_rows(const float* src, void* dst, int dst_elem, int64_t n_elems, uint64_t* overflowed, void* stream);
/* The same rows through the copy engines instead of a kernel: n hipMemcpyAsync of `row_bytes` each from the
 * page-locked store into a contiguous (NCHW, as stored) device batch.  `indices` is a HOST array; an index outside
 * [0, n_store) returns PNMN_EINVAL with the copies before it queued.  The stem's layout pass then reads the batch
 * like any NCHW input (readers.py:63-108 + _trainer.py:272-287: lookup, cast, collate, .to(device)). */
int pnmn_copy_rows_h2d(const void* store, const int64_t* indices, void* dst, int n, int64_t n_store,
                       int64_t row_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * classifier.1-3: ReLU (already applied by the conv) + MaxPool2d(2,2) + Flatten   nmn.py:77-79
 *   in  [n][H*W][C] NHWC  ->  out [n][C*(H/2)*(W/2)] in the reference's NCHW-flatten order
 * backward scatters dout to the arg-max position (first maximum in window scan order, as torch)
 * and applies the ReLU gate of the conv output.
 * ------------------------------------------------------------------------------------------- */
int pnmn_maxpool2_flatten_fwd(const float* in, float* out, int n, int H, int W, int C, void* stream);
int pnmn_maxpool2_flatten_bwd(const float* in, const float* dout, float* din, int n, int H, int W,
                              int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Answer loss                                                          nmn.py:245-269
 *   logprobs = log_softmax(logits[b]); pred[b] = argmax (first); loss[b] = -logprobs[answer[b]]
 *   (answers == NULL: loss[b] = -max logprob, dlogits = 0); invalid rows: pred = unknown_index, loss = 3.33
 *   dlogits[b] = (softmax - onehot) * scale for valid rows, 0 for invalid rows.
 * ------------------------------------------------------------------------------------------- */
int pnmn_answer_loss(const float* logits, const int64_t* answers, const int32_t* valid,
                     int64_t* predictions, float* loss, float* dlogits, int n, int num_answers,
                     int unknown_index, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Marginal answer over several programs (csrc/answer_marginal.hip).  Not in the reference, which answers from ONE
 * program: it extends nmn.py:245-269 (log-softmax and first arg-max of one row of logits, @@UNKNOWN@@ for an invalid
 * program) and scripts/inference.py:76-91 (one sampled program per question) to
 *     p(a | x, image) = sum_z q(z | x) p(a | z, image)
 * over the hypothesis rows of each question.  Rows [group_start[g], group_start[g + 1]) are group g's, in that order.
 *   row r is USABLE when (valid == NULL or valid[r] != 0) and (log_weight == NULL or log_weight[r] is finite)
 *   support[g]         = number of usable rows of group g
 *   w_r                = exp(log_weight[r] - logsumexp of log_weight over the group's usable rows);
 *                        log_weight == NULL: w_r = 1 / support[g]
 *   row_weight[r]      = w_r for a usable row, 0 otherwise
 *   row_predictions[r] = first arg-max of logits[r] (pnmn_answer_loss's rule); unknown_index where valid[r] == 0
 *   log_marginal[g][a] = log sum over usable rows of w_r * softmax(logits[r])[a], in log space with the maxima subtracted
 *                        (finite fp32 logits)
 *   predictions[g]     = first arg-max of log_marginal[g] as stored
 *   support[g] == 0 (no rows, all invalid, or no finite weight): log_marginal[g][:] = -inf, predictions[g] = unknown_index
 * Group bounds are clamped into [0, n_rows] with end >= start before use, so no group_start reads or writes outside the
 * arrays; a row that no group covers is not written, a row that two groups cover is written by both.  A group's outputs
 * depend only on its own rows in their order: the same bits alone or inside a batch, and from run to run.  One launch,
 * one wavefront per group, no LDS, no atomics, no wait on another workgroup.
 * n_groups == 0 returns 0 without a launch.  PNMN_EINVAL, with no launch and no HIP call: a null logits (n_rows > 0),
 * group_start, log_marginal or predictions; num_answers < 1; n_rows < 0; n_groups < 0.  num_answers > 1024: PNMN_ESHAPE.
 * ------------------------------------------------------------------------------------------- */
int pnmn_answer_marginal(const float* logits /* [n_rows][num_answers] */, const int32_t* valid /* [n_rows], may be NULL */,
                         const float* log_weight /* [n_rows], may be NULL */, const int32_t* group_start /* DEVICE [n_groups + 1] */,
                         float* log_marginal /* [n_groups][num_answers] */, int64_t* predictions /* [n_groups] */,
                         int64_t* row_predictions /* [n_rows], may be NULL */, float* row_weight /* [n_rows], may be NULL */,
                         int32_t* support /* [n_groups], may be NULL */, int n_groups, int n_rows, int num_answers,
                         int unknown_index, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Posterior over a question's program hypotheses (csrc/hypothesis_posterior.hip).  Not in the reference, which scores
 * sampled programs with the prior and the reconstructor in training only (elbo.py:130-161) and answers from one sampled
 * program (scripts/inference.py:76-91): the hypotheses of a question reranked by
 *     score[r] = w_x log p(x | z_r) + w_z log p(z_r) + w_q log q(z_r | x)
 * from the teacher-forced logits of the reconstructor (x) and of the prior (z) and the tokens they score.  Rows
 * [group_start[g], group_start[g + 1]) are group g's, in that order, as for pnmn_answer_marginal.
 * Per row, for a term k in {x, z} whose logits are given (row r's tokens are the T_k entries at k_tokens + r * k_token_stride):
 *   lp_k[r] = sum over t with tok_k[r][t] != pad_k of (z_t[tok] - max_v z_t) - log sum_v exp(z_t[v] - max_v z_t),
 *             z_t = k_logits[r][t][:]: every step rounded at its own size, summed over t in ascending order; 0 for a row
 *             whose tokens are all padding; a true log-probability (a sum): with n scored tokens, -lp_k / n is
 *             pnmn_seq_nll_fwd's loss for the same logits and tokens
 *   a token that is neither pad_k nor in [0, V_k) is never used as an index: lp_k[r] = -inf
 *   log_px[r] = lp_x[r], log_pz[r] = lp_z[r] (each written only when its logits are given; a term that neither is asked
 *             for nor enters the score is not computed)
 * A term ENTERS the score only when its input pointer (x_logits, z_logits, log_q) is not NULL and its coefficient is not
 * exactly 0: a term that does not is left out entirely, no 0 * -inf is ever formed, and a NULL input gives the same bits as
 * a zero coefficient.  Row r is USABLE when score[r] is finite.  Per group, over its usable rows:
 *   support[g]       = their number
 *   log_evidence[g]  = max + log sum exp(score - max), max being the largest usable score
 *   log_posterior[r] = (score[r] - max) - log sum exp(score - max); -inf for a row that is not usable
 *   best_row[g]      = the absolute index r of the first usable row with the largest score
 *   support[g] == 0 (no rows, or none usable): log_evidence[g] = -inf, best_row[g] = -1, log_posterior = -inf over the rows
 * Group bounds are clamped into [0, n_rows] with end >= start before use, so no group_start reads or writes outside the
 * arrays; a row that no group covers is not written.  The scores of a group pass through its log_posterior slots, so groups
 * that share a row (bounds that decrease) get unspecified values -- every other group keeps its own.  A group's outputs
 * depend only on its own rows in their order: the same bits alone or inside a batch, and from run to run.  One launch, one
 * 512-thread workgroup per group (its wavefronts take the rows in turn), no LDS, no atomics, no wait on another workgroup.
 * n_groups == 0 returns 0 without a launch.  PNMN_EINVAL, with no launch and no HIP call: n_groups < 0 or n_rows < 0; a
 * null group_start, log_posterior, log_evidence or best_row; logits without their tokens; x_logits, z_logits and log_q all
 * null; T < 1 or V < 1 of a term whose logits are given; a coefficient that is not finite.  Vx or Vz > 1024 (of a term
 * whose logits are given): PNMN_ESHAPE.  The checks run in this order: the counts; then the empty case -- n_groups == 0
 * returns 0 whatever else is given --; then the pointers, the sizes of the given terms and the coefficients; then the shape.
 *
 * GRADIENT MODE: best_row == NULL and at least one of log_px, log_pz != NULL.  The marginal-likelihood loss of group g over
 * its candidate rows is -log_evidence[g] = -log sum_r p(x | z_r)^w_x p(z_r)^w_z q(z_r | x)^w_q; this mode computes it together
 * with its gradient with respect to the logits of every sequence term -- a row's per-step cross-entropy gradient scaled by
 * the row's posterior share.  The log_px slot is then read as d_x_logits, fp32 [n_rows][Tx][Vx], and requires x_logits; the
 * log_pz slot is read as d_z_logits, fp32 [n_rows][Tz][Vz], and requires z_logits (PNMN_EINVAL otherwise).  lp_x and lp_z
 * themselves are not reported and best_row is not written.  log_posterior, log_evidence and support keep their rules and
 * are the same bits as a launch with best_row on the same inputs.  For a term k in {x, z} whose slot is given, over a
 * second sweep of the group's rows, with share_k[r] = w_k * exp(log_posterior[r]):
 *   d_k_logits[r][t][v] = share_k[r] * (softmax(k_logits[r][t])[v] - [v == tok_k[r][t]])   for a usable row r and a scored
 *                         step t (tok_k[r][t] != pad_k)
 *                       = d(-log_evidence[g]) / d k_logits[r][t][v]; a logit of -inf gets exactly 0
 *   d_k_logits[r][t][v] = 0 exactly for every padding step of a covered row; for every step of a covered row that is not
 *                         usable (a row with a token that is no index, whose lp is -inf, among them) -- so for every row of
 *                         a group without support --; and for every covered row of a term that does not enter the score
 *                         (w_k exactly 0), whose logits are then not read
 * A row that no group covers is not written; the target's column is found by comparing v, never by indexing with an
 * unchecked token.  A group's d_logits rows depend only on its own rows in their order: the same bits alone or inside a
 * batch, and from run to run.  One launch, no LDS, no atomics, no wait on another workgroup; every wavefront of the
 * workgroup reaches both of its barriers.  The checks, their order and their codes are those above with "best_row" read as
 * "best_row or (in its absence) a log_px / log_pz slot": log_posterior and log_evidence remain required.  No call that was
 * accepted before this mode existed changes its meaning or its bits: every such call passed a best_row, and a call without
 * one was refused with PNMN_EINVAL -- a call with none of best_row, log_px and log_pz still is.  The derivative with respect
 * to log_q, d(-log_evidence[g]) / d log_q[r] = -w_q * exp(log_posterior[r]), is a function of an output and has no slot:
 * the caller forms it.
 * ------------------------------------------------------------------------------------------- */
int pnmn_hypothesis_posterior(const float* x_logits /* [n_rows][Tx][Vx], may be NULL */, const int64_t* x_tokens /* [n_rows] rows of Tx */,
                              int64_t x_token_stride, const float* z_logits /* [n_rows][Tz][Vz], may be NULL */,
                              const int64_t* z_tokens /* [n_rows] rows of Tz */, int64_t z_token_stride,
                              const float* log_q /* [n_rows], may be NULL */, const int32_t* group_start /* DEVICE [n_groups + 1] */,
                              float w_x, float w_z, float w_q, int pad_x, int pad_z, float* log_px /* [n_rows], may be NULL */,
                              float* log_pz /* [n_rows], may be NULL */, float* log_posterior /* [n_rows] */,
                              float* log_evidence /* [n_groups] */, int32_t* best_row /* [n_groups] */,
                              int32_t* support /* [n_groups], may be NULL */, int n_groups, int n_rows, int Tx, int Vx, int Tz,
                              int Vz, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Posterior over a question's program hypotheses given its ANSWER (csrc/answer_posterior.hip).  Not in the reference,
 * which uses p(a | z, image) only to answer from one sampled program (nmn.py:245-269, scripts/inference.py:76-91) and
 * never to judge the program: the hypotheses of a question reranked by
 *     score[r] = log_w[r] + w_a log p(a | z_r, image)
 * from the answer logits of every hypothesis row, the given answer answers[g] of each question and the log-weight a row
 * has before the answer is seen -- log q(z_r | x), or pnmn_hypothesis_posterior's log_posterior, with which (w_a = 1) the
 * result is p(z | x, a, image) on the candidate set.  Rows [group_start[g], group_start[g + 1]) are group g's, in that
 * order, as for pnmn_answer_marginal.
 *   row r is BASE-USABLE when (valid == NULL or valid[r] != 0) and (log_weight == NULL or log_weight[r] is finite)
 *   log_w[r]           = log_weight[r] - logsumexp of log_weight over the group's base-usable rows; log_weight == NULL:
 *                        -log of their number
 *   log_answer[r]      = (z[a] - max z) - log sum exp(z - max z), z = logits[r], a = answers[g]; written for every covered
 *                        row, base-usable or not; an answer outside [0, num_answers) is never used as an index:
 *                        log_answer[r] = -inf
 *   row_predictions[r] = first arg-max of logits[r]; unknown_index where valid[r] == 0 (pnmn_answer_marginal's rule)
 *   score[r]           = log_w[r] + w_a * log_answer[r]; when w_a is exactly 0 the answer term is left out entirely -- no
 *                        0 * -inf is formed -- and log_answer is still reported
 * Row r is USABLE when it is base-usable and score[r] is finite.  Per group, over its usable rows:
 *   support[g]          = their number
 *   log_evidence[g]     = max + log sum exp(score - max), max being the largest usable score; with w_a = 1 it is
 *                         log p(a | x, image) on the candidate set: pnmn_answer_marginal's log_marginal[g][answers[g]]
 *   log_posterior[r]    = (score[r] - max) - log sum exp(score - max); -inf for a covered row that is not usable
 *   best_row[g]         = the absolute index r of the first usable row with the largest score
 *   consistent_count[g] = number of usable rows whose row_predictions equals answers[g]
 *   first_consistent[g] = the absolute index of the first such row, -1 when there is none
 *   support[g] == 0 (no rows, or none usable): log_evidence[g] = -inf, best_row[g] = -1, consistent_count[g] = 0,
 *                         first_consistent[g] = -1
 * Group bounds are clamped into [0, n_rows] with end >= start before use, so no group_start reads or writes outside the
 * arrays; a row that no group covers is not written.  The scores of a group pass through its log_posterior slots, so groups
 * that share a row (bounds that decrease) get unspecified values -- every other group keeps its own.  A group's outputs
 * depend only on its own rows in their order: the same bits alone or inside a batch, and from run to run.  One launch, one
 * wavefront (a 64-thread workgroup) per group, no LDS, no atomics, no wait on another workgroup.
 * n_groups == 0 returns 0 without a launch.  PNMN_EINVAL, with no launch and no HIP call: n_groups < 0 or n_rows < 0;
 * num_answers < 1; a null group_start, answers, log_posterior, log_evidence or best_row; a null logits (n_rows > 0); a w_a
 * that is not finite.  num_answers > 1024: PNMN_ESHAPE.  The checks run in this order: the counts and num_answers < 1; then
 * the empty case -- n_groups == 0 returns 0 whatever the pointers and w_a are --; then the pointers and w_a; then the shape.
 *
 * GRADIENT MODE: best_row == NULL and log_answer != NULL.  The marginal-likelihood loss of group g over its candidate
 * programs is -log_evidence[g] = -log sum_r w_r p(a_g | z_r, image)^w_a; this mode computes it together with its gradient
 * with respect to the logits -- a row's cross-entropy gradient scaled by the row's posterior share.  The log_answer slot is
 * then read as d_logits, fp32 [n_rows][num_answers]; log_answer itself is not reported and best_row is not written.
 * log_posterior, log_evidence, row_predictions, support, consistent_count and first_consistent keep their rules and are the
 * same bits as a launch with best_row on the same inputs.  Over a fourth sweep of the group's rows:
 *   d_logits[r][c] = w_a * exp(log_posterior[r]) * (softmax(logits[r])[c] - [c == answers[g]])      for a usable row r
 *                  = d(-log_evidence[g]) / d logits[r][c]; a logit of -inf gets exactly 0
 *   d_logits[r][c] = 0 exactly for every covered row that is not usable -- so for every row of a group without support --,
 *                    and for every covered row when w_a is exactly 0
 * A row that no group covers is not written; the given answer's column is found by comparing c, never by indexing with an
 * unchecked answer.  A group's d_logits rows depend only on its own rows in their order: the same bits alone or inside a
 * batch, and from run to run.  The checks, their order and their codes are those above with "best_row" read as "best_row or
 * (in its absence) log_answer": log_posterior and log_evidence remain required.  No call that was accepted before this
 * mode existed changes its meaning or its bits: every such call passed a best_row, and a call without one was refused
 * with PNMN_EINVAL -- a call with neither best_row nor log_answer still is.  The derivative with respect to log_weight,
 * exp(log_w[r]) - exp(log_posterior[r]), has no slot and is not computed.
 * ------------------------------------------------------------------------------------------- */
int pnmn_answer_posterior(const float* logits /* [n_rows][num_answers] */, const int32_t* valid /* [n_rows], may be NULL */,
                          const float* log_weight /* [n_rows], may be NULL */, const int64_t* answers /* DEVICE [n_groups] */,
                          const int32_t* group_start /* DEVICE [n_groups + 1] */, float w_a,
                          float* log_answer /* [n_rows], may be NULL */, int64_t* row_predictions /* [n_rows], may be NULL */,
                          float* log_posterior /* [n_rows] */, float* log_evidence /* [n_groups] */,
                          int32_t* best_row /* [n_groups] */, int32_t* support /* [n_groups], may be NULL */,
                          int32_t* consistent_count /* [n_groups], may be NULL */,
                          int32_t* first_consistent /* [n_groups], may be NULL */, int n_groups, int n_rows, int num_answers,
                          int unknown_index, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Glue of the seq2seq passes (csrc/seqglue.hip): what the reference -- through AllenNLP 0.9.0 -- does with
 * chains of small tensor ops and per-row Python loops, one launch each.
 *
 * pnmn_token_prep          allennlp.nn.util.add_sentence_boundary_token_ids + get_text_field_mask +
 *                          the index get_final_encoder_states gathers (seq2seq_base.py:97-141 call sites):
 *     full[b] = [bos, tokens[b][0..T), 0],  full[b][1 + n_b] = eos,  n_b = #(tokens[b] != pad)
 *     out = full ([B][T+2]; drop_first = 0) or full[:, 1:] ([B][T+1]; drop_first = 1)
 *     fmask = (out != pad) as float (may be null), last[b] = sum(fmask[b]) - 1 (may be null)
 * pnmn_trim_predictions    seq2seq_base.py:278-293: keep a row up to and including its first `end`; all zeros
 *                          when it starts with `end`; whole when it has none
 * pnmn_mask_last_fwd/bwd   PytorchSeq2SeqWrapper's zeroed padded steps + get_final_encoder_states:
 *     enc = hs * fmask[..., None],  hlast[b] = enc[b][last[b]]  (negative index: from the end)
 *     dhs = (denc + [t == last[b]] dhlast[b]) * fmask        (denc, dhlast may be null)
 * pnmn_length_order        the rows of a pass grouped by length, for the recurrent layer kernels (pnmn_lstm_seq_*_ordered
 *                          below; no reference counterpart other than PytorchSeq2SeqWrapper's sort-and-pack):
 *     steps[b] = clamp(last[b] + 1, 1, T)            (last: what pnmn_token_prep writes)
 *     order [B] = the rows sorted by steps, longest first, equal lengths in row order (a counting sort in one
 *                 workgroup: deterministic, no host synchronisation; T <= 4096)
 *     tile_steps [ceil(B/16)]: tile_steps[i] = max of steps over order[16 i .. 16 i + 15]
 * pnmn_embedding_grad      dw[v] = sum_{rows with token v} dy[row]   (V <= 128, C % 4 == 0; dw is written whole, or --
 *                          accumulate != 0 -- added to;
 *                          rows = (b, t) of tokens [B][T]; shift = 1: row (b, t) takes token (b, t-1) and
 *                          `start` at t = 0; token `skip` contributes nothing; workspace: device memory of
 *                          pnmn_embedding_grad_workspace_bytes(B, T, V) bytes, any contents)
 * pnmn_derive_params       once per optimiser step and model: MFMA-fragment copies of the recurrent weights
 *                          (kind 0: of src [n][k]; kind 1: of its transpose, src stored [k][n]; ld = row
 *                          stride of src) and bias sums (kind 2: dst = src + src2, n floats).
 *                          max_quads = max over jobs of n*k/4 (kinds 0, 1) or n/4 (kind 2).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* src;
    const float* src2;
    float* dst;
    int32_t n, k, ld, kind;
} pnmn_derive_job;

int pnmn_token_prep(const int64_t* tokens, int64_t token_row_stride, int B, int T, int pad, int bos, int eos,
                    int drop_first, int64_t* out, float* fmask, int* last, void* stream);
int pnmn_length_order(const int32_t* last, int B, int T, int32_t* order, int32_t* tile_steps, void* stream);
/* The same lists from the rows' step counts: steps[b] = clamp(steps_in[b], 1, T)  (what pnmn_attn_lstm_fwd_group_stop writes). */
int pnmn_length_order_steps(const int32_t* steps_in, int B, int T, int32_t* order, int32_t* tile_steps, void* stream);
/* A decoder pass's rows for pnmn_length_order: last[b] = max(steps_b, 1) - 1 with steps_b as pnmn_valid_rows (below) defines a
 * decoder segment's, from the same mask tokens (the ones pnmn_seq_nll_fwd is given).  One launch, no atomics, no host
 * synchronisation. */
int pnmn_decoder_last(const int64_t* mask_tokens, int64_t mask_stride, int pad, int rows, int T, int32_t* last, void* stream);
/* The valid (row, step) pairs of padded [rows][T][.] passes as lists of storage rows, for pnmn_gemm_rows.  n <= 8 segments
 * (HOST arrays of n entries each); segment i is a pass of rows[i] sequences of T[i] steps whose sequence b has
 *   steps_b = clamp(last[i][b] + 1, 1, T[i])                                  where last[i] != NULL (an encoder pass:
 *             what pnmn_length_order takes), else
 *   steps_b = 1 + the last t with mask_tokens[i][b * mask_stride[i] + t] != pad[i], 0 when there is none  (a decoder
 *             pass: the last step pnmn_seq_nll_fwd weights, given the same mask tokens -- a pad inside a sampled
 *             program drops no later step).
 * Consecutive segments with the same list[i] are passes stored one behind the other (a decoder's flat buffers): their
 * entries are appended, storage rows counted on from the segments before.  Per list: entries (row, prev) of two int32,
 * row = b T + t for t < steps_b in ascending order, prev = row - 1, or ~b (b counted over the list's segments) at t = 0;
 * *count[i] = their number.  list[i] must hold sum rows x T entries of 8 bytes.  One workgroup per list scans its rows in
 * order: deterministic, no atomics, no host synchronisation. */
int pnmn_valid_rows(const int32_t* const* last /* HOST array */, const int64_t* const* mask_tokens /* HOST array */,
                    const int64_t* mask_stride /* HOST array */, const int32_t* pad /* HOST array */,
                    const int32_t* rows /* HOST array */, const int32_t* T /* HOST array */, int32_t* const* list /* HOST array */,
                    int32_t* const* count /* HOST array */, int n, void* stream);
int pnmn_trim_predictions(const int64_t* raw, int B, int T, int end, int64_t* out, void* stream);
int pnmn_mask_last_fwd(const float* hs, const float* fmask, const int* last, int B, int T, int H, float* enc,
                       float* hlast, void* stream);
int pnmn_mask_last_bwd(const float* denc, const float* dhlast, const float* fmask, const int* last, int B, int T,
                       int H, float* dhs, void* stream);
int64_t pnmn_embedding_grad_workspace_bytes(int B, int T, int V);
int pnmn_embedding_grad(const float* dy, const int64_t* tokens, int64_t token_row_stride, int B, int T, int C,
                        int V, int shift, int start, int skip, int accumulate, float* dw, void* workspace, void* stream);
int pnmn_derive_params(const pnmn_derive_job* jobs, int n_jobs, int max_quads, void* stream);

/* Per-token projection table of an embedding layer (V <= 128 rows; K, N multiples of 16 / 64):
 *   table[v][n] = bias[n] + sum_k emb[v][k] weight[n][k]
 * = F.linear(embedding.weight, W_ih, b_ih + b_hh) of the first encoder layers and of the decoder cell's embedding
 * half (reference modules/seq2seq_base.py:101-141 embeds and projects every (row, step); here the V rows are
 * projected once and pnmn_lstm_seq_fwd / pnmn_attn_lstm_fwd look their step inputs up by token).
 * weight rows are weight_row_stride floats apart (a column slice of the cell's W_ih).  Backward: dtable [V][N] ->
 * demb [V][K] (row padding_idx zeroed; -1 = none), dweight [N][K] (contiguous), dbias [N]; each may be NULL. */
int pnmn_token_table_fwd(const float* emb, const float* weight, int64_t weight_row_stride,
                         const float* bias, int V, int K, int N, float* table, void* stream);
int pnmn_token_table_bwd(const float* dtable, const float* emb, const float* weight,
                         int64_t weight_row_stride, int V, int K, int N, int padding_idx, float* demb,
                         float* dweight, int64_t dweight_row_stride /* 0: K */, float* dbias,
                         float* dbias2 /* second copy of dbias (b_ih and b_hh receive the same) or NULL */, void* stream);

/* Rows of token matrices gathered through an index, concatenated and right-padded into one [sum rows][W] matrix:
 * the index_select / cat / F.pad a training iteration applies to its question / program matrices to form the
 * supervised and unsupervised row subsets (reference question_coding_trainer.py:128-160, joint_training_trainer.py:150-190). */
#define PNMN_TOKEN_SEGS 4
typedef struct pnmn_token_seg {
    const int64_t* src;        /* [.][row_stride] */
    const int64_t* index;      /* [rows] row numbers in src, or NULL: rows 0 .. rows-1 */
    int64_t        row_stride;
    int32_t        rows;
    int32_t        width;      /* columns copied; columns width .. W-1 of the output are `pad` */
} pnmn_token_seg;
int pnmn_token_rows(const pnmn_token_seg* segs /* HOST array */, int n_segs, int64_t* dst, int W, int64_t pad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-sequence masked-mean negative log-likelihood            seq2seq_base.py:235-254 (sampled programs:
 * -sum_t logprob_t mask_t / (sum mask + 1e-12)), :334-341 -> allennlp sequence_cross_entropy_with_logits
 * (average=None, eps 1e-13), program_prior.py:146-151
 *   w[b][t]  = mask_tokens[b][t] != pad
 *   loss[b]  = sum_t w * (logsumexp(logits[b][t]) - logits[b][t][tokens[b][t]]) / (sum_t w + eps)
 *   lse[b][t] (saved for the backward);  dlogits[b][t][k] = dloss[b] * w / (sum w + eps) * (softmax_k - [k == token])
 * Row strides are in elements (logits: between sequences, T*V for a contiguous tensor; tokens / mask_tokens:
 * between rows), so views such as logits[:, :-1] and targets[:, 1:] are passed without a copy.
 * ------------------------------------------------------------------------------------------- */
int pnmn_seq_nll_fwd(const float* logits, int64_t logits_bstride, const int64_t* tokens, int64_t tok_bstride,
                     const int64_t* mask_tokens, int64_t mask_bstride, int pad, float* loss, float* lse,
                     int B, int T, int V, float eps, void* stream);
int pnmn_seq_nll_bwd(const float* logits, int64_t logits_bstride, const int64_t* tokens, int64_t tok_bstride,
                     const int64_t* mask_tokens, int64_t mask_bstride, int pad, const float* lse,
                     const float* dloss, float* dlogits, int64_t dlogits_bstride, int B, int T, int V,
                     float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * REINFORCE / ELBO combination over the sampled rows   elbo.py:28-34 (Reinforce.forward), :61-89
 * (_ElboWithReinforce._forward), :150-160 / :253-270 (the "ours" rewards)
 *   inputs: per-row negative log-likelihoods pg (= -log q), qr (= -log p(x|z)), prior (= -log p(z), or NULL),
 *           nmn (= -log p(a|z,i), or NULL), the moving baseline b (device scalar)
 *   R = -qr - beta * prior + beta * pg - gamma * nmn ;  c = R - b ;  kl = -pg * c + beta * pg ;  elbo = -qr - kl
 *   sums[6] = sum(-qr), sum(kl), sum(elbo), sum(R), sum(nmn), sum(c)   (the caller divides by n, all-reduces
 *             sum(c) for the baseline update b += decay * mean(c))
 *   dpg[n]  = d sum(elbo) / d pg[n] = c[n] - beta   (d / d qr[n] = -1; R is a constant of the estimator)
 * ------------------------------------------------------------------------------------------- */
int pnmn_elbo_rows(const float* pg_loss, const float* qr_loss, const float* prior_loss, const float* nmn_loss,
                   const float* baseline, float beta, float gamma, int n, float* sums, float* dpg, void* stream);

/* The scalar end of a question-coding / joint-training iteration in ONE launch   question_coding_trainer.py:128-165,
 * joint_training_trainer.py:150-191 (with elbo.py as above): the ELBO combination over the n sampled rows, the means
 * of the m supervised rows' cross entropies, the objective
 *     J = w_unsup (gamma mean(nmn) - mean(elbo)) + w_sup alpha (mean(pg_sup) + mean(qr[n..n+m)))
 * and its per-row derivatives (the reference's chain of ~30 scalar torch ops and their autograd nodes).
 *   qr       [n + m]: the reconstructor's per-row losses, sampled rows first, supervised rows behind them
 *   w_*      device scalars (data parallel: n_local * world / n_global) or NULL = 1
 *   baseline device scalar b; update_baseline != 0: b += decay * mean(c) after the rows have read it (a single
 *            process; under data parallelism the caller all-reduces stats[5] = sum(c) and stats[9] = n first)
 *   stats    [10] = mean(-qr), mean(kl), mean(elbo), mean(R), mean(nmn), sum(c), mean(pg_sup), mean(qr_sup), J, n
 *   objective [1] = J again (its own tensor on the autograd side)
 *   d_pg [n], d_qr [n + m], d_nmn [n] (NULL with nmn == NULL), d_pg_sup [m] = dJ / d(row loss)
 *
 * baseline == NULL: the LEAVE-ONE-OUT baseline in the moving one's place (no state: nothing is read or written for it,
 * decay is ignored).  `update_baseline` then holds K, the programs drawn per question, 2 .. 64; the n sampled rows are
 * n / K questions of K rows each, question-major (row i = q K + k), and each sample's reward is centred by the mean reward
 * of the question's OTHER K - 1 samples (Kool et al. 2019, "Buy 4 REINFORCE samples, get a baseline for free"): per
 * question and independent of the sample it centres, so the score-function gradient stays unbiased.  Per row as above
 * but for c:   S_q = sum of the question's R, added in the order k = 0 .. K-1 ;  c_i = R_i - (S_q - R_i) / (K - 1)
 *   stats    [11] = the ten above (stats[5] = sum(c): zero up to rounding) and
 *            stats[10] = reward_variance = mean over questions of sum_k (R_k - S_q / K)^2 / (K - 1)
 *   d_pg [n] = -s (c - beta), d_qr [0..n) = s, d_nmn [n] = s gamma, with the ONE factor s = w_unsup * (1 / n): a row sees
 *            the batch through s alone, so its derivative has the same bits alone and in a batch of any size whenever s is
 *            the same, whichever thread takes its question.  d_qr [n..n+m) and d_pg_sup [m] as above.
 * Its own kernel (the moving baseline is not folded into it); no atomics; every loop is bounded by the arguments; n == 0
 * with m > 0 is a batch without sampled rows.
 *
 * PNMN_EINVAL: a negative count, stats or objective NULL, a NULL row pointer where rows exist (pg, qr, d_pg, d_qr with
 * n > 0; pg_sup, qr, d_pg_sup, d_qr with m > 0), nmn without d_nmn or the reverse; with baseline == NULL also K outside
 * [2, 64] (so every call that was refused for its missing baseline still is: the flag was 0 or 1) and n no multiple of K. */
int pnmn_joint_objective(const float* pg, const float* qr, const float* prior, const float* nmn, const float* pg_sup,
                         float* baseline, const float* w_unsup, const float* w_sup, float alpha, float beta, float gamma,
                         float decay, int update_baseline, int n, int m, float* stats, float* objective, float* d_pg,
                         float* d_qr, float* d_nmn, float* d_pg_sup, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused gradient clamp + Adam (trainers: clamp_(-5,5) then optimizer.step()).
 * module_training_trainer.py:94-96, joint_training_trainer.py:182-188, _trainer.py:103-108,193
 * torch.optim.Adam semantics (no amsgrad): g = clamp(g) + wd*p; m,v EMA; bias correction per
 * item; p -= lr * mhat / (sqrt(vhat) + eps).
 * lr, beta1, beta2, eps, weight_decay and clamp are rounded to float32 on entry and the update is this formula AT THE
 * ROUNDED VALUES, in float32: the weight of g^2 is 1 - (float)beta2 (for 0.999: 0.99998713e-3, where torch rounds 1 - beta2
 * itself: 1.3e-5 of the weight apart -- the same update for a beta2 that differs by 1.3e-8).
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_adam_item {
    float*       param;
    const float* grad;
    float*       exp_avg;
    float*       exp_avg_sq;
    int64_t      n;
    /* bias corrections of THIS parameter's Adam step count s >= 1 (torch.optim.Adam keeps one count per parameter: a
     * module first used at iteration k starts its state there), computed by the caller in double as torch does on the
     * host: bc1 = 1 - beta1^s, bc2_sqrt = sqrt(1 - beta2^s).  One launch serves items of different counts. */
    float        bc1;
    float        bc2_sqrt;
} pnmn_adam_item;         /* 48 bytes */
int pnmn_clamp_adam(const pnmn_adam_item* items, int n_items, double lr, double beta1, double beta2,
                    double eps, double weight_decay, double clamp, void* stream);
/* ... with `blocks_per_item` workgroups walking each item (pnmn_clamp_adam: 2048).  A launch of a few hundred (two per CU)
 * still streams at the HBM rate and leaves wave slots on every CU: the multi-CU recurrent kernels of ANOTHER stream, which
 * need all their workgroups resident before their first step, then start beside it instead of behind it. */
int pnmn_clamp_adam_blocks(const pnmn_adam_item* items, int n_items, double lr, double beta1, double beta2, double eps,
                           double weight_decay, double clamp, int blocks_per_item, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM cell gate math (torch nn.LSTM / nn.LSTMCell, gate order i,f,g,o), the point-wise half of
 * every encoder step (allennlp PytorchSeq2SeqWrapper(nn.LSTM), seq2seq_base.py:145) and decoder
 * step (SimpleSeq2Seq._decoder_cell, seq2seq_base.py:201):
 *   gates[b][4H] = x W_ih^T + b_ih + h W_hh^T + b_hh  (computed by the caller's GEMMs)
 *   c' = sig(f) c + sig(i) tanh(g);  h' = sig(o) tanh(c');  act (optional) keeps the activated gates
 * backward: given dh, dc_in (either may be NULL) -> dgates[b][4H] (wrt the pre-activations), dc_prev.
 * ------------------------------------------------------------------------------------------- */
int pnmn_lstm_cell_fwd(const float* gates, const float* c_prev, float* h, float* c, float* act,
                       int B, int hidden, void* stream);
int pnmn_lstm_cell_bwd(const float* act, const float* c_prev, const float* c, const float* dh,
                       const float* dc_in, float* dgates, float* dc_prev, int B, int hidden,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Persistent LSTM layer over a whole padded sequence (hidden = 256): the recurrent half of
 * nn.LSTM (PytorchSeq2SeqWrapper(nn.LSTM), seq2seq_base.py:145; program_prior.py:117).
 *   forward : gates_t = xp[b][t] + h_{t-1} W_hh^T (xp = X W_ih^T + b_ih + b_hh, all steps, from the
 *             caller's GEMM), zero initial state -> hs[b][t][H], cs[b][t][H], act[b][t][4H]
 *   backward: dhs[b][t][H] (gradient wrt every h_t) -> dgates[b][t][4H] (= gradient wrt xp);
 *             w_hh_t is W_hh transposed ([H][4H]); dW_hh = sum_t dgates_t^T h_{t-1} is the
 *             caller's GEMM over the saved hs.
 * One workgroup owns 16 batch rows for all T steps (h in LDS, c in registers, W_hh streamed).
 * WEIGHT LAYOUT: w_hh / w_hh_t (and w_c, w_hh, w_c_t, w_hh_t of the decoder below) are passed
 * packed in MFMA-fragment order: for W [N][K] row-major,
 *     packed[N/16][K/16][64][4], packed[nt][kb][16*g + li][j] = W[16*nt + li][16*kb + 4*g + j]
 * (one wave-wide operand load = 1 KiB contiguous).
 * `tokens` (pnmn_lstm_seq_fwd; NULL = xp as above): the layer's input is an embedding, xp is the [V][4H]
 * table Emb W_ih^T + b_ih + b_hh and step t of row b uses its row tokens[b * token_stride + t] -- the per-token
 * projection is never materialised per (row, step); dgates is then scattered into the table's gradient with
 * pnmn_embedding_grad.
 * ------------------------------------------------------------------------------------------- */
int pnmn_lstm_seq_fwd(const float* xp, const int64_t* tokens, int64_t token_stride, const float* w_hh,
                      float* hs, float* cs, float* act, int B, int T, int hidden, void* workspace,
                      void* stream);
int pnmn_lstm_seq_bwd(const float* dhs, const float* act, const float* cs, const float* w_hh_t,
                      float* dgates, int B, int T, int hidden, void* workspace, void* stream);
/* Multi-CU variants: with a `workspace` of pnmn_lstm_seq_workspace_bytes(B, backward) bytes (device
 * memory, any contents; 0 bytes = the batch already fills the chip) 4 or 8 workgroups share each
 * 16-row tile, each holding its slice of W_hh in registers and exchanging the recurrent vector through
 * L2 once per step.  Every accumulation keeps the operand order of the workspace == NULL kernels (one
 * workgroup per tile); results agree to the last few ulps (fma contraction of the cell update).  The
 * kernel needs every workgroup resident at once; the library sizes the grid for that.  The hand-off
 * counters of the multi-CU kernels (these and the decoder's) live in a block the library keeps per stream
 * (hipMalloc on a stream's first launch; the kernels leave it zeroed); while the stream is being captured
 * into a graph they go to the head of `workspace` behind a zeroing kernel node instead. */
int64_t pnmn_lstm_seq_workspace_bytes(int B, int backward);
/* Rows grouped by length: the same kernels (with or without a workspace) given pnmn_length_order's `order` and
 * `tile_steps`.  Slot s of the 16-row tiles holds batch row order[s] -- a device-side indirection: every tensor stays
 * in batch order -- and tile i runs tile_steps[i] steps instead of T (forward from step 0, backward from step
 * tile_steps[i] - 1 down), which is where a batch of ragged rows spends its time: the kernels are latency-bound per
 * step.  A row's accumulation order does not depend on the lane or tile that holds it, so for t < steps[b] the
 * outputs are bit for bit those of pnmn_lstm_seq_fwd / _bwd with the same workspace choice.
 * The skipped steps, t in [tile_steps[tile of b], T): hs[b][t] (forward) and dgates[b][t] (backward) are written
 * as zeros -- the mask multiply and the dX / dW / bias products read them; cs and act are left unwritten there (only
 * the backward kernel reads them, and it skips the same steps).
 * CONTRACT (backward): dhs[b][t] for t >= steps[b] is taken as zero, whatever the buffer holds at t >= tile_steps;
 * pnmn_mask_last_bwd and the products of zero dgates rows give exactly that.  Between steps[b] and its tile's count
 * a row is computed as by the unordered kernels (forward: states nobody uses; backward: zeros from zero dhs). */
int pnmn_lstm_seq_fwd_ordered(const float* xp, const int64_t* tokens, int64_t token_stride, const float* w_hh,
                              float* hs, float* cs, float* act, int B, int T, int hidden, const int32_t* order,
                              const int32_t* tile_steps, void* workspace, void* stream);
int pnmn_lstm_seq_bwd_ordered(const float* dhs, const float* act, const float* cs, const float* w_hh_t,
                              float* dgates, int B, int T, int hidden, const int32_t* order,
                              const int32_t* tile_steps, void* workspace, void* stream);
/* Data parallel (replaces nothing in the reference, whose nn.DataParallel is one process:
 * trainers/_trainer.py:94-100): keep `cus` compute units out of the grids of the multi-CU recurrent kernels
 * (these and the decoder's), so that RCCL's workgroups -- resident for a whole collective, waiting for their
 * peers -- never have to share the chip with a grid that needs every CU at once.  A batch whose tiles no longer
 * fit one launch runs as several launches over row ranges.  cus < 0 only queries.  Returns the CU count the
 * multi-CU launches are sized for (<= 0 without a device).  Also settable as PNMN_CLUSTER_RESERVE_CUS. */
int pnmn_cluster_reserve_cus(int cus);

/* ---------------------------------------------------------------------------------------------
 * One decoding step's token choice                                   seq2seq_base.py:203-220
 *   greedy:   tokens[b] = argmax softmax(logits[b])            (first maximum)
 *   sampling: weights = softmax(logits[b]) with pad/unk/start zeroed; tokens[b] ~ weights
 *             (inverse CDF in index order; u from Philox4x32-10 keyed by `seed`, counter =
 *             (row_offset + b, step) -- shard-invariant under data parallelism)
 *   logprobs[b] = log_softmax(logits[b])[tokens[b]]            (unmodified distribution)
 * V <= 512.
 * Token choice is always an index in [0, V), also for rows that are not all finite (the same rule in the decoder kernels):
 *   greedy:   torch.argmax semantics -- a NaN counts as the maximum, the first index wins.
 *   sampling, no NaN or +inf in the row but the allowed weights underflow to a total of 0: the weights are recomputed
 *             relative to the largest allowed logit (the same distribution without the underflow).
 *   sampling, a NaN or +inf in the row, or every allowed logit -inf: the first allowed index with the largest logit,
 *             a NaN counting as the largest; logprobs stays log_softmax(logits[b])[tokens[b]] (NaN propagates).
 *   no allowed token (V <= 3, pad / unk / start cover the row): the greedy choice.
 * A finite row with a positive allowed total never reaches these rules (its draw does not change).
 *
 * The filter rule: temperature, top-k and nucleus (top-p) truncation of the distribution a token is drawn from.
 * A filter is (temperature, top_k, top_p); (1, 0, 1) is the identity.  It applies to sampling only: a greedy choice and
 * a teacher-forced pass ignore it.  For one row of logits z[0..V):
 *   A      = every index but pad, unk and start (the allowed set, as above)
 *   s_j    = z_j / temperature, w_j = exp(s_j - max_A s)                                  for j in A
 *   rank   j ranks before i when w_j > w_i, or w_j == w_i and j < i                       (within A)
 *   top_k > 0: keep the top_k first-ranked indices (top_k >= |A| keeps all of A)
 *   top_p < 1: of those, keep i iff the summed weight of the kept indices ranked before i is < top_p * total, total = the
 *              weight top-k kept; the first-ranked index is always kept
 *   draw   inverse CDF in INDEX order over the kept weights, from the uniform pnmn_sample_tokens draws: Philox4x32-10,
 *          counter (row_offset + row, step) -- a filtered and an unfiltered decode from one seed share their random numbers
 *   logprobs (and any loss built from them) stay log_softmax(z)[token] of the UNMODIFIED distribution, as the reference
 *          already scores a draw from which pad / unk / start were removed (seq2seq_base.py:204,220)
 * A row that holds a NaN or +inf, or whose allowed weights sum to 0 in the unfiltered rule, follows that rule's fallback
 * unchanged and ignores the filter; a token is always in [0, V).  With the identity filter, as with a null one, an entry
 * point runs its unfiltered kernel: the same output, bit for bit.  It returns PNMN_EINVAL and launches nothing for a
 * temperature that is not finite or <= 0, top_k < 0, or a top_p outside (0, 1] (NaN included), also where the filter
 * would be ignored.  The filters are HOST memory, read before the call returns, and travel by value in the launch
 * arguments: no device allocation, no copy, no synchronisation.
 * pnmn_attn_lstm_fwd_group: filters[i] belongs to jobs[i] and applies when that job's sample == 1; for any other job it
 * is checked and ignored.
 * ------------------------------------------------------------------------------------------- */
struct pnmn_sampling_filter {
    float temperature;
    int32_t top_k;
    float top_p;
    int32_t reserved;
};                         /* 16 bytes; a host argument block (see the declaration conventions), not a work-item record */
int pnmn_sample_tokens(const float* logits, int64_t* tokens, float* logprobs, int B, int V,
                       int greedy, uint64_t seed, uint64_t row_offset, uint32_t step, int pad_index,
                       int unk_index, int start_index, const struct pnmn_sampling_filter* filter /* HOST, may be NULL */,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Persistent attention-LSTM decoder (hidden = 256): the whole decoding loop of
 * Seq2SeqBase._forward_loop (seq2seq_base.py:186-224 -> allennlp _prepare_output_projections) in one
 * launch; one workgroup owns 16 batch rows for all T steps.
 *   per step: w = masked_softmax(enc . h, mask); ctx = w . enc; gates = xe_t + ctx W_c^T + h W_hh^T;
 *             LSTM cell; [sample != 0: logits = h W_p^T + b_p, token choice, next xe from etable]
 *   W_ih of the reference's LSTMCell is [W_c | W_e] (input = cat(ctx, embedding)); xe / etable carry
 *   the embedding half plus both biases.  sample: 0 teacher forced (xe; or xe == NULL and step t's
 *   input taken as row in_tokens[b * in_token_stride + t] of etable), 1 sample, 2 greedy: the token choice of
 *   pnmn_sample_tokens (same Philox stream, counter (row_offset + b, t); same rule for rows that are not all finite,
 *   so a token is always in [0, V)).
 *   saved for backward: act, cs, hs, ctx, probs (softmax before masking).
 * backward: dhs (gradient wrt every h_t) -> dgates (= d xe), denc (+=, zero on entry), dh0.
 * S <= 64 encoder positions, V <= 128 sampled vocabulary.
 * One forward pass = one pnmn_decoder_fwd_job record, its fields named as above; pnmn_attn_lstm_fwd takes ONE record in
 * HOST memory, pnmn_attn_lstm_fwd_group (below) an array of them.  `filter` (may be NULL) applies to a sample == 1 pass by
 * the filter rule beside pnmn_sample_tokens; it is checked whatever the mode.  B <= 0 or T <= 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_decoder_fwd_job {
    const float *xe, *etable, *enc, *mask, *h0, *w_c, *w_hh, *w_p, *b_p;
    float *hs, *cs, *act, *ctx, *probs;
    int64_t* tokens;
    const int64_t* in_tokens;
    int64_t in_token_stride;
    uint64_t seed, row_offset;
    int32_t B, T, S, V, sample, pad_index, unk_index, start_index;
} pnmn_decoder_fwd_job;    /* 184 bytes */
/* The automaton rule: sampling and greedy decoding under a token automaton.  The free-running modes of pnmn_attn_lstm_fwd /
 * _fwd_group emit only strings the automaton accepts.  A constrained draw is not a draw from the model's distribution q
 * but from q_c, q renormalised over A_c step by step: a loss on such tokens is scored under q_c (pnmn_grammar_logits,
 * include/probnmn_grammar.h, masks the logits to the same sets), never under the logprobs below.  The tables (token_class, next_state, min_left, n_states, n_classes, state 0 = start,
 * 255 = no completion) and the test of a candidate are those of pnmn_attn_lstm_beam below: HOST pointers, every entry checked,
 * passed by value in the launch arguments and staged into LDS once per workgroup -- no device allocation, no copy, no
 * synchronisation.
 * Every row carries an automaton state (0 at the start) and a finished flag (false at the start).  At step t (0-based) of T a
 * row in state s that has not finished has the allowed set A_c(s, t):
 *   token v, not pad / unk / start and v != end_index   iff  min_left[next_state[s][token_class[v]]] <= T - 1 - t
 *   end_index                                           iff  min_left[s] == 0
 * and its token is chosen as by pnmn_sample_tokens, with or without a filter, with A_c in the place of A:
 *   sample == 1: inverse CDF in index order over softmax(z) restricted to A_c, the uniform from the same Philox counter
 *                (row_offset + row, t) -- a constrained and an unconstrained decode from one seed share their random numbers;
 *                under a filter other than the identity: rank, top-k and top-p WITHIN A_c, then the same draw
 *   sample == 2: the first index of the largest logit WITHIN A_c (the unconstrained arg-max looks at all of [0, V))
 *   a row that holds a NaN or +inf (greedy: a NaN), or whose A_c weights sum to 0, follows the fallback rule stated beside
 *                pnmn_sample_tokens with A_c as the allowed set (greedy: the arg-max of that rule within A_c): still in A_c
 *   a row that has emitted end_index is finished: every later step of it emits end_index, its state is frozen, and the token
 *                is fed to the next step as usual
 *   state:       unchanged on end_index, otherwise s <- next_state[s][token_class[token]]
 * By induction min_left[s] <= T - t before every step, so A_c is never empty, and every row, cut at its first end_index, is
 * accepted by the automaton.  With one state, one class and min_left = {0} a sampling pass emits what the unconstrained pass
 * emits up to and including each row's first end_index.  logprobs, and the loss the inference decodes report, stay
 * log_softmax(z)[token] of the UNMODIFIED distribution, exactly as for the filtered draw; the trainers that sample under the
 * automaton take log_softmax over A_c instead (pnmn_grammar_logits), which is the distribution of the unfiltered draw.
 * A filter (null or the identity: the unfiltered draw) applies to sample == 1 within A_c, as stated.
 * pnmn_attn_lstm_fwd_group: the automaton applies to every job with sample != 0, which share one vocabulary size V; for a job
 * with sample == 0 it is checked as far as it can be without a vocabulary, and ignored.
 * A call with tables returns PNMN_EINVAL and launches nothing for: some but not all of the tables, a table entry out of range
 * (token_class[v] >= n_classes for v < V, next_state >= n_states), n_states outside 1..PNMN_BEAM_MAX_STATES, n_classes outside
 * 1..PNMN_BEAM_MAX_CLASSES, V outside 1..128, end_index outside [0, V), min_left[0] > T (no accepted string fits; group: any
 * free-running job's T), an invalid filter.  Otherwise: the arguments, limits and return codes of the call without tables. */
int pnmn_attn_lstm_fwd(const pnmn_decoder_fwd_job* job /* HOST, one record */, int hidden,
                       const struct pnmn_sampling_filter* filter /* HOST, may be NULL */, int end_index,
                       const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                       const uint8_t* min_left /* HOST */, int n_states, int n_classes, void* stream);
int pnmn_attn_lstm_bwd(const float* dhs, const float* act, const float* cs, const float* hs,
                       const float* ctx, const float* probs, const float* enc, const float* mask,
                       const float* h0, const float* w_c_t, const float* w_hh_t, float* dgates,
                       float* denc, float* dh0, int B, int T, int S, int hidden, void* stream);

/* Beam-search decoding with the same per-step arithmetic (decoder_beam.hip): inference only, nothing saved, no backward.
 * One workgroup owns 16 / beam questions x beam hypotheses for all T steps.  enc [B][S][H], mask [B][S] and h0 [B][H] are
 * per QUESTION (never repeated per hypothesis); etable / w_c / w_hh / w_p / b_p as for pnmn_attn_lstm_fwd (w_c, w_hh in
 * fragment order).  Selection rule, per question b:
 *   score[b][0] = 0, score[b][k>0] = -inf, last[b][k] = start_index                 (step 0 expands one state)
 *   each step: logp[k][v] = log_softmax(h_k W_p^T + b_p)[v]; logp[k][pad|unk|start] = -inf;
 *              last[b][k] == end_index: logp[k][:] = -inf, logp[k][end] = 0         (a finished hypothesis keeps its score)
 *              cand[k*V+v] = score[b][k] + logp[k][v]                               (a non-finite cand counts as -inf)
 *              new beams = the `beam` largest cand, best first; equal cand: the smaller k*V+v first;
 *              a slot left without a finite candidate: token end_index, back-pointer 0, score -inf
 *   Scores are plain sums of log-probabilities (fp32).  The survivors' h, c and last token follow the back-pointers.
 * outputs: tokens [B][beam][T] (back-tracked, best first, every token in [0, V), @end@ after a hypothesis's first @end@),
 *          scores [B][beam]; optional trace of every step, [B][T][beam] each (all three or none): the token, the
 *          back-pointer (slot of the previous step) and the running score of every slot.
 * Limits: hidden = 256, 1 <= S <= 64, 1 <= V <= 128, T <= 64, beam in {1, 2, 4, 8, 16}, start / end index inside [0, V);
 * anything else (or a missing pointer) returns PNMN_EINVAL.
 *
 * The beam-automaton rule: with the three tables given, only hypotheses the automaton accepts leave the decoder.
 *   token_class [V]                    class of every target token, each < n_classes
 *   next_state  [n_states][n_classes]  each < n_states; state 0 is the start state
 *   min_left    [n_states]             fewest further tokens from the state to an accepting one: 0 = accepting,
 *                                      255 = no completion exists
 * The three tables are HOST pointers; every entry is checked, and they travel by value in the launch arguments (no device
 * allocation, no copy, no synchronisation; the caller's arrays are free again when the call returns).  Every slot carries
 * a state, state[b][k] = 0 at the start.  The selection rule above changes at the candidates only; at step t (0-based) a
 * hypothesis k that has not finished, in state s, offers
 *   token v (not pad / unk / start, v != end)  only if  min_left[next_state[s][token_class[v]]] <= T - 1 - t
 *   end_index                                  only if  min_left[s] == 0
 * and every other candidate of it is -inf; a finished hypothesis offers only end_index at its own score, as above.
 * A survivor's state is the one reached from its parent's (by back-pointer) on its token; on end_index, the parent's.
 * Selection, ties, the slot without a finite candidate, the back-track and the trace are the unconstrained ones.
 * Consequence: every hypothesis with a finite score, cut at its first end_index, is accepted by the automaton; when
 * min_left[0] <= T, slot 0 of every question is finite.  With one state, one class and min_left = {0} the call computes
 * what it computes without tables, bit for bit.
 * Limits with tables: 1 <= n_states <= 32, 1 <= n_classes <= 16; some but not all of the tables, or an entry out of range,
 * returns PNMN_EINVAL. */
#define PNMN_BEAM_MAX_STATES 32
#define PNMN_BEAM_MAX_CLASSES 16
int pnmn_attn_lstm_beam(const float* etable, const float* enc, const float* mask, const float* h0,
                        const float* w_c, const float* w_hh, const float* w_p, const float* b_p,
                        int64_t* tokens, float* scores, int32_t* trace_tokens, int32_t* trace_backptr,
                        float* trace_scores, int B, int T, int S, int V, int hidden, int beam,
                        int pad_index, int unk_index, int start_index, int end_index,
                        const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                        const uint8_t* min_left /* HOST */, int n_states, int n_classes, void* stream);

/* Stochastic beam search (Kool, van Hoof and Welling, ICML 2019) on the same kernel (its second candidate stage): the `beam`
 * hypotheses of a question are an exact sample WITHOUT replacement from the decoder's sequence distribution, in the order a
 * sequential sample would draw them.  Every argument up to n_classes means what it means for pnmn_attn_lstm_beam; attention,
 * gates, cell, logits, selection order, gather, early stop, back-track and the automaton rule are that call's.  Every slot
 * carries phi (its log-probability, returned in `scores`) and G (its perturbed value).  Per question b:
 *   phi[b][0] = G[b][0] = 0, phi[b][k>0] = G[b][k>0] = -inf, last[b][k] = start_index
 *   each step t, hypothesis k that has not finished:
 *     offered tokens    exactly those pnmn_attn_lstm_beam offers (never pad / unk / start; with tables, the automaton rule)
 *     lse               log-sum-exp of the logits of the offered tokens whose logit is finite
 *     phi(k,v)        = phi[b][k] + logit[k][v] - lse         (the softmax RESTRICTED to the offered tokens: the distribution
 *                                                              the (constrained) sampling decode draws from)
 *     u(k,v)          = (2 * (x0 >> 9) + 1) * 2^-24, x0 = word 0 of Philox4x32-10 with counter {row lo, row hi, t, 0x9E3779B9}
 *                       and key {seed lo, seed hi} (the generator of pnmn_sample_tokens),
 *                       row = ((question_offset + b) * 16 + k) * 128 + v: a draw depends on neither beam, V nor the batch
 *     g(k,v)          = phi(k,v) - log(-log u(k,v));  Z = max of g(k,.) over the candidates with a finite phi
 *     w               = G[b][k] - g(k,v) + log(1 - exp(g(k,v) - Z))
 *     G~(k,v)         = G[b][k] - max(0, w) - log1p(exp(-|w|))           (the arg-max child: w = -inf, G~ = G[b][k])
 *   a finished hypothesis offers only end_index, with phi and G unchanged; no uniform is drawn for it
 *   a candidate whose phi or G~ is not finite counts as -inf
 *   new beams = the `beam` largest G~, best first; equal G~: the smaller k*V+v first; a survivor takes phi(k,v) and G~(k,v);
 *   a slot left without a finite candidate: token end_index, back-pointer 0, phi = G = -inf
 * outputs: tokens, scores (= phi) and the three traces as pnmn_attn_lstm_beam; perturbed [B][beam] = G of every returned
 * hypothesis; trace_perturbed [B][T][beam] = G of every slot at every step, given exactly when the three traces are.
 * Checks and limits are those of pnmn_attn_lstm_beam; in addition a NULL `perturbed`, question_offset < 0, or some but not
 * all of the four traces returns PNMN_EINVAL. */
int pnmn_attn_lstm_beam_stochastic(const float* etable, const float* enc, const float* mask, const float* h0,
                                   const float* w_c, const float* w_hh, const float* w_p, const float* b_p,
                                   int64_t* tokens, float* scores, int32_t* trace_tokens, int32_t* trace_backptr,
                                   float* trace_scores, int B, int T, int S, int V, int hidden, int beam,
                                   int pad_index, int unk_index, int start_index, int end_index,
                                   const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                                   const uint8_t* min_left /* HOST */, int n_states, int n_classes,
                                   float* perturbed, float* trace_perturbed, uint64_t seed, int64_t question_offset,
                                   void* stream);

/* Multi-CU variants of pnmn_attn_lstm_fwd / _bwd (decoder_multi.hip): eight workgroups per 16-row tile,
 * each keeping its rows' encoder outputs in LDS and its slices of W_c / W_hh in registers, two L2
 * hand-offs per step.  A job = the arguments and saved tensors of pnmn_attn_lstm_fwd / _bwd for one pass; every call
 * also takes a device `workspace` of pnmn_attn_lstm_group_workspace_bytes(rows, n, backward) bytes, rows[i] = B of
 * job i (n = 1: 0 = device too small, use pnmn_attn_lstm_fwd / _bwd).
 * The backward emits dctx [B,T,H] (gradient wrt every context vector) and dscore [B,T,S] (gradient
 * wrt the attention scores) instead of accumulating denc; the caller forms
 *     denc = w^T dctx + dscore^T h_prev      (two GEMMs per row over the T steps; w = the masked, renormalised
 *                                             attention weights, which the kernel writes to `weights` [B,T,S])
 * Sums over source positions / gate columns are associated differently from the one-workgroup
 * kernels: results agree to fp32 round-off, not bit for bit.
 *
 * `jobs` is an array of n INDEPENDENT passes (forward n = 1..2, backward n = 1..3) that go out side by side in ONE
 * launch.  These kernels are bound by their per-step hand-off latency, so passes that fit the chip together take as
 * long as the longest instead of the sum.  Forward: a training iteration's teacher-forced decodes, the reconstructor
 * over the questions and the generator over the supervised programs (question_coding_trainer.py:128-160,
 * joint_training_trainer.py:150-190 call them one after the other).  Backward: those two and the generator's decode of
 * the sampled programs (the samples are discrete, no gradient flows from the reconstruction back into the generator).
 * Fit: every job has B > 0 and T > 0 and the jobs' tiles, each job rounded up to whole groups of 8 tiles, are resident
 * together (512 rows on 256 CUs, at most 128 tiles).  Jobs that do not fit go out as the first n - 1 by the same rule,
 * then the last alone (identical results): three -> pair + single, pair -> single, single.  A single job beyond what
 * fits the chip at once runs as successive launches over its rows; one with B <= 0 or T <= 0 is skipped.
 * n out of range or a missing jobs / workspace pointer returns PNMN_EINVAL (the workspace query: 0).
 * Forward options: `filters` (HOST, one per job, or NULL: none) by the filter rule beside pnmn_sample_tokens, the tables by
 * the automaton rule beside pnmn_attn_lstm_fwd.  Neither changes the fit and fall-back rule. */
typedef struct pnmn_decoder_bwd_job {
    const float *dhs, *act, *cs, *hs, *probs, *enc, *mask, *h0, *w_c_t, *w_hh_t;
    float *dgates, *dctx, *dscore, *weights, *dh0;
    int32_t B, T, S, reserved;
} pnmn_decoder_bwd_job;    /* 136 bytes */
int64_t pnmn_attn_lstm_group_workspace_bytes(const int32_t* rows, int n, int backward);
int pnmn_attn_lstm_fwd_group(const pnmn_decoder_fwd_job* jobs, const struct pnmn_sampling_filter* filters /* HOST, may be NULL */,
                             int end_index, const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                             const uint8_t* min_left /* HOST */, int n_states, int n_classes,
                             int n, int hidden, void* workspace, void* stream);
int pnmn_attn_lstm_bwd_group(const pnmn_decoder_bwd_job* jobs, int n, int hidden, void* workspace, void* stream);
/* Rows grouped by length: the same calls given, per job, pnmn_length_order's `order` [B] and `tile_steps` [ceil(B/16)] (device
 * int32, with the meaning they have in pnmn_lstm_seq_fwd_ordered) of the steps pnmn_decoder_last counts.  `order` and
 * `tile_steps` are HOST arrays of n device pointers (or both NULL); entry i belongs to job i, both NULL = the job runs as in the
 * calls above, which forward here with NULLs.  For a job with an order
 *   - slot s of 16-row tile k addresses batch row order[16 k + s] in EVERY tensor of the job; nothing is permuted in memory,
 *     and a (row, step) the tile runs holds the bits the call without an order writes there;
 *   - tile k runs tile_steps[k] steps (clamped to [1, T]): forward t = 0 .. tile_steps[k] - 1, backward from there down to 0
 *     with zero d h / d c carried in;
 *   - from tile_steps[k] on, the tile's rows hold ZEROS in what later calls read over all T steps: forward hs and ctx,
 *     backward dgates, dctx, dscore and weights.  cs, act and probs, which only the backward of the same order reads, are
 *     left unwritten there;
 *   - backward contract, as for pnmn_lstm_seq_bwd_ordered: dhs[b][t] is not read for t >= tile_steps, and must be exactly
 *     zero for t >= the row's own steps (pnmn_seq_nll_bwd writes zeros there) -- then dgates, dctx, dscore and dh0 are what
 *     the call without an order computes at every step the row has, and zero behind it;
 *   - the job goes out in launches of its own (a group that holds one falls back like a group that does not fit); cut into
 *     row ranges, a range from slot r0 takes order + r0 and tile_steps + r0 / 16 and the job's own base pointers.
 * An index in `order` is held inside [0, B).  A free-running job (sample != 0) given an order, one list without the other,
 * or hidden / S outside the limits above with an order, returns PNMN_EINVAL. */
int pnmn_attn_lstm_fwd_group_ordered(const pnmn_decoder_fwd_job* jobs, const struct pnmn_sampling_filter* filters /* HOST, may be NULL */,
                                     int end_index, const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                                     const uint8_t* min_left /* HOST */, int n_states, int n_classes, int n, int hidden,
                                     const int32_t* const* order /* HOST array, may be NULL */,
                                     const int32_t* const* tile_steps /* HOST array, may be NULL */, void* workspace, void* stream);
int pnmn_attn_lstm_bwd_group_ordered(const pnmn_decoder_bwd_job* jobs, int n, int hidden,
                                     const int32_t* const* order /* HOST array, may be NULL */,
                                     const int32_t* const* tile_steps /* HOST array, may be NULL */, void* workspace, void* stream);
/* Free-running tiles that stop: the forward call given, per job, `steps_out` [B] (device int32; a HOST array of n device pointers
 * as `order` is, or NULL; entry i belongs to job i, NULL = the job runs as in pnmn_attn_lstm_fwd_group_ordered, which forwards
 * here with NULL).  A job with steps_out must be free running (sample != 0) with end_index inside [0, V), and then
 *   - a row that has chosen end_index chooses end_index at every later step (the finished row of the automaton rule), and
 *     steps_out[b] = 1 + the step of row b's first end_index, T when it has none;
 *   - a 16-row tile leaves its step loop behind the step at which the last of its rows has chosen end_index; which step that
 *     is, every workgroup of the tile decides for itself from the tokens it has drawn itself -- the same tokens in all of
 *     them, as they always were -- so no exchange is added;
 *   - up to and including its first end_index (t < steps_out[b]) a row's tokens, hs, cs, act, ctx and probs are the bits the
 *     call without steps_out writes there; between there and its tile's last step they are those of a row fed end_index;
 *   - from its tile's last step on, a row holds end_index in tokens and ZEROS in hs, ctx (read by later calls over all T), cs,
 *     act and probs (which a backward whose rows are grouped by steps_out may read at a step the row's tile here never ran:
 *     there every gradient is 0 x these values, and with probs = 0 the attention's renormalisation stays finite);
 *   - the job goes out in launches of its own, as a job with an order does; cut into row ranges, a range from row r0 takes
 *     steps_out + r0.
 * With steps_out - 1 as pnmn_length_order's `last` (pnmn_length_order_steps takes steps_out itself), the lists serve
 * pnmn_attn_lstm_bwd_group_ordered for that job: its contract holds when dhs is zero from steps_out[b] on, as the loss over the
 * trimmed samples makes it.  A teacher-forced job given steps_out, end_index outside [0, V), an automaton table or a
 * non-identity filter of the job beside steps_out returns PNMN_EINVAL. */
int pnmn_attn_lstm_fwd_group_stop(const pnmn_decoder_fwd_job* jobs, const struct pnmn_sampling_filter* filters /* HOST, may be NULL */,
                                  int end_index, const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                                  const uint8_t* min_left /* HOST */, int n_states, int n_classes, int n, int hidden,
                                  const int32_t* const* order /* HOST array, may be NULL */,
                                  const int32_t* const* tile_steps /* HOST array, may be NULL */,
                                  int32_t* const* steps_out /* HOST array, may be NULL */, void* workspace, void* stream);
/* The encoder-output gradient from what pnmn_attn_lstm_bwd_group emits, in one bandwidth-bound launch instead of two
 * strided-batched library GEMMs of B tiny [S x T].[T x 256] products (allennlp SimpleSeq2Seq._prepare_attended_input /
 * DotProductAttention under autograd; seq2seq_base.py:201):
 *   denc[b][s][:] = sum_t weights[b][t][s] * dctx[b][t][:] + dscore[b][t][s] * h_{t-1}[b][:]   (h_{-1} = h0)
 * hidden = 256, T <= 64. */
int pnmn_attn_denc(const float* weights, const float* dscore, const float* dctx, const float* hs, const float* h0,
                   float* denc, int B, int T, int S, int hidden, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Free-running samples from the program prior p(z), all T steps in one launch       program_prior.py:174-301
 * Per row, with (h0, c0, h1, c1) = 0 and last = start_index, step t = 0 .. T-1 is
 *   g0 = table0[last] + h0 W_hh0^T, then the LSTM cell (gate order i, f, g, o)  -> h0', c0'
 *        table0 [V][4H] = Emb W_ih0^T + b_ih0 + b_hh0: the per-token table of pnmn_token_table_fwd
 *   g1 = b1 + h0' W_ih1^T + h1 W_hh1^T, then the cell                           -> h1', c1'      (b1 = b_ih1 + b_hh1)
 *   p  = h1' W_proj^T  (256 wide),   z = p W_out^T  (W_out [V][256] row major: the tied embedding, no bias)
 *   tokens[b][t]:  mode 1  the draw of pnmn_sample_tokens from z, Philox counter (row_offset + b, t)
 *                  mode 2  its first arg-max
 *                  mode 0  in_tokens[b * in_token_stride + t] in the place of the choice (clamped into [0, V))
 *   logprob_vocab[b][t] = log_softmax(z)[token]      (the UNMODIFIED distribution, whatever filter or automaton chose)
 *   logprob_proj[b][t]  = log_softmax(p)[token]      (over all 256 entries of p: the reference's own quirk, :243-244)
 *   proj[b][t][0..256) = p  when `proj` is not null;   last = token
 * A row keeps running after end_index, as the reference's loop does; the caller trims.
 * w_hh0, w_ih1, w_hh1 ([1024][256]) and w_proj ([256][256]) are in MFMA fragment order (see pnmn_lstm_seq_fwd).
 * `filter` (HOST, may be null = the identity) applies to mode 1 only, by the rule beside pnmn_sample_tokens.  The
 * automaton tables (HOST; all three null = unconstrained) apply to modes 1 and 2 by the rule beside
 * pnmn_attn_lstm_fwd: A_c in the place of the allowed set, a finished row emits end_index, its state frozen; mode 0
 * checks them as far as it can without a vocabulary and ignores them.  The non-finite fallbacks of pnmn_sample_tokens apply,
 * so a token is always in [0, V).  With the identity filter and no automaton the plain kernel runs: the same output, bit for
 * bit, as with filter = null.
 * One workgroup owns 16 rows for all T steps; rows are independent, so a batch of any size is a plain grid of ceil(B / 16)
 * workgroups: no workspace, no counters, no co-residency.
 * Returns PNMN_EINVAL and launches nothing for: hidden != 256, V outside 1..128, T < 1, B < 0, mode outside 0..2, start_index
 * outside [0, V), mode 0 without in_tokens, a null required pointer (everything but proj, in_tokens, filter and the tables), an
 * invalid filter, some but not all of the tables, and whatever pnmn_attn_lstm_fwd refuses in its tables (min_left[0] > T
 * included).  B == 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------------- */
int pnmn_prior_sample(const float* table0, const float* w_hh0, const float* w_ih1, const float* w_hh1, const float* b1,
                      const float* w_proj, const float* w_out,
                      int64_t* tokens, float* logprob_vocab, float* logprob_proj, float* proj /* optional */,
                      int B, int T, int V, int hidden, int mode, int pad_index, int unk_index, int start_index,
                      uint64_t seed, uint64_t row_offset, const int64_t* in_tokens, int64_t in_token_stride,
                      const struct pnmn_sampling_filter* filter /* HOST, may be NULL = identity */, int end_index,
                      const uint8_t* token_class /* HOST */, const uint8_t* next_state /* HOST */,
                      const uint8_t* min_left /* HOST */, int n_states, int n_classes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Host-side launch sequencer (no device work of its own): `list` is a HOST array; entry i calls the entry
 * point named by `op` with (a, b, c, n, p[...]) in that entry point's argument order (pointers first, then
 * the item count, then the integer arguments), all on `stream`; stops at the first non-zero return code.
 * Replaces ~160 one-by-one calls per step of the per-example interpreter loop (nmn.py:197-238) with two.
 *   CONV  a items, n, p = H, W, cin_chunks, ntaps, in_stride, out_stride, cout_blocks, relu; c = CU budget (0 = all)
 *   WGRAD a items, b jobs, n = n_jobs, p = H, W, ntaps, cin_blocks, cout_blocks, x_stride, dy_stride, CU budget (0 = none)
 *   TRANSPOSE_WEIGHTS a items, n      DOT_* / SAME_* / MASK_BWD a items, n, p = HW      MINMAX_* p = HW, C
 *   MAXPOOL_FWD a in, b out, n, p = H, W, C       MAXPOOL_BWD a in, b dout, c din, n, p = H, W, C
 *   NCHW_TO_NHWC a src, b dst, n, p = C, HW
 * ------------------------------------------------------------------------------------------- */
#define PNMN_OP_CONV              0
#define PNMN_OP_WGRAD             1
#define PNMN_OP_TRANSPOSE_WEIGHTS 2
#define PNMN_OP_DOT_FWD           3
#define PNMN_OP_DOT_BWD           4
#define PNMN_OP_SAME_FWD          5
#define PNMN_OP_SAME_BWD          6
#define PNMN_OP_MINMAX_FWD        7
#define PNMN_OP_MINMAX_BWD        8
#define PNMN_OP_MASK_BWD          9
#define PNMN_OP_MAXPOOL_FWD       10
#define PNMN_OP_MAXPOOL_BWD       11
#define PNMN_OP_NCHW_TO_NHWC      12
#define PNMN_OP_SET_ROWS          13   /* a items, n                                      (pnmn_set_rows) */
#define PNMN_OP_ACCUMULATE        14   /* a items, n                                      (pnmn_accumulate) */
#define PNMN_OP_ZERO              15   /* a device pointer, b = byte count (as a pointer-sized integer): hipMemsetAsync */
#define PNMN_OP_FEAT_GATHER       16   /* a items, b gfeat, n = n_items, p = n_examples, HW   (pnmn_feat_grad_gather) */
typedef struct pnmn_launch {
    const void* a;
    const void* b;
    const void* c;
    int32_t     op;
    int32_t     n;
    int32_t     p[8];
} pnmn_launch;             /* 64 bytes */
int pnmn_run_launches(const pnmn_launch* list, int n, void* stream);

/* Launch trace (measurement only: bench.py's roofline passes, scripts/conv_launch_table.py).  Between _begin and _end
 * every CONV / WGRAD entry that pnmn_run_launches issues -- the trunk planner's lists included, i.e. the SHIPPED host
 * path -- is bracketed by two events on its stream.  _end waits for them and reports, per traced entry in issue order,
 * the launch duration and the algorithmic work of the call (the call's items are copied to the host
 * in stream order in front of the launch -- outside the bracket -- since a step re-uses its record buffers).  Returns PNMN_EAGAIN when more than `capacity` entries were traced (*n_out = how many; the trace is KEPT: call again with room for them -- it is dropped by a successful _end or the next _begin).  The reference has
 * no counterpart: its per-module timing is whatever torch.profiler shows around nmn.py:191-241. */
typedef struct pnmn_launch_timing {
    int32_t op, n;          /* PNMN_OP_CONV / PNMN_OP_WGRAD; items (CONV) or jobs (WGRAD) of the call */
    int32_t p[8];           /* the entry's parameters */
    int32_t n_items;        /* items of the call (WGRAD: over all jobs) */
    float   ms;             /* launch duration */
    double  flops, bytes;   /* algorithmic FLOPs and HBM bytes */
} pnmn_launch_timing;      /* 64 bytes */
int pnmn_launch_trace_begin(void);
int pnmn_launch_trace_end(pnmn_launch_timing* out, int capacity, int* n_out);

/* ---------------------------------------------------------------------------------------------
 * Trunk planner: sampled programs -> launched module programs in ONE call (host side; replaces the per-example
 * interpreter loop nmn.py:191-241 together with the Python half of the scheduler that used to sit between the
 * sampling decode and the first module launch of a joint-training step: joint_training_trainer.py:150-166).
 *
 *   create   per network: token kinds (program_compiler.classify_token), per-token weight offset tables (floats
 *            into the parameter / gradient / transposed-weight arenas; -1 = none), map size.
 *   plan_and_launch
 *            programs (HOST int64 [n][length]) -> compiled (cache keyed by the token row) -> structure templates
 *            (cache keyed by the call structure: primitives, dependency levels, arena offsets) -> pnmn_plan_batch
 *            straight into page-locked staging -> one H2D copy into a device buffer the planner owns -> the forward
 *            launch list (SET_ROWS for invalid / feature-result programs, the level-ordered grouped launches,
 *            `fwd_tail`) issued on `stream`; the backward list (`bwd_head`, ZERO of the gradient arena block,
 *            ACCUMULATE for feature-result programs, levels in reverse, deferred weight gradients, `bwd_tail`) is
 *            written to `bwd` for pnmn_run_launches once d(pooled) exists.  `bwd_piece_cut` = number of leading
 *            entries of `bwd` after which every module / classifier-conv gradient has been queued (data parallel:
 *            that range of the gradient arena may start its all-reduce).
 *            Returns PNMN_EAGAIN with `arena_floats` set when the activation arena is too small (nothing launched).
 *   The records stay valid until the next call on the same planner (the backward of this step must be queued, on
 *   the same stream, before that).
 * ------------------------------------------------------------------------------------------- */
#define PNMN_EAGAIN (-3)
typedef struct pnmn_trunk_config {
    const int32_t* kinds;      /* [n_kinds] */
    const int64_t* w3;         /* [n_kinds][6] projection, conv1..conv5 weights */
    const int64_t* b3;         /* [n_kinds][6] biases */
    const int64_t* wt3;        /* [n_kinds][6] transposed copies */
    const int64_t* dotw;       /* [n_kinds] one-channel head weight */
    const int64_t* dotb;       /* [n_kinds] */
    int32_t n_kinds, channels, H, W, wgrad_chunk, wgrad_groups, fuse_mask_bwd, sole_writer, sort_by_weight, reserved;
} pnmn_trunk_config;       /* 88 bytes */
typedef struct pnmn_trunk_io {
    const int64_t*     programs;      /* in: host [n_programs][length] */
    uint64_t           params, grads, wt, act, gact, feat, gfeat, final_, gfinal, ones;  /* in: device bases */
    int64_t            act_capacity;  /* in: floats behind act (and gact) */
    const pnmn_launch* fwd_tail;      /* in: host, appended to the forward list */
    const pnmn_launch* bwd_head;      /* in: host, opens the backward list */
    const pnmn_launch* bwd_tail;      /* in: host, closes it */
    pnmn_launch*       bwd;           /* out: host [bwd_capacity] */
    uint8_t*           valid;         /* out: host [n_programs] */
    int64_t            arena_floats;  /* out */
    int32_t            n_programs, length, n_fwd_tail, n_bwd_head, n_bwd_tail, bwd_capacity, need_backward, launch;
    int32_t            n_bwd, bwd_piece_cut, n_prims, n_fwd, depth, n_invalid, n_feat_result;
    int32_t            conv_cus;      /* in: CU budget of the module programs' conv launches (0 = all CUs) */
    int32_t            wgrad_cus;     /* in: CU budget of their weight-gradient launches (0 = none) */
    int32_t            n_conv, n_proj;           /* out: 3x3 / projection records of the batch (FLOP accounting)       */
    int32_t            reserved;
    uint64_t           touched_tokens[4];        /* out: bit t set = some VALID program's result depends on a call of program
                                                    token t (t < 256) -- the modules the reference's autograd reaches: a chain
                                                    a later `scene` drops is executed there but gets no gradient (nmn.py:197-241) */
} pnmn_trunk_io;           /* 256 bytes */
int pnmn_trunk_planner_create(const pnmn_trunk_config* config, void** planner);
int pnmn_trunk_planner_destroy(void* planner);
int pnmn_trunk_plan_and_launch(void* planner, pnmn_trunk_io* io, void* stream);
/* test hook: the forward list of the last call (launch == 0 leaves it un-issued); returns the entry count */
int pnmn_trunk_last_forward(void* planner, pnmn_launch* out, int capacity);
/* test hook: the record words of the last launch == 0 call (the list entries then point into a buffer that would start
 * at device address 0x10000); returns their size in bytes */
int64_t pnmn_trunk_last_records_bytes(void* planner, uint64_t* out, int64_t capacity_words);
/* For the last pnmn_trunk_plan_and_launch call: offsets[i][p] = float offset into `act` of the one-channel map written by
 * the module call of token position p of program i, or -1.  Returns n_programs * length, PNMN_EINVAL on a null
 * planner / short capacity.  Works after launch == 0 calls too (no device).
 * -1: the program is invalid; the token is skipped or `scene`; the call's output has `channels` channels (query,
 * comparison, and / or with a wide operand); the call is not executed because the result does not depend on it.  Every
 * executed call has a slot of its own in the arena, so the maps stay intact until the planner's next call.  A call that
 * failed (PNMN_EAGAIN included) leaves nothing to ask about: 0. */
int64_t pnmn_trunk_last_attention(void* planner, int64_t* offsets /* HOST [n_programs][length] */, int64_t capacity);

/* ---------------------------------------------------------------------------------------------
 * Host-side batch planner (no device work)                    replaces the per-example interpreter loop of
 * nmn.py:191-238 together with probnmn.runtime.schedule.BatchScheduler (csrc/host_plan.hip)
 *   in:   the template bank ([n_templates][pmax][18] int64 primitive tables, see schedule.py), per valid
 *         example its template id, batch index, first float of its arena block and the token of each call
 *         ([nv][cmax]); per-token weight offset tables (floats into the parameter / gradient / transposed-weight
 *         arenas); device base addresses in bytes
 *   out:  out_words = the record matrices back to back (uint64 words, bit-identical to the structs above):
 *         0 conv, 1 dgrad, 2 wgrad items (3x3), 3 wgrad jobs (3x3), 4 proj, 5 pdgrad, 6 wgrad items (proj),
 *         7 wgrad jobs (proj), 8 dot, 9 same, 10 minmax, 11 maskbwd -- each sorted by (level, weight)
 *         meta[0] = primitives, meta[1] = deepest level, meta[2 + 3k ..] = (first word, rows, words per row) of
 *         record kind k, meta[38] = number of cuts
 *         cuts[i] = (kind, level, begin, end): runs of one level in a sorted record array (kinds 0 conv, 1 proj,
 *         2 dot, 3 same, 4 minmax, 5 dgrad, 6 maskbwd, 7 pdgrad -- pdgrad levels are 2*level + operand), and
 *         kind 8 = a group of 3x3 weight-gradient jobs (lowest forward level of the group, first job, one past)
 *   returns PNMN_EINVAL when a capacity is too small (out_capacity words, cuts_capacity rows of 4 int32)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const int64_t* tables;
    const int64_t* nprims;
    const int64_t* tids;
    const int64_t* examples;
    const int64_t* base;
    const int64_t* tokens;
    const int64_t* w3;
    const int64_t* b3;
    const int64_t* wt3;
    const int64_t* dotw;
    const int64_t* dotb;
    uint64_t params, grads, wt, act, gact, feat, gfeat, final_, gfinal, ones;
    int32_t n_templates, pmax, nv, cmax;
    int32_t hw, channels, wgrad_chunk, wgrad_groups;
    int32_t fuse_mask_bwd, sole_writer, sort_by_weight, reserved;
} pnmn_plan_in;   /* 216 bytes */
int pnmn_plan_batch(const pnmn_plan_in* in, uint64_t* out_words, int64_t out_capacity, int64_t* meta, int32_t* cuts,
                    int32_t cuts_capacity);
/* ---------------------------------------------------------------------------------------------
 * Host-side batch program compiler (no device work)        nmn.py:191-238, SURVEY App. C
 *   tokens [n_programs][length] int64 prefix programs; kinds[token] = module class of each
 *   vocabulary entry (0 skip, 1 scene, 2 and, 3 or, 4 comparison, 5 attention, 6 query, 7 relate,
 *   8 same; probnmn.runtime.program_compiler.classify_token).
 *   per program: valid (the reference interpreter would not raise), n_calls, the calls in execution
 *   order as 7 int32 each (kind, token, a, b, a_channels, b_channels, out_channels; value ids:
 *   0 = stem features, 1 = all-ones attention, k >= 2 = output of call k-2) into
 *   calls[n_programs][length][7], and the value id of the result.
 * ------------------------------------------------------------------------------------------- */
int pnmn_compile_programs(const int64_t* tokens, int n_programs, int length, const int32_t* kinds,
                          int n_kinds, int channels, uint8_t* valid, int32_t* n_calls,
                          int32_t* calls, int32_t* result);

/* ---------------------------------------------------------------------------------------------
 * Feature extractor (csrc/resnet.hip): the convolutions of torchvision's ResNet-101 up to stage 3, which the reference
 * runs offline to produce the NMN's input features (/root/reference/scripts/preprocess/extract_features.py:98-105 build
 * resnet101(pretrained=True) with layer4 / avgpool / fc replaced by Identity, eval mode; :124-131 run it under no_grad).
 * Tensors are NHWC fp32 on the device.
 *
 * pnmn_conv2d_nhwc: y[n][oy][ox][co] = act( scale[co] * sum_{ky,kx,ci} x[n][oy*stride-pad+ky][ox*stride-pad+kx][ci] *
 *                   w[co][(ky*kw+kx)*Cin+ci] + shift[co] (+ residual[n][oy][ox][co]) ),  act = ReLU if `relu`.
 *   Replaces nn.Conv2d(bias=False) + nn.BatchNorm2d in eval mode (+ the block's `out += identity; relu`) of
 *   torchvision.models.resnet (0.5.0: Bottleneck.forward, ResNet._forward_impl); scale = gamma / sqrt(var + eps),
 *   shift = beta - mean * scale are folded by the host.  Cin a multiple of 4 (the image is padded from 3 to 4 channels),
 *   Cout a multiple of 64; w is [Cout][Kpad] with K = kh*kw*Cin padded with zeros to pnmn_conv2d_weight_floats / Cout.
 *   Ho / Wo must equal floor((H + 2 pad - k) / stride) + 1 (PNMN_ESHAPE otherwise).
 * pnmn_maxpool3x3s2_nhwc: nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (ResNet.maxpool); C a multiple of 4. */
typedef struct pnmn_conv2d_desc {
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    const float* residual;  /* or NULL */
    float*       y;
    int32_t      N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, relu;
} pnmn_conv2d_desc;         /* 96 bytes */
int pnmn_conv2d_nhwc(const pnmn_conv2d_desc* desc, void* stream);
int pnmn_conv2d_weight_floats(int Cout, int Cin, int kh, int kw);
int pnmn_maxpool3x3s2_nhwc(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image front end of the feature extractor (csrc/image_prep.hip): decoded uint8 images -> the stem convolution's input.
 * Replaces: Image.resize((224, 224), BILINEAR) + ToTensor + Normalize of the reference's transform
 *           (scripts/preprocess/extract_features.py:60-73), which runs on the CPU in Pillow and torchvision.
 * Pillow's 8-bit resampler is integer arithmetic, and this is that arithmetic: bit-identical results.  Per axis the host
 * supplies Pillow's coefficient table (probnmn.data.feature_extractor.resize_coefficients): for output index i the taps
 * k[i][0 .. ksize) in 22-bit fixed point and bounds[i] = (first input index, number of taps n <= ksize); one pass is
 *   pass(in)[i] = clip(((1 << 21) + sum_{t < n} in[first + t] * k[i][t]) >> 22, 0, 255)          -> uint8
 * The horizontal pass runs first, the vertical pass on its uint8 result, then
 *   out[n][y][x][c] = lut[c][resized[n][y][x][c]]  for c < 3,   out[n][y][x][3] = 0
 * with lut[c][v] = (v / 255 - mean[c]) / std[c] computed by the host in fp32.
 *   images   [N][Hin][Win][3] uint8, image n at images + n * image_stride bytes (image_stride >= 3 * Hin * Win)
 *   kx, ky   int32 [Wout][ksx], [Hout][ksy];   xbounds, ybounds   int32 [Wout][2], [Hout][2];   lut   fp32 [3][256]
 *   out      fp32 [N][Hout][Wout][4], 16-byte aligned
 * Limits (PNMN_EINVAL beyond them, as for a null pointer, a non-positive size or a short image_stride; nothing is
 * launched): ksx, ksy <= PNMN_IMAGE_PREP_MAX_TAPS (33: a 16x downscale), Wout <= PNMN_IMAGE_PREP_MAX_WIDTH, Hin, Win,
 * Hout <= PNMN_IMAGE_PREP_MAX_SIZE.  N == 0 returns 0 without a launch.  No byte outside [images, images + N *
 * image_stride) is read whatever the tables hold: every index is clamped to the image.
 * ------------------------------------------------------------------------------------------- */
#define PNMN_IMAGE_PREP_MAX_TAPS  33
#define PNMN_IMAGE_PREP_MAX_WIDTH 448
#define PNMN_IMAGE_PREP_MAX_SIZE  16384
int pnmn_image_prep(const uint8_t* images, int64_t image_stride, int N, int Hin, int Win, const int32_t* kx,
                    const int32_t* xbounds, int ksx, const int32_t* ky, const int32_t* ybounds, int ksy,
                    const float* lut, float* out, int Hout, int Wout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention maps of the module programs (csrc/attention_maps.hip): where a program looked.
 * Not in the reference (its interpreter drops every intermediate output: probnmn/models/nmn.py:197-238).
 *
 * pnmn_attention_gather: row j of out = the HW floats at act + offsets[j] (pnmn_trunk_last_attention's offsets, on the
 *   device), or zeros where offsets[j] < 0.  n == 0 returns 0 without a launch; null pointers or HW <= 0: PNMN_EINVAL.
 *
 * pnmn_attention_overlay: map j, resized to the image with bilinear interpolation (half-pixel centres, as
 *   F.interpolate(..., align_corners=False)), coloured through `lut` and blended over image image_of[j].  Integer
 *   arithmetic throughout (tests/helpers/overlay_reference.py restates it in numpy, bit for bit):
 *     quantise     q = (int)fmaf(fminf(fmaxf(a, 0), 1), 255.0f, 0.5f)                               (NaN -> 0)
 *     per axis     (output size n_out, map size n_in, output index X)  num = (2X + 1) * n_in - n_out, den = 2 * n_out;
 *                  num < 0: i0 = 0, f = 0; else i0 = num / den, f = ((num - i0 * den) * 256) / den;
 *                  then i0 = min(i0, n_in - 1), i1 = min(i0 + 1, n_in - 1)
 *     interpolate  v = ((q[y0][x0] * (256 - fx) + q[y0][x1] * fx) * (256 - fy)
 *                       + (q[y1][x0] * (256 - fx) + q[y1][x1] * fx) * fy + 32768) >> 16               (0 .. 255)
 *     blend        w = (v * strength + 127) / 255;
 *                  out[j][Y][X][c] = (img[Y][X][c] * (255 - w) + lut[v][c] * w + 127) / 255         for c < 3
 *   maps     fp32 [n][H][W];   image_of   int32 [n], clamped into [0, n_images): no byte outside the images is read
 *   images   uint8 [n_images][Hi][Wi][3], image i at images + i * image_stride bytes (image_stride >= 3 * Hi * Wi)
 *   lut      uint8 [256][3];   out   uint8 [n][Hi][Wi][3], any alignment
 *   Limits (PNMN_EINVAL beyond them or with a null pointer; nothing is launched): 1 <= H, W <= PNMN_ATTENTION_MAX_MAP,
 *   1 <= Hi, Wi <= PNMN_ATTENTION_MAX_IMAGE, 0 <= strength <= 255, n_images >= 1, n >= 0.  n == 0 returns 0 without a launch.
 *   Items that share an image are best handed over next to each other: the image is then read from HBM once.
 * ------------------------------------------------------------------------------------------- */
#define PNMN_ATTENTION_MAX_MAP   64
#define PNMN_ATTENTION_MAX_IMAGE 16384
int pnmn_attention_gather(const float* act, const int64_t* offsets /* DEVICE [n] */, float* out /* [n][HW] */, int n, int HW, void* stream);
int pnmn_attention_overlay(const float* maps /* [n][H][W] */, const int32_t* image_of /* DEVICE [n] */, const uint8_t* images,
                           int64_t image_stride, int n_images, int Hi, int Wi, const uint8_t* lut /* DEVICE [256][3] */,
                           int strength /* 0..255 */, uint8_t* out /* [n][Hi][Wi][3] */, int n, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Several LSTM-layer passes in ONE launch; the two layers of an encoder as a wavefront (csrc/lstm_stack.hip).
 * Replaces: the stacked nn.LSTM of the seq2seq encoders and of ProgramPrior under autograd
 *           (probnmn/modules/seq2seq_base.py:56-60 via allennlp PytorchSeq2SeqWrapper; probnmn/models/program_prior.py:50-56),
 *           i.e. pnmn_lstm_seq_fwd + the input-projection GEMM + pnmn_lstm_seq_fwd per encoder (and the same backward).
 * A job = one layer over [B][T] (hidden 256).  dep < 0: the layer's step inputs / output gradients are given (`xp` + `tokens`
 * as pnmn_lstm_seq_fwd; `dhs` as pnmn_lstm_seq_bwd).  dep >= 0, forward: the layer ABOVE job `dep` -- its input is that
 * job's `hs`, projected in the kernel with `w_ih` (fragment order of W_ih [4H][H]) and `bias` (b_ih + b_hh); backward: the
 * layer BELOW job `dep` -- its output gradient is that job's dgates times `w_ih` (fragment order of W_ih^T, i.e. of the
 * matrix [H][4H]).  A job has at most one dependant, chains are two long, linked jobs have equal B and T.  `w_hh`:
 * fragment order of W_hh (forward) / of W_hh^T (backward), as pnmn_lstm_seq_*.  All jobs' workgroups (8 per 16 rows) must
 * be resident at once: pnmn_lstm_stack_workspace_bytes returns 0 when they are not (use the per-layer entry points).
 * ------------------------------------------------------------------------------------------- */
#define PNMN_LSTM_STACK_JOBS 6
typedef struct pnmn_lstm_stack_job {
    const float*   xp;            /* forward, dep < 0 */
    const int64_t* tokens;
    int64_t        token_stride;
    const float*   w_hh;
    const float*   w_ih;          /* dep >= 0 */
    const float*   bias;          /* forward, dep >= 0 */
    float*         hs;            /* forward out */
    float*         cs;            /* forward out, backward in */
    float*         act;           /* forward out, backward in */
    const float*   dhs;           /* backward, dep < 0 */
    float*         dgates;        /* backward out */
    int32_t        B, T, dep, reserved;
} pnmn_lstm_stack_job;            /* 104 bytes */
int64_t pnmn_lstm_stack_workspace_bytes(const pnmn_lstm_stack_job* jobs /* HOST */, int n, int backward);
int pnmn_lstm_stack_fwd(const pnmn_lstm_stack_job* jobs /* HOST */, int n, void* workspace, void* stream);
int pnmn_lstm_stack_bwd(const pnmn_lstm_stack_job* jobs /* HOST */, int n, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM dropout between an encoder's layers (csrc/lstm_dropout.hip, csrc/lstm_stack.hip, csrc/dropout.h).
 * Replaces: nn.LSTM(..., dropout=p) in training mode (reference probnmn/modules/seq2seq_base.py:57,78;
 *           probnmn/models/program_prior.py:42,56): the output of every layer but the last, at every step, times a mask on
 *           its way to the next layer's input.
 * Mask: y = x * keep * scale with scale = 1.0f / (1.0f - p) (fp32) and keep(row, t, u) from Philox4x32-10 (the generator of
 *   pnmn_sample_tokens): key {seed lo, seed hi}, counter {row lo, row hi, t, u}, output word 0 -> u01 = (x0 >> 8) * 2^-24;
 *   keep iff u01 < 1.0f - p (fp32).  row = row_offset + the row's index in the pass.  A dropped element is x * 0 (p = 1:
 *   zeros).  Backward applies the same call to the gradient (the same seed and row_offset regenerate the mask).
 * pnmn_lstm_dropout: y = mask(x) over [rows][T][H] (H % 4 == 0, 16-byte aligned; y == x allowed).
 * pnmn_lstm_stack_{fwd,bwd}_dropout: pnmn_lstm_stack_{fwd,bwd} with one descriptor per job (drops[k] for jobs[k]; p = 0:
 *   none).  Forward, p > 0 only on a job with dep < 0 that has a dependant: it also writes hsd = mask(hs) and the dependant
 *   reads hsd instead of hs.  Backward, p > 0 only on a job with dep >= 0: the gradient arriving from the layer above is
 *   masked.  When no job has p > 0 these run exactly the kernels of pnmn_lstm_stack_{fwd,bwd}.
 * ------------------------------------------------------------------------------------------- */
typedef struct pnmn_lstm_dropout_desc {
    float*   hsd;           /* forward: [B][T][H] out, the job's hs after the mask */
    uint64_t seed;
    int64_t  row_offset;
    float    p;             /* in [0, 1]; 0 = no dropout on this job */
    int32_t  reserved;
} pnmn_lstm_dropout_desc;   /* 32 bytes */
int pnmn_lstm_dropout(const float* x, float* y, int rows, int T, int H, float p, uint64_t seed, int64_t row_offset, void* stream);
int pnmn_lstm_stack_fwd_dropout(const pnmn_lstm_stack_job* jobs /* HOST */, const pnmn_lstm_dropout_desc* drops /* HOST */, int n,
                                void* workspace, void* stream);
int pnmn_lstm_stack_bwd_dropout(const pnmn_lstm_stack_job* jobs /* HOST */, const pnmn_lstm_dropout_desc* drops /* HOST */, int n,
                                void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 GEMM, up to PNMN_GEMM_MAX independent problems per launch (csrc/gemm.hip).
 * Replaces: every product over all time steps that the reference reaches through nn.LSTM / nn.Linear / autograd in
 *           the seq2seq models (probnmn/modules/seq2seq_base.py:101-155 via allennlp's SimpleSeq2Seq: encoder input
 *           projections, `_output_projection_layer`, and the weight / data gradients autograd derives for them) and
 *           ProgramPrior's projection + tied output layer (probnmn/models/program_prior.py:101-104).
 *   C[M][N] (row stride ldc) = [C +] op(A) op(B) [+ bias[N]]
 *   A: [M][K] with row stride lda, or -- PNMN_GEMM_A_TRANSPOSED -- stored [K][M] (a weight gradient's dy^T)
 *   B: [K][N] with row stride ldb, or -- PNMN_GEMM_B_TRANSPOSED -- stored [N][K] (nn.Linear's weight)
 *   shift_t > 0 (B as [K][N] only): k row r reads storage row r - 1, and where r % shift_t == 0 row r / shift_t of
 *     shift_h0 (row stride ld_h0; zeros when NULL): "h_{t-1}" of a [B][T][N] tensor of states without a shifted copy
 *   split_k > 1: the K range is cut into that many chunks (whole 32-wide k tiles) whose partial tiles go to
 *     `workspace` (pnmn_gemm_workspace_bytes) and are added in chunk order (+ bias, + C when accumulating) by a second
 *     small launch behind the product on the same stream: deterministic, no atomics.  pnmn_gemm_split_k proposes a count.
 *   colsum != NULL (PNMN_GEMM_A_TRANSPOSED only, else PNMN_ESHAPE): colsum[m] = sum_k A[k][m], m < M, also stored to
 *     colsum2 when given -- the bias gradient torch's autograd forms as dy.sum(0) beside the weight gradient dy^T x; the
 *     rows of dy pass through the workgroups of the first tile column anyway (fixed summation order, split or not).
 * ------------------------------------------------------------------------------------------- */
#define PNMN_GEMM_MAX 8
#define PNMN_GEMM_A_TRANSPOSED 1
#define PNMN_GEMM_B_TRANSPOSED 2
#define PNMN_GEMM_ACCUMULATE   4
typedef struct pnmn_gemm_desc {
    const float* a;
    const float* b;
    float*       c;
    const float* bias;      /* [N] or NULL */
    int64_t      lda, ldb, ldc;
    int32_t      M, N, K;
    int32_t      flags;     /* PNMN_GEMM_* */
    int32_t      split_k;   /* <= 1: none */
    int32_t      shift_t;
    const float* shift_h0;
    int64_t      ld_h0;
    float*       workspace; /* split_k > 1 */
    float*       colsum;    /* A stored [K][M] only: colsum[m] = sum_k A[k][m] (the bias gradient beside a weight gradient */
    float*       colsum2;   /*   dy^T x: the rows of dy pass through the kernel anyway), also stored here; or NULL          */
} pnmn_gemm_desc;
int pnmn_gemm(const pnmn_gemm_desc* descs /* HOST array */, int n, void* stream);
/* ... with at most `max_workgroups` workgroups (0 = one per tile): a launch that shares the chip with another stream's
 * dependent chain of kernels (the NMN trunk beside the seq2seq passes) and must not take every CU from it. */
int pnmn_gemm_cus(const pnmn_gemm_desc* descs /* HOST array */, int n, int max_workgroups, void* stream);
int64_t pnmn_gemm_workspace_bytes(int M, int N, int split_k);
int pnmn_gemm_split_k(int M, int N, int K, int cus);
/* ... over a LIST of k rows: rows[i] / count[i] (HOST arrays of n DEVICE addresses) give problem i a list of *count[i]
 * entries (row, prev) as pnmn_valid_rows builds it, and the product contracts the listed storage rows only -- a weight
 * gradient dy^T x of a padded [B][T][.] pass, whose dy is zero at the padded pairs, skips them.  The list serves both
 * operands, so they must both be stored with k as the slow index: PNMN_GEMM_A_TRANSPOSED without PNMN_GEMM_B_TRANSPOSED,
 * anything else with a list returns PNMN_ESHAPE.  rows[i] == NULL (or rows == NULL): problem i runs as in pnmn_gemm_cus.
 * The shifted operand of a listed row reads storage row `prev`, or -- prev = ~b < 0 -- row b of shift_h0 (zeros when NULL);
 * shift_t is then only a flag.  colsum / colsum2 sum the listed rows.  Nothing is read back: K, split_k and the workspace
 * are those of the full product, the kernel reads *count (clamped to [0, K]) and every chunk takes its equal share of the
 * listed k tiles; a chunk left without any writes a zero partial, count == 0 gives C = [C +] 0 [+ bias]. */
int pnmn_gemm_rows(const pnmn_gemm_desc* descs /* HOST array */, int n, const int32_t* const* rows /* HOST array */,
                   const int32_t* const* count /* HOST array */, int max_workgroups, void* stream);

/* out[c] = [out[c] +] sum_r x[r*ld + c], c < C; also stored to out2 when not NULL (an LSTM layer's b_ih and b_hh receive
 * the same gradient: torch autograd's sum over rows of the gate gradients).  workspace: pnmn_colsum_workspace_bytes,
 * zeroed once by the caller. */
int pnmn_colsum(const float* x, int64_t ld, int R, int C, float* out, float* out2, int accumulate, void* workspace, void* stream);
int64_t pnmn_colsum_workspace_bytes(int R, int C);

/* Library self-description (no GPU needed).  13 also carries pnmn_valid_rows / pnmn_gemm_rows (new functions only: no record changes).  12: pnmn_gemm_desc gains colsum / colsum2 (120 bytes), pnmn_gemm_workspace_bytes includes the column-sum partials.  11 = round 6: pnmn_gemm / pnmn_colsum / pnmn_token_rows, an accumulate flag on pnmn_embedding_grad, row stride + second bias output on pnmn_token_table_bwd.  10 = round 5.  8 = round 4: the trunk executor of version 7 removed again (pnmn_trunk_exec, pnmn_plan_batch_owners, the EXEC launch op; pnmn_trunk_io shrinks to 224 bytes), streamed convolution kernel behind the same pnmn_conv_nhwc entry points (split 16 gone).  7: the trunk executor (pnmn_trunk_exec, EXEC launch op, pnmn_trunk_io grows to 232 bytes), conv segments in one launch; 6 = round 3: pnmn_conv_nhwc_cus, paired decoder launches, pnmn_attn_denc, pnmn_joint_objective, ingest by copy engine; 5: the trunk planner (pnmn_trunk_*), pnmn_set_rows, SET_ROWS / ACCUMULATE / ZERO launch ops; 4: pnmn_cluster_reserve_cus.  3 = round 2: 28x28 maps in the conv / weight-gradient / layout /
 * pool entry points, pnmn_conv_nhwc_launches takes H and W, sequence-loss / ELBO / feature-ingest entry points
 * added, the persistent dataflow executor (pnmn_dataflow) removed. */
#define PNMN_ABI_VERSION 14   /* what pnmn_abi_version() returns; the binding refuses a library built from another */
int pnmn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PROBNMN_HIP_H */
