// Feature ingest for gfx950: a batch's image features go from a page-locked host store straight into
// the NHWC device buffer the stem reads -- one launch, no staging copy, no per-row memcpy calls.
//
// The reference keeps features as float64 (N, 1024, H, W) in HDF5, indexes one row per example on the
// host, casts to float and lets the DataLoader collate and the trainer `.to(device)` the batch
// (probnmn/data/readers.py:63-108, datasets.py:137-142, trainers/_trainer.py:272-287): three host passes
// over 0.8 MB per question before the H2D copy.  Here the store is pre-cast fp32 in hipHostMalloc memory
// (device-visible on ROCm); the kernel reads the selected rows over PCIe (coalesced 256-byte runs of one
// channel's pixels), transposes 64 channels x <= 392 pixels through LDS and writes full 256-byte NHWC
// pixel rows.  It replaces the gather, the cast, the H2D copy AND the NCHW -> NHWC pass of the stem's
// prologue.  Bound by PCIe Gen5 x16 (63 GB/s spec): 0.8 MB per question -> ~78 k questions/s per GPU.
//
// The store may also keep its rows as fp16 or bf16 (pnmn_gather_features_typed): half the bytes over the link per
// question, widened -- exactly -- on the way into the same fp32 NHWC batch (gather_narrow_kernel); and a store that lives in
// HBM at two bytes per element is filled by the fp32 kernel rounding in its write-out and read back, widened, by
// pnmn_expand_rows.  The networks compute in fp32 either way.
//
// The same at one byte per element (PNMN_ELEM_F8E4M3 / PNMN_ELEM_F8E5M2, fp8_convert.h): a quarter of the bytes over the
// link, the same kernels with 1-byte elements, and pnmn_narrow_rows for a chunk that is already on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/probnmn_hip.h"
#include "fp8_convert.h"

namespace {

// Element conversions of the half-precision stores (PNMN_ELEM_F16 / PNMN_ELEM_BF16).  Widening is exact; narrowing is
// round to nearest even with overflow to infinity and subnormals kept, what torch's Tensor.to(dtype) gives on the host
// (fp16: the hardware conversion, whose fp16 denormals are always on; bf16: the integer form of the same rounding).
// The 8-bit stores (PNMN_ELEM_F8E4M3 / PNMN_ELEM_F8E5M2): fp8_convert.h, which states the same contract -- with NaN in the
// place of infinity for e4m3fn, which has none.
struct F16 { typedef uint16_t bits_t; uint16_t bits; };
struct BF16 { typedef uint16_t bits_t; uint16_t bits; };
struct F8E4M3 { typedef uint8_t bits_t; uint8_t bits; };
struct F8E5M2 { typedef uint8_t bits_t; uint8_t bits; };
template <class T> __device__ __forceinline__ float widen(uint16_t h);
template <> __device__ __forceinline__ float widen<F16>(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
template <> __device__ __forceinline__ float widen<BF16>(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }
template <> __device__ __forceinline__ float widen<F8E4M3>(uint16_t b) { return pnmn_f8::widen_e4m3((uint8_t)b); }
template <> __device__ __forceinline__ float widen<F8E5M2>(uint16_t b) { return pnmn_f8::widen_e5m2((uint8_t)b); }
template <class T> __device__ __forceinline__ T narrow(float x);
template <> __device__ __forceinline__ float narrow<float>(float x) { return x; }
template <> __device__ __forceinline__ F16 narrow<F16>(float x) { return F16{__builtin_bit_cast(uint16_t, (_Float16)x)}; }
template <> __device__ __forceinline__ BF16 narrow<BF16>(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return BF16{(uint16_t)0x7fc0};  // (NaN: torch's quiet NaN)
    return BF16{(uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16)};
}
template <> __device__ __forceinline__ F8E4M3 narrow<F8E4M3>(float x) { return F8E4M3{pnmn_f8::narrow_e4m3(x)}; }
template <> __device__ __forceinline__ F8E5M2 narrow<F8E5M2>(float x) { return F8E5M2{pnmn_f8::narrow_e5m2(x)}; }
__device__ __forceinline__ bool is_finite(F8E4M3 v) { return pnmn_f8::finite_e4m3(v.bits); }
__device__ __forceinline__ bool is_finite(F8E5M2 v) { return pnmn_f8::finite_e5m2(v.bits); }

// A FIXED, small number of workgroups walks the (example, 64-channel block, pixel range) work items: the kernel is
// bound by PCIe, not by the chip -- a few hundred KB in flight saturate the link -- and it runs on the loader's
// stream BESIDE a training step.  One workgroup per work item (round 2: 16 384 of them, 50 KB of LDS each) let the
// dispatcher park two or three of these on every CU, where they wait out microsecond PCIe round trips while their
// LDS keeps the step's convolution workgroups (98 KB) off the CU: the step ran 1.45x slower with its ingest beside
// it.  With `gridDim.x` <= 12 resident workgroups (16-byte loads, eight in flight per thread: 42.7 GB/s on an idle chip,
// the most this kernel reaches with any grid) and a 26 KB tile a convolution workgroup still fits next to one.  Measured
// beside the 1024-question step (round 3, gpurun_out r03k-r03n): 4 / 8 / 12 / 16 / 32 / 64 / 1024 workgroups -> 51.6 /
// 40.8 / 39.5 / 39.8 / 44.7 / 49.3 / 52.8 ms per step against 32.4 ms with resident features -- below ~12 the link is
// not filled (the ingest becomes the critical path), above it the step slows with the number of PCIe reads in flight
// (they hold memory-system queue entries for microseconds each), and ~7 ms of the step's 32 stay unhidden at best.
// `Out`: float, or F16 / BF16 / F8E4M3 / F8E5M2 when the fp32 staging buffer fills a narrower device store -- the same
// kernel, the rounding in the store of the write-out.
template <class Out>
__global__ __launch_bounds__(256) void gather_features_kernel(const float* __restrict__ store,
                                                              const int64_t* __restrict__ indices,
                                                              Out* __restrict__ dst, int64_t n_store, int Cn,
                                                              int HW, int PT, int n, int parts) {
    extern __shared__ float tile[];  // [64][PT+1]
    const int cblocks = (Cn + 63) / 64;
    const int total_items = n * cblocks * parts;
    const int ld = PT + 1;
    constexpr int NB = 8;  // loads in flight per thread: the PCIe round trip is microseconds
    for (int item = blockIdx.x; item < total_items; item += gridDim.x) {
        const int part = item % parts, cb = (item / parts) % cblocks, e = item / (parts * cblocks);
        const int c0 = cb * 64;
        const int p0 = part * PT;
        const int np = (HW - p0) < PT ? (HW - p0) : PT;
        const int cw = (Cn - c0) < 64 ? (Cn - c0) : 64;
        int64_t row = indices[e];
        if (row < 0 || row >= n_store) row = 0;  // (validated on the host; never index outside the store)
        const float* src = store + ((size_t)row * Cn + c0) * HW + p0;
        const int total = cw * np;
        if (((np | HW | p0) & 3) == 0) {
            // 16-byte loads (every channel's pixel run starts 16-byte aligned): a quarter of the load instructions per
            // byte -- the kernel shares its CUs' issue slots with the step it runs beside
            const int nq = np >> 2, total4 = cw * nq;
            typedef float f4 __attribute__((ext_vector_type(4)));
            for (int i0 = threadIdx.x; i0 < total4; i0 += 256 * NB) {
                f4 v[NB];
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const int i = i0 + k * 256;
                    const int c = i / nq;
                    v[k] = i < total4 ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(src + (size_t)c * HW + 4 * (i - c * nq)))
                                      : f4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const int i = i0 + k * 256;
                    const int c = i / nq;
                    if (i < total4) {
                        float* t = tile + c * ld + 4 * (i - c * nq);
                        t[0] = v[k].x, t[1] = v[k].y, t[2] = v[k].z, t[3] = v[k].w;
                    }
                }
            }
        } else
        for (int i0 = threadIdx.x; i0 < total; i0 += 256 * NB) {
            float v[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int i = i0 + k * 256;
                const int c = i / np;
                v[k] = i < total ? __builtin_nontemporal_load(src + (size_t)c * HW + (i - c * np)) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int i = i0 + k * 256;
                const int c = i / np;
                if (i < total) tile[c * ld + (i - c * np)] = v[k];
            }
        }
        __syncthreads();
        Out* out = dst + ((size_t)e * HW + p0) * Cn + c0;
        for (int i = threadIdx.x; i < total; i += 256) {
            const int p = i / cw, c = i - p * cw;
            out[(size_t)p * Cn + c] = narrow<Out>(tile[c * ld + p]);
        }
        __syncthreads();  // the tile is refilled by the next item
    }
}

// One stage of the gather from a narrow store: `nruns` runs of `run_len` elements of 1 or 2 bytes, run r at src + r *
// stride, into the tile at r * ld -- V elements (16, 8, 4 bytes or one element) per load, eight non-temporal loads in
// flight per thread.  The caller has checked that every run start, `ld` and `run_len` are multiples of V elements.
template <class E, int V> struct vec_of { typedef E type __attribute__((ext_vector_type(V))); };
template <class E> struct vec_of<E, 1> { typedef E type; };
template <class E, int V>
__device__ __forceinline__ void load_runs(const E* __restrict__ src, E* __restrict__ tile, int nruns, int run_len, int stride,
                                          int ld) {
    typedef typename vec_of<E, V>::type vec;
    constexpr int NB = 8;
    const int nq = run_len / V, units = nruns * nq;
    for (int i0 = threadIdx.x; i0 < units; i0 += 256 * NB) {
        vec v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = i0 + k * 256;
            const int r = i / nq;
            if (i < units) v[k] = __builtin_nontemporal_load(reinterpret_cast<const vec*>(src + (size_t)r * stride + V * (i - r * nq)));
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = i0 + k * 256;
            const int r = i / nq;
            if (i < units) *reinterpret_cast<vec*>(tile + r * ld + V * (i - r * nq)) = v[k];
        }
    }
}

// The gather from a narrow store (F16 / BF16 / F8E4M3 / F8E5M2 -> fp32): the same fixed grid and the same kind of work
// item, at half or a quarter of the bytes over the link.  The tile holds the elements as they are stored, [CB][PT]
// without padding, and the write-out widens.
//
// 2-byte elements, CB = 64: a channel's 196 pixels are 392 bytes -- every second channel's run starts 8 bytes off a
// 16-byte boundary -- so where the whole map fits the tile (parts == 1: HW <= 200, 25 088 bytes at 14x14) the item's 64
// channels are read as the ONE contiguous run they are in the store, which starts 16-byte aligned whenever the store
// does (64 channels x HW x 2 bytes = 128 HW).  Larger maps (28x28) are cut into ranges of 200 pixels (400 bytes: 16-byte
// aligned when HW is a multiple of 8) and read channel by channel.  Whatever does not divide -- HW not a multiple of 4,
// a channel tail below 64 whose run is no multiple of 8 elements -- falls to 8-byte and then 2-byte loads.  (The
// unpadded tile costs the write-out a 2- to 4-way bank conflict, stride 2 HW bytes between the channels of a pixel; the
// kernel waits for PCIe, not for LDS.)
//
// 1-byte elements: the same, with 16 / 8 / 4 / 1-byte loads (a channel's 196 bytes start 4 mod 16: the one contiguous
// run again) and pixel ranges of 400.  The link is filled by the bytes in flight, and twelve workgroups have one item
// each in flight: 64 channels x 196 bytes are 12.5 KB, half of what a 2-byte item keeps on the link.  So an item whose
// whole map fits takes CB = 128 channels (up to 256 for smaller maps) -- the same 25 KB tile, the same bytes in flight
// per workgroup as the half kernel, 512-byte pixel rows in the write-out.  (An fp32 tile, widened on the way in, would
// hold 6.4 KB of the store per 26 KB of LDS: a quarter of the link's appetite.  The tile therefore keeps the bytes.)
extern __shared__ __attribute__((aligned(16))) unsigned char narrow_tile[];  // [CB][PT] elements
template <class In>
__global__ __launch_bounds__(256) void gather_narrow_kernel(const typename In::bits_t* __restrict__ store,
                                                            const int64_t* __restrict__ indices, float* __restrict__ dst,
                                                            int64_t n_store, int Cn, int HW, int PT, int n, int parts, int CB) {
    typedef typename In::bits_t E;
    constexpr int V16 = 16 / (int)sizeof(E);  // elements in 16 bytes
    E* htile = reinterpret_cast<E*>(narrow_tile);
    const int cblocks = (Cn + CB - 1) / CB;
    const int total_items = n * cblocks * parts;
    for (int item = blockIdx.x; item < total_items; item += gridDim.x) {
        const int part = item % parts, cb = (item / parts) % cblocks, e = item / (parts * cblocks);
        const int c0 = cb * CB;
        const int p0 = part * PT;
        const int np = (HW - p0) < PT ? (HW - p0) : PT;
        const int cw = (Cn - c0) < CB ? (Cn - c0) : CB;
        int64_t row = indices[e];
        if (row < 0 || row >= n_store) row = 0;  // (validated on the host; never index outside the store)
        const E* src = store + ((size_t)row * Cn + c0) * HW + p0;
        // parts == 1: PT == HW, the channels' runs follow each other without a gap, in the store and in the tile
        const int nruns = parts == 1 ? 1 : cw, run_len = parts == 1 ? cw * HW : np;
        const int every = nruns == 1 ? run_len : (run_len | HW | PT);  // what every run start and length is a multiple of
        const unsigned at = (unsigned)(uintptr_t)src;
        if (every % V16 == 0 && (at & 15) == 0) load_runs<E, V16>(src, htile, nruns, run_len, HW, PT);
        else if (every % (V16 / 2) == 0 && (at & 7) == 0) load_runs<E, V16 / 2>(src, htile, nruns, run_len, HW, PT);
        else if (sizeof(E) == 1 && (every & 3) == 0 && (at & 3) == 0) load_runs<E, 4>(src, htile, nruns, run_len, HW, PT);
        else load_runs<E, 1>(src, htile, nruns, run_len, HW, PT);
        __syncthreads();
        const int total = cw * np;
        float* out = dst + ((size_t)e * HW + p0) * Cn + c0;
        if (sizeof(E) == 1 && ((np | PT) & 3) == 0) {
            // four pixels of a channel per thread and turn: one 4-byte LDS read, four stores a pixel row apart (the lanes
            // still walk the channels).  A workgroup is one wave per SIMD, so every turn of this loop pays its LDS read's and
            // its index arithmetic's latency in full; at one byte per element those turns, not the link, bound the kernel.
            const unsigned totalq = (unsigned)cw * (unsigned)(np >> 2);
#pragma unroll 2
            for (unsigned i = threadIdx.x; i < totalq; i += 256) {
                const unsigned q = i / (unsigned)cw, c = i - q * (unsigned)cw;
                const uint32_t w = *reinterpret_cast<const uint32_t*>(htile + c * PT + 4 * q);
                float* o = out + (size_t)(4 * q) * Cn + c;
                o[0] = widen<In>(w & 0xffu);
                o[Cn] = widen<In>((w >> 8) & 0xffu);
                o[2 * (size_t)Cn] = widen<In>((w >> 16) & 0xffu);
                o[3 * (size_t)Cn] = widen<In>(w >> 24);
            }
        } else
        for (int i = threadIdx.x; i < total; i += 256) {
            const int p = i / cw, c = i - p * cw;
            out[(size_t)p * Cn + c] = widen<In>(htile[c * PT + p]);
        }
        __syncthreads();  // the tile is refilled by the next item
    }
}

// Rows of a narrow device store widened into an fp32 batch (pnmn_expand_rows): a work item is 16 KB of one row -- 256
// threads x 4 loads of 16 bytes in flight, 8192 elements of two bytes or 16 384 of one, 2 or 4 x 16 bytes stored per
// load -- and the grid walks the (row, chunk) pairs.  HBM to HBM on the step's own stream: it may fill the chip.
template <class In>
__global__ __launch_bounds__(256) void expand_rows_kernel(const typename In::bits_t* __restrict__ rows,
                                                          const int64_t* __restrict__ indices, float* __restrict__ dst,
                                                          int64_t n_store, int64_t row_elems, int64_t chunks_per_row,
                                                          int64_t items, int vectors) {
    typedef typename In::bits_t E;
    constexpr int VE = 16 / (int)sizeof(E);  // elements of a 16-byte load
    typedef E ev __attribute__((ext_vector_type(VE)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t e = item / chunks_per_row, chunk = item - e * chunks_per_row;
        int64_t row = indices[e];
        if (row < 0 || row >= n_store) row = 0;
        const E* src = rows + (size_t)row * row_elems;
        float* out = dst + (size_t)e * row_elems;
        if (vectors) {
            const int64_t nv = row_elems / VE;
            ev v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = chunk * 1024 + k * 256 + threadIdx.x;
                if (j < nv) v[k] = *reinterpret_cast<const ev*>(src + VE * j);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = chunk * 1024 + k * 256 + threadIdx.x;
                if (j < nv) {
#pragma unroll
                    for (int q = 0; q < VE; q += 4)
                        *reinterpret_cast<f4*>(out + VE * j + q) =
                            f4{widen<In>(v[k][q]), widen<In>(v[k][q + 1]), widen<In>(v[k][q + 2]), widen<In>(v[k][q + 3])};
                }
            }
        } else {
            const int64_t lo = chunk * (1024 * VE), hi = lo + 1024 * VE < row_elems ? lo + 1024 * VE : row_elems;
            for (int64_t j = lo + threadIdx.x; j < hi; j += 256) out[j] = widen<In>(src[j]);
        }
    }
}

// An fp32 chunk that is already on the device, in the store's own (NHWC) order, rounded into rows of an 8-bit store
// (pnmn_narrow_rows): no transpose, 16 bytes read and 4 written per thread and turn where both ends are aligned,
// element by element otherwise.  `overflowed` counts what was finite in fp32 and is not in `Out`: a thread counts its
// own, the workgroup adds them up in LDS and adds a non-zero sum to the counter once.
template <class Out>
__global__ __launch_bounds__(256) void narrow_rows_kernel(const float* __restrict__ src, Out* __restrict__ dst, int64_t n,
                                                          int vectors, unsigned long long* __restrict__ overflowed) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ unsigned wg_bad;
    if (threadIdx.x == 0) wg_bad = 0;
    __syncthreads();
    unsigned bad = 0;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    const int64_t nv = vectors ? n >> 2 : 0;
    for (int64_t j = first; j < nv; j += step) {
        const f4 v = *reinterpret_cast<const f4*>(src + 4 * j);
        uint32_t packed = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const Out o = narrow<Out>(v[q]);
            bad += pnmn_f8::finite_f32(v[q]) && !is_finite(o);
            packed |= (uint32_t)o.bits << (8 * q);
        }
        *reinterpret_cast<uint32_t*>(dst + 4 * j) = packed;
    }
    for (int64_t j = 4 * nv + first; j < n; j += step) {  // (all of it without vectors, else the last n % 4)
        const Out o = narrow<Out>(src[j]);
        bad += pnmn_f8::finite_f32(src[j]) && !is_finite(o);
        dst[j] = o;
    }
    if (bad) atomicAdd(&wg_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0 && wg_bad) atomicAdd(overflowed, (unsigned long long)wg_bad);
}
}  // namespace

static int ingest_wgs() {  // (tuning hook)
    static const int max_wgs = [] {
        const char* e = getenv("PNMN_INGEST_WGS");
        const int v = e ? atoi(e) : 12;
        return v > 0 ? v : 12;
    }();
    return max_wgs;
}

template <class Out>
static int launch_gather_f32(const void* store, const int64_t* indices, void* dst, int n, int64_t n_store, int Cn, int HW,
                             void* stream) {
    // pixel ranges of 100 pixels (a multiple of four: 16-byte loads): a 26 KB tile (see the kernel's header)
    const int PT = HW < 100 ? HW : 100;
    const int parts = (HW + PT - 1) / PT;
    const size_t lds = (size_t)64 * (PT + 1) * sizeof(float);
    const int max_wgs = ingest_wgs();
    const long items = (long)n * ((Cn + 63) / 64) * parts;
    hipLaunchKernelGGL(gather_features_kernel<Out>, dim3((unsigned)(items < max_wgs ? items : max_wgs)), dim3(256), lds,
                       static_cast<hipStream_t>(stream), static_cast<const float*>(store), indices, static_cast<Out*>(dst),
                       n_store, Cn, HW, PT, n, parts);
    return (int)hipGetLastError();
}

template <class In>
static int launch_gather_narrow(const void* store, const int64_t* indices, void* dst, int n, int64_t n_store, int Cn, int HW,
                                void* stream) {
    typedef typename In::bits_t E;
    // a tile of at most 25 600 bytes: the whole map where 64 channels of it fit (HW <= 200 at two bytes, 400 at one),
    // else pixel ranges of that many; at one byte per element as many channels of a whole map as fit, 64 to 256
    const int most = 400 / (int)sizeof(E);
    const int PT = HW < most ? HW : most;
    const int parts = (HW + PT - 1) / PT;
    int CB = 64;
    if (sizeof(E) == 1 && parts == 1) CB = 25600 / HW >= 256 ? 256 : 25600 / HW >= 128 ? 128 : 64;
    const size_t lds = (size_t)CB * PT * sizeof(E);
    const int max_wgs = ingest_wgs();
    const long items = (long)n * ((Cn + CB - 1) / CB) * parts;
    hipLaunchKernelGGL(gather_narrow_kernel<In>, dim3((unsigned)(items < max_wgs ? items : max_wgs)), dim3(256), lds,
                       static_cast<hipStream_t>(stream), static_cast<const E*>(store), indices, static_cast<float*>(dst),
                       n_store, Cn, HW, PT, n, parts, CB);
    return (int)hipGetLastError();
}

static bool narrow_elem(int elem) {
    return elem == PNMN_ELEM_F16 || elem == PNMN_ELEM_BF16 || elem == PNMN_ELEM_F8E4M3 || elem == PNMN_ELEM_F8E5M2;
}

extern "C" int pnmn_gather_features_typed(const void* store, int src_elem, const int64_t* indices, void* dst, int dst_elem,
                                          int n, int64_t n_store, int Cn, int HW, void* stream) {
    const bool pair_ok = (src_elem == PNMN_ELEM_F32 && (dst_elem == PNMN_ELEM_F32 || narrow_elem(dst_elem))) ||
                         (narrow_elem(src_elem) && dst_elem == PNMN_ELEM_F32);
    if (!pair_ok) return PNMN_EINVAL;
    if (n <= 0) return 0;
    if (!store || !indices || !dst || Cn <= 0 || HW <= 0 || n_store <= 0) return PNMN_EINVAL;
    if ((long)n * ((Cn + 63) / 64) * ((HW + 99) / 100) > 0x7fffffffL) return PNMN_EINVAL;  // (the kernels count items in an int)
    switch (src_elem) {
        case PNMN_ELEM_F16: return launch_gather_narrow<F16>(store, indices, dst, n, n_store, Cn, HW, stream);
        case PNMN_ELEM_BF16: return launch_gather_narrow<BF16>(store, indices, dst, n, n_store, Cn, HW, stream);
        case PNMN_ELEM_F8E4M3: return launch_gather_narrow<F8E4M3>(store, indices, dst, n, n_store, Cn, HW, stream);
        case PNMN_ELEM_F8E5M2: return launch_gather_narrow<F8E5M2>(store, indices, dst, n, n_store, Cn, HW, stream);
    }
    switch (dst_elem) {
        case PNMN_ELEM_F16: return launch_gather_f32<F16>(store, indices, dst, n, n_store, Cn, HW, stream);
        case PNMN_ELEM_BF16: return launch_gather_f32<BF16>(store, indices, dst, n, n_store, Cn, HW, stream);
        case PNMN_ELEM_F8E4M3: return launch_gather_f32<F8E4M3>(store, indices, dst, n, n_store, Cn, HW, stream);
        case PNMN_ELEM_F8E5M2: return launch_gather_f32<F8E5M2>(store, indices, dst, n, n_store, Cn, HW, stream);
    }
    return launch_gather_f32<float>(store, indices, dst, n, n_store, Cn, HW, stream);
}

extern "C" int pnmn_gather_features(const float* store, const int64_t* indices, float* dst, int n, int64_t n_store,
                                    int Cn, int HW, void* stream) {
    return pnmn_gather_features_typed(store, PNMN_ELEM_F32, indices, dst, PNMN_ELEM_F32, n, n_store, Cn, HW, stream);
}

template <class In>
static int launch_expand_rows(const void* rows, const int64_t* indices, void* dst, int n, int64_t n_store, int64_t row_elems,
                              void* stream) {
    typedef typename In::bits_t E;
    constexpr int VE = 16 / (int)sizeof(E);
    const int vectors = row_elems % VE == 0 && (((uintptr_t)rows | (uintptr_t)dst) & 15) == 0;
    const int64_t chunks_per_row = (row_elems + 1024 * VE - 1) / (1024 * VE), items = (int64_t)n * chunks_per_row;
    const unsigned grid = (unsigned)(items < 4096 ? items : 4096);  // 16 workgroups per CU: the rest of the items by stride
    hipLaunchKernelGGL(expand_rows_kernel<In>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const E*>(rows), indices, static_cast<float*>(dst), n_store, row_elems, chunks_per_row, items,
                       vectors);
    return (int)hipGetLastError();
}

extern "C" int pnmn_expand_rows(const void* rows, int src_elem, const int64_t* indices, void* dst, int n, int64_t n_store,
                                int64_t row_elems, void* stream) {
    if (!narrow_elem(src_elem)) return PNMN_EINVAL;
    if (n <= 0) return 0;
    if (!rows || !indices || !dst || n_store <= 0 || row_elems <= 0) return PNMN_EINVAL;
    switch (src_elem) {
        case PNMN_ELEM_F16: return launch_expand_rows<F16>(rows, indices, dst, n, n_store, row_elems, stream);
        case PNMN_ELEM_BF16: return launch_expand_rows<BF16>(rows, indices, dst, n, n_store, row_elems, stream);
        case PNMN_ELEM_F8E4M3: return launch_expand_rows<F8E4M3>(rows, indices, dst, n, n_store, row_elems, stream);
    }
    return launch_expand_rows<F8E5M2>(rows, indices, dst, n, n_store, row_elems, stream);
}

template <class Out>
static int launch_narrow_rows(const float* src, void* dst, int64_t n, uint64_t* overflowed, void* stream) {
    const int vectors = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0;
    const int64_t turns = ((vectors ? (n + 3) / 4 : n) + 255) / 256;
    hipLaunchKernelGGL(narrow_rows_kernel<Out>, dim3((unsigned)(turns < 4096 ? turns : 4096)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, static_cast<Out*>(dst), n, vectors,
                       reinterpret_cast<unsigned long long*>(overflowed));
    return (int)hipGetLastError();
}

extern "C" int pnmn_narrow_rows(const float* src, void* dst, int dst_elem, int64_t n_elems, uint64_t* overflowed, void* stream) {
    if (dst_elem != PNMN_ELEM_F8E4M3 && dst_elem != PNMN_ELEM_F8E5M2) return PNMN_EINVAL;
    if (n_elems <= 0) return 0;
    if (!src || !dst || !overflowed) return PNMN_EINVAL;
    if (dst_elem == PNMN_ELEM_F8E4M3) return launch_narrow_rows<F8E4M3>(src, dst, n_elems, overflowed, stream);
    return launch_narrow_rows<F8E5M2>(src, dst, n_elems, overflowed, stream);
}

// The same ingest on the COPY ENGINES: one hipMemcpyAsync per selected row (0.8 MB, contiguous in the store) into a
// plain NCHW batch, which the stem's layout pass reads like any other input.  No compute unit takes part: a kernel
// that reads over PCIe keeps its loads outstanding for microseconds, and with enough of them in flight to fill the
// link the step running beside it slowed down by 24-52 % whatever the grid size (r03h_ingest_step.txt); the DMA
// engines move the same bytes without touching the CUs' memory pipelines.  `indices` is a HOST array.
extern "C" int pnmn_copy_rows_h2d(const void* store, const int64_t* indices, void* dst, int n, int64_t n_store,
                                  int64_t row_bytes, void* stream) {
    if (n <= 0) return 0;
    if (!store || !indices || !dst || n_store <= 0 || row_bytes <= 0) return PNMN_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int i = 0; i < n; ++i) {
        const int64_t row = indices[i];
        if (row < 0 || row >= n_store) return PNMN_EINVAL;
        const hipError_t e = hipMemcpyAsync(static_cast<char*>(dst) + (size_t)i * row_bytes,
                                            static_cast<const char*>(store) + (size_t)row * row_bytes, (size_t)row_bytes,
                                            hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}
