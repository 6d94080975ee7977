// Hand-off primitives shared by the multi-CU recurrent kernels (seq2seq.hip, lstm_stack.hip, decoder_multi.hip).
//
// S workgroups that share one 16-row tile step in lockstep; between phases they exchange small vectors
// through L2.  One monotonic counter per tile: every member adds 1 per hand-off, so after the k-th
// hand-off the counter reads S * k -- no reset, no ABA.
//   signal: this wave's stores have reached L2 (s_waitcnt vmcnt(0)) -> workgroup barrier -> ONE
//           increment of the counter (agent-scope release)
//   wait:   thread 0 spins on the counter (bounded: a trap, not a hung GPU, if the partners never show
//           up -- the grid is sized by the host so that every member is resident), one agent-scope
//           acquire (also invalidates this CU's vector L1, which all waves of the workgroup share), barrier
// blockIdx -> (tile, member) keeps a tile's members on one XCD (dispatch is round-robin over the 8
// XCDs), which makes the exchange an L2 hit; correctness does not depend on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

namespace pnmn {

// ---- the pieces of a hand-off: each exists once, here ----------------------------------------------------------------
// A tile's counter LINE is 64 ints (CLUSTER_COUNTER_STRIDE) of the per-stream block below, five of them in use:
//   [0] arrivals of the tile's own members (monotonic)
//   [1] start vote of an unlinked tile: OR of (1 << XCC id) over the members | members started << 16
//   [2] members that finished
//   [3] cross arrivals: the members of a PRODUCER tile count here, in their consumer's line (lstm_stack.hip)
//   [4] start vote of a LINKED pair, in the consumer's line (both tiles' members: 2 S of them)
// Cluster (a tile on its own) uses [0..2]; lstm_stack.hip's Sync adds [3] and [4].  Every launch leaves every line it
// used zeroed (handoff::finish), whichever of the two ran: they share the block, and the next launch on the stream
// may be the other one.
namespace handoff {

// One thread: wait until (word >> shift) >= target.  Bounded: a trap, not a hung GPU, if the others never show up.
__device__ __forceinline__ void spin_until(int* word, int target, int shift = 0) {
    int spins = 0;
    while ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> shift) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 26)) __builtin_trap();
    }
}

// Whole workgroup, in front of publish(): this wave's stores have reached L2, and so have every other wave's.
__device__ __forceinline__ void stores_out() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// One thread: one more arrival at `word`.  `fast` (all members on one XCD, see vote()): L2 is the members' common
// coherence point, so a hand-off needs neither the L2 write-back of an agent-scope release nor the L2 invalidate of an
// agent-scope acquire -- only "my stores have reached L2" on one side and "drop this CU's L1" on the other.  Measured
// on MI355X the agent-scope pair costs 6-9 us per hand-off with 256 workgroups resident (every release writes back all
// of the XCD's dirty output lines); the same-XCD pair costs a fraction of that.
__device__ __forceinline__ void publish(int* word, bool fast) {
    if (fast)
        __hip_atomic_fetch_add(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        __hip_atomic_fetch_add(word, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// Whole workgroup: thread 0 waits for `target` arrivals at `word`, one acquire (which also drops this CU's vector L1,
// shared by all waves of the workgroup), barrier.
__device__ __forceinline__ void await(int* word, int target, bool fast) {
    if (threadIdx.x == 0) {
        spin_until(word, target);
        if (fast)
            asm volatile("buffer_inv sc0\n\ts_waitcnt vmcnt(0)" ::: "memory");  // this CU's vector L1 only
        else
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

// Start of a launch, whole workgroup: the `expect` members that share `word` publish the XCD they run on and all take the
// same decision: true = all on one XCD.  ONE word carries both the OR of (1 << XCC id) (low half) and the number of
// members that have published (high half): a member's two relaxed read-modify-writes of that word are ordered (same
// address), so whoever reads the full count also reads every member's bit -- no release / acquire pair, which with 256
// workgroups resident costs 6-9 us per launch (an agent-scope release writes back the XCD's dirty lines; a step has ~20
// such launches).  Nothing else is published here: what the members read of earlier kernels is ordered by the kernel
// boundary.
__device__ __forceinline__ bool vote(int* word, int expect) {
    if (threadIdx.x == 0) {
        const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;  // HW_REG_XCC_ID[3:0]
        __hip_atomic_fetch_or(word, 1 << xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(word, 1 << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        spin_until(word, expect, 16);
    }
    __syncthreads();
    // (the word only grows until the finish() of the last member of the line that holds it: whoever reads it now reads
    // every member's bit)
    return __builtin_popcount(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xFFFF) == 1;
}

// Last act of a member.  The member of the line that finishes last puts the line's first `words` words back to zero,
// so the next launch on the stream finds the block as the library created it and no zeroing dispatch has to go in front
// of every launch (16 per training step).  Every member has passed its last await() when it gets here, so nobody polls
// the words any more; vmcnt(0) first: this member's last publish() has been performed.
__device__ __forceinline__ void finish(int* line, int members, int words) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int before = __hip_atomic_fetch_add(line + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == members - 1)
            for (int k = 0; k < words; ++k) __hip_atomic_store(line + k, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace handoff

// Hand-off state of one workgroup of a tile on its own: `members` workgroups, one counter, `fast` decided once per launch.
struct Cluster {
    int* counter;   // the tile's line (words [0..2])
    int handoffs;
    int members;
    bool fast;

    __device__ __forceinline__ void start(int* tile_counter, int n_members) {
        counter = tile_counter;
        handoffs = 0;
        members = n_members;
        fast = handoff::vote(counter + 1, members);
    }

    __device__ __forceinline__ void signal() {
        handoff::stores_out();
        if (threadIdx.x == 0) handoff::publish(counter, fast);
    }

    __device__ __forceinline__ void wait() { handoff::await(counter, members * ++handoffs, fast); }

    __device__ __forceinline__ void finish() { handoff::finish(counter, members, 3); }
};

// (tile, member) of this workgroup for a grid of 8 * S * ceil(tiles / 8) workgroups
template <int S>
__device__ __forceinline__ void cluster_coords(int& tile, int& member) {
    const int slot = blockIdx.x >> 3;
    tile = (blockIdx.x & 7) + 8 * (slot / S);
    member = slot % S;
}

// CUs the multi-CU kernels leave alone.  A data-parallel run keeps RCCL's workgroups (one per channel, resident
// for the whole collective, waiting for their PEERS) off the CUs these kernels size their grids for: a grid that
// needs every CU while part of the chip is held by a kernel that itself waits is what stalled round 1.
// Set by pnmn_cluster_reserve_cus() or PNMN_CLUSTER_RESERVE_CUS; one instance per library (inline, C++17).
inline int& cluster_reserved_cus() {
    static int reserved = [] {
        const char* e = getenv("PNMN_CLUSTER_RESERVE_CUS");
        const int v = e ? atoi(e) : 0;
        return v > 0 ? v : 0;
    }();
    return reserved;
}

inline int physical_cus() {
    // cached per device: the design is one process per GPU, but a process that drives several devices must
    // not size a grid for device 1 from device 0's CU count
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus[dev] = -1;
    return cus[dev];
}

// CUs a multi-CU launch may count on (physical minus the reserve, never fewer than 32 of a real device)
inline int device_cus() {
    const int cus = physical_cus();
    if (cus <= 0) return cus;
    const int left = cus - cluster_reserved_cus();
    return left >= 32 ? left : (cus < 32 ? cus : 32);
}

// Largest number of 16-row tiles ONE multi-CU launch can take (four members per tile); 0 = none.
inline int cluster_max_tiles() {
    const int cus = device_cus();
    return cus >= 32 ? 8 * (cus / 32) : 0;
}

// Members per tile such that the whole grid is resident with one workgroup per CU; 0 = does not fit.
inline int cluster_split(int tiles, bool allow4 = true) {
    const int cus = device_cus();
    if (cus <= 0) return 0;
    const int groups = (tiles + 7) / 8;
    if (8 * groups * 8 <= cus) return 8;
    if (allow4 && 8 * groups * 4 <= cus) return 4;
    return 0;
}

// One counter line per tile, each on its own 256-byte line: the members of up to 128 tiles poll and increment
// concurrently, and counters sharing a line would serialise all of them on one L2 channel.
//
// The lines live in a block the LIBRARY owns, one per (device, stream), zeroed once when it is created; the
// kernels leave it zeroed (handoff::finish), and launches on one stream run one after the other.  Only while
// the stream is being captured into a hipGraph do the counters go into the caller's workspace behind a
// zeroing KERNEL (a replayed graph may run next to eager launches of the stream it was captured on; and a
// memset node was seen to run out of order with the kernel nodes around it -- kernel nodes keep stream order).
static __global__ void cluster_zero_kernel(int* words, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) words[i] = 0;
}

constexpr int CLUSTER_COUNTER_STRIDE = 64;                                     // ints
constexpr size_t CLUSTER_SYNC_BYTES = 128 * CLUSTER_COUNTER_STRIDE * sizeof(int);  // up to 128 tiles

// The counter block a launch on `stream` uses; `workspace` = the caller's (>= CLUSTER_SYNC_BYTES), used under capture.
inline hipError_t cluster_sync_block(void* workspace, hipStream_t stream, int** out) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(stream, &cap);
    if (e != hipSuccess) return e;
    if (cap != hipStreamCaptureStatusNone) {
        *out = static_cast<int*>(workspace);
        hipLaunchKernelGGL(cluster_zero_kernel, dim3(8), dim3(256), 0, stream, *out, (int)(CLUSTER_SYNC_BYTES / sizeof(int)));
        return hipGetLastError();
    }
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, int*> blocks;
    int dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    int*& b = blocks[{dev, stream}];
    if (!b) {
        void* p = nullptr;
        if ((e = hipMalloc(&p, CLUSTER_SYNC_BYTES)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(p, 0, CLUSTER_SYNC_BYTES, stream)) != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
        b = static_cast<int*>(p);
    }
    *out = b;
    return hipSuccess;
}

}  // namespace pnmn
