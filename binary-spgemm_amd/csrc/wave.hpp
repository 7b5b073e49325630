// wave.hpp -- wave64 primitives for gfx950 (CDNA4).  Device code only.
//
// Everything here assumes a 64-lane wavefront and full EXEC (call from wave-uniform control
// flow only).  Scans use DPP row shifts + row broadcasts (the GFX9 cross-lane path that needs no
// LDS traffic), because the accumulator kernels keep the LDS pipe busy with atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsp {

typedef unsigned long long u64;
typedef unsigned int u32;

__device__ __forceinline__ int lane_id()
{
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// mix32 of include/bspgemm.h: the hash behind every seeded order and weight.  Part of the public contract; written once.
__device__ __forceinline__ u32 mix32(u32 x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// bits below / up to and including this lane
__device__ __forceinline__ u64 mask_lt(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ u64 mask_le(int lane) { return (2ull << lane) - 1ull; }

// DPP controls (GFX9): row_shr:n = 0x110+n, row_bcast:15 = 0x142, row_bcast:31 = 0x143
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_or_zero(int x)
{
    // lanes without a valid source, or rows masked out, receive `old` = 0
    return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xF, false);
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int wave_incl_scan(int x)
{
    x += dpp_or_zero<0x111, 0xF>(x);   // row_shr:1
    x += dpp_or_zero<0x112, 0xF>(x);   // row_shr:2
    x += dpp_or_zero<0x114, 0xF>(x);   // row_shr:4
    x += dpp_or_zero<0x118, 0xF>(x);   // row_shr:8   -> scan inside each row of 16
    x += dpp_or_zero<0x142, 0xA>(x);   // row_bcast:15 into rows 1 and 3
    x += dpp_or_zero<0x143, 0xC>(x);   // row_bcast:31 into rows 2 and 3
    return x;
}

__device__ __forceinline__ int wave_bcast(int x, int lane)   // lane must be wave-uniform
{
    return __builtin_amdgcn_readlane(x, lane);
}

__device__ __forceinline__ u64 wave_bcast64(u64 x, int lane)
{
    u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)x, lane);
    u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(x >> 32), lane);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ int wave_first(int x) { return __builtin_amdgcn_readfirstlane(x); }

// 64-bit inclusive scan for the (cold) device-wide scans; LDS-crossbar shuffles are fine there
__device__ __forceinline__ long long wave_incl_scan64(long long x)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        long long y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// orders this wave's LDS traffic for the compiler between phases that hand data from lane to
// lane through LDS.  DS operations of one wave execute in issue order, so no hardware barrier is
// needed; the fence only stops the compiler from moving accesses across the phase boundary.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Blocked scan of a slot array of 64*W words: lane l owns the W consecutive words [l*W, l*W+W)
// (vector LDS reads), does its own running popcount in registers, ONE wave scan joins the lanes,
// and the W prefixes go back as one vector store.  pre[t] = number of set bits in P[0..t).
// Cost is fixed per row (the arrays are zero beyond the live slots) and replaces a loop of
// ceil(n/64) dependent scan steps.
template <int W>
__device__ __forceinline__ int scan_blocked(const u32 *P, unsigned short *pre, int lane)
{
    u32 x[W];
#pragma unroll
    for (int k = 0; k < W; k++) x[k] = P[lane * W + k];
    int e[W];
    int run = 0;
#pragma unroll
    for (int k = 0; k < W; k++) {
        e[k] = run;
        run += __popc(x[k]);
    }
    const int inc = wave_incl_scan(run);
    const int base = inc - run;
#pragma unroll
    for (int k = 0; k < W; k++) pre[lane * W + k] = (unsigned short)(base + e[k]);
    return wave_bcast(inc, 63);
}

// Staging index swizzle: lanes write runs of ~W consecutive outputs, i.e. at a stride of ~W words
// (8-way bank conflicts at stride 8); XOR-ing the low 5 bits with the next 5 spreads any such
// stride over all 32 banks and keeps the final contiguous read-out conflict-free.
__device__ __forceinline__ int stage_swz(int x) { return x ^ ((x >> 5) & 31); }

template <int W>
__device__ __forceinline__ void clear_blocked(u32 *P, int lane)
{
#pragma unroll
    for (int k = 0; k < W; k++) P[lane * W + k] = 0u;
}

// sum / maximum / minimum of x over the wave, in every lane (xor shuffles, off = 32 .. 1); T: int, long long, u64
template <typename T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_max(T x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_min(T x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, 64));
    return x;
}

// the wave's lanes with `take` append `v` to list[*size ...]: one atomic per wave, the lane's rank by its mask of lower
// lanes.  The store is bounded by `cap` entries (C: int or long long, compared in its own width) whatever *size holds; a
// caller whose list cannot pass `cap` says why at its call.  list is not __restrict__: a launch may read the list plainly
// elsewhere.
template <typename T, typename C>
__device__ __forceinline__ void wave_append(bool take, T v, T *list, int *size, C cap, int lane)
{
    const u64 m = __ballot(take);
    if (m == 0) return;                                      // (wave-uniform)
    int base = 0;
    if (lane == 0) base = atomicAdd(size, __popcll(m));
    base = wave_first(base);
    const int at = base + __popcll(m & mask_lt(lane));
    // (the test stands inside the condition in either width: computed into a bool first, or widened for both, it compiles
    // to other code in the callers)
    if constexpr (sizeof(C) == 8) {
        if (take && (unsigned long long)at < (unsigned long long)cap) list[at] = v;
    } else {
        if (take && (unsigned)at < (unsigned)cap) list[at] = v;
    }
}

// the wave's count of `x` added to *word by one atomic
__device__ __forceinline__ void wave_count(bool x, int *word, int lane)
{
    const u64 m = __ballot(x);
    if (m && lane == 0) atomicAdd(word, __popcll(m));
}

// the workgroup's count of `x` added to *word (and *also, unless NULL) by one atomic each; wsum: THREADS / 64 ints of LDS.
// Called by every thread of the workgroup (THREADS of them).
template <int THREADS>
__device__ __forceinline__ void block_add(bool x, int *word, int *also, int *wsum)
{
    const u64 m = __ballot(x);
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int q = 0; q < THREADS / 64; q++) s += wsum[q];
        if (s) atomicAdd(word, s);
        if (s && also) atomicAdd(also, s);
    }
    __syncthreads();                                                     // (wsum is free again)
}

// the workgroup's minimum of x, valid in thread 0 ALONE: the caller sends it on by one atomic.  part: THREADS / 64 words of
// LDS, not free again before the caller's next barrier.  Called by every thread of the workgroup (THREADS of them).  (There
// is no block_max: its one candidate, k_sssp_finish, shares block_add's barriers and keeps its open code.)
template <int THREADS>
__device__ __forceinline__ u64 block_min(u64 x, u64 *part)
{
    x = wave_min(x);
    if (lane_id() == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < THREADS / 64; q++) x = min(x, part[q]);
    }
    return x;
}

}  // namespace bsp
