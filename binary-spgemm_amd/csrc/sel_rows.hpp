// sel_rows.hpp -- device code that the entry-parallel passes of select.hip, setop.hip, bfs.hip and cc.hip share: the tile
// geometry, the 16-byte entry loads, the DPP join of a lane's four flags into the 64-bit flag word of 64 entries, the search
// of an entry's row in the tile's window of row_ptr (staged in LDS; tile_row comes from k_sel_tile_rows) and the lower bound
// of a column in a row of another operand.  Device code only.
#pragma once
#include "kernels.hpp"
#include "wave.hpp"

namespace bsp {

constexpr int kSelThreads = 256;                      // four waves
constexpr int kSelGroup = 256;                        // entries of one wave step: four per lane, four flag words
constexpr int kSelSteps = 4;                          // steps per wave: the 16-byte loads a lane has in flight
constexpr int kSelWaveSpan = kSelSteps * kSelGroup;   // consecutive entries of one wave
constexpr int kSelStage = 4096;                       // rows of the tile's row_ptr window that are staged in LDS
static_assert(kSelTile == 4 * kSelWaveSpan, "a workgroup's four waves cover one tile");

typedef int v4i __attribute__((ext_vector_type(4)));

// entries e .. e + 3 of p (e a multiple of four); vec: p is 16-byte aligned.  Entries at or past E read as 0.
template <bool NT>
__device__ __forceinline__ v4i load4(const int *__restrict__ p, long long e, long long E, bool vec)
{
    if (vec && e + 3 < E) {
        const v4i *q = reinterpret_cast<const v4i *>(p + e);
        return NT ? __builtin_nontemporal_load(q) : *q;
    }
    v4i v = {0, 0, 0, 0};
    if (e < E) v.x = p[e];
    if (e + 1 < E) v.y = p[e + 1];
    if (e + 2 < E) v.z = p[e + 2];
    if (e + 3 < E) v.w = p[e + 3];
    return v;
}

// The flag word of the 64 entries that a DPP row of 16 lanes holds, four per lane (nib: the lane's four flags): complete
// in lane 15 of the row.  The nibbles occupy disjoint bits, so the row's inclusive sum is their OR.  Full EXEC.
__device__ __forceinline__ u64 row_flag_word(unsigned nib, int lane)
{
    const int sh = 4 * (lane & 15);
    int lo = sh < 32 ? (int)(nib << sh) : 0;
    int hi = sh >= 32 ? (int)(nib << (sh - 32)) : 0;
    lo += dpp_or_zero<0x111, 0xF>(lo);
    hi += dpp_or_zero<0x111, 0xF>(hi);
    lo += dpp_or_zero<0x112, 0xF>(lo);
    hi += dpp_or_zero<0x112, 0xF>(hi);
    lo += dpp_or_zero<0x114, 0xF>(lo);
    hi += dpp_or_zero<0x114, 0xF>(hi);
    lo += dpp_or_zero<0x118, 0xF>(lo);
    hi += dpp_or_zero<0x118, 0xF>(hi);
    return ((u64)(u32)hi << 32) | (u64)(u32)lo;
}

__device__ __forceinline__ void store_flag_word(u64 word, long long first_entry, int lane, u64 *__restrict__ flags,
                                                int *__restrict__ cnt)
{
    if ((lane & 15) == 15) {
        const long long w = (first_entry >> 6) + (lane >> 4);
        flags[w] = word;
        cnt[w] = __popcll(word);
    }
}

// largest r in [lo, hi] with rp[r] <= e: the row that holds entry e (empty rows share their row_ptr with the next row)
template <typename P>
__device__ __forceinline__ int sel_row_of(P rp, int lo, int hi, int e)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rp[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// first position in [lo, hi) of y whose column is not below c
__device__ __forceinline__ int sel_lower_bound(const int *__restrict__ y, int lo, int hi, int c)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (y[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The rows of one tile of kSelTile entries.  Every entry of tile blockIdx.x lies in rows rb .. rl (tile_row: the row of
// each tile's first entry); their window of row_ptr is staged in LDS (srp: kSelStage + 1 ints) unless the tile spans more
// than kSelStage rows (mostly empty ones), which are then searched in row_ptr itself.  (k_sel_flags_struct spells the
// same steps out in its body: routed through this struct the compiler schedules that kernel differently, and its code is
// kept instruction for instruction.)
struct SelTileRows {
    const int *row_ptr;
    const int *srp;
    int rb, rl, span;
    bool staged;
    // the row at or after `lo` that holds entry e
    __device__ __forceinline__ int find(int lo, int e) const
    {
        return staged ? rb + sel_row_of(srp, lo - rb, span - 1, e) : sel_row_of(row_ptr, lo, rl, e);
    }
    __device__ __forceinline__ int row_begin(int r) const { return staged ? srp[r - rb] : row_ptr[r]; }
    __device__ __forceinline__ int row_end(int r) const { return staged ? srp[r - rb + 1] : row_ptr[r + 1]; }
};

// called by every thread of the workgroup (it holds a barrier); the grid is ceil(E / kSelTile)
__device__ __forceinline__ SelTileRows sel_stage_tile_rows(const int *__restrict__ row_ptr, int rows, long long E,
                                                           const int *__restrict__ tile_row, int *srp)
{
    const long long b0 = (long long)blockIdx.x * kSelTile;               // < E
    const bool last = b0 + kSelTile >= E;
    SelTileRows t;
    t.row_ptr = row_ptr;
    t.srp = srp;
    t.rb = tile_row[blockIdx.x];
    t.rl = last ? rows - 1 : tile_row[blockIdx.x + 1];
    t.span = t.rl - t.rb + 1;
    t.staged = t.span <= kSelStage;                                      // (else: mostly empty rows)
    if (t.staged)
        for (int q = threadIdx.x; q <= t.span; q += kSelThreads) srp[q] = row_ptr[t.rb + q];
    __syncthreads();
    return t;
}

}  // namespace bsp
