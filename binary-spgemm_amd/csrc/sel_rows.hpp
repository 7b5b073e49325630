// sel_rows.hpp -- device code that the entry-parallel passes share: the tile geometry, the 16-byte entry loads, the DPP join
// of a lane's four flags into the 64-bit flag word of 64 entries, the search of an entry's row in the tile's window of
// row_ptr (staged in LDS; tile_row comes from k_sel_tile_rows), the lower bound of a column in a row of another operand,
// the walk itself, and the intersection of two ascending rows on top of the two.  Who uses what:
//     sel_walk_entries   the walk over a tile's entries with an op (load / row / entry): k_merge_disjoint (bfs.hip),
//                        k_dot_count (dot.hip), k_lcc_weights, k_lcc_count (lcc.hip)
//     isect_lane,        the light intersection inside that walk and the list of the entries too long for it: k_dot_count,
//     IsectHeavy         k_lcc_count
//     IsectHeavyList,    the list as the second kernel reads it, and one wave's intersection of a listed entry: k_dot_heavy
//     isect_wave         (a plain grid stride over the list), k_lcc_heavy (chunks of the list, lcc.hip says why)
//     sel_sweep_graph    the same walk behind the graph adapter (range check, self-loop skip, changed / bad words) with
//                        an op (row / edge): k_cc_hook (cc.hip), k_scc_mark, k_scc_forward, k_scc_backward (scc.hip)
//     SelTileRows alone  k_set_flags (setop.hip): it also needs row_begin, the column in front of the lane's four and a
//                        flag word for the steps past E, so it keeps its own loop
//     the pieces         k_sel_flags_struct (select.hip) spells the staging out in its body, see SelTileRows
// Device code only.
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

// The entry-parallel walk.  A workgroup owns the kSelTile consecutive entries of tile blockIdx.x whatever rows they belong
// to, a wave kSelWaveSpan of them, a lane four per step by one 16-byte load of `col` (NT: non-temporal), all kSelSteps
// loads in flight before the first is used; the tile's window of row_ptr is staged in LDS -- a hub row costs what its
// entries cost.  One row search per lane and step, then a walk of the four entries that searches again when the row ends.
//     op.load(j, e)          before the walk, beside the column load of step j (entries e .. e + 3, e possibly past E):
//                            where an op issues 16-byte loads of its own
//     op.row(r)              whenever the lane enters row r
//     op.entry(r, p, c, s)   entry p of row r with column c; s = 4 * j + k, the lane's s-th entry (a constant once the loops
//                            are unrolled: it indexes what op.load fetched)
// Called by every thread of the workgroup (it holds the staging barrier); the grid is ceil(E / kSelTile).
template <bool NT, typename Op>
__device__ __forceinline__ void sel_walk_entries(const int *__restrict__ row_ptr, const int *__restrict__ col, int rows,
                                                 long long E, bool vec, const int *__restrict__ tile_row, Op &op)
{
    __shared__ int srp[kSelStage + 1];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const SelTileRows tr = sel_stage_tile_rows(row_ptr, rows, E, tile_row, srp);
    const long long w0 = (long long)blockIdx.x * kSelTile + w * kSelWaveSpan;
    v4i c4[kSelSteps];
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        c4[j] = load4<NT>(col, e, E, vec);
        op.load(j, e);
    }
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e0 = w0 + j * kSelGroup + 4 * lane;
        if (e0 >= E) continue;
        const int c[4] = {c4[j].x, c4[j].y, c4[j].z, c4[j].w};
        int r = tr.find(tr.rb, (int)e0);                                 // one search per lane and step, then a walk
        int end = tr.row_end(r);
        op.row(r);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long long p = e0 + k;
            if (p >= E) break;
            if (p >= end) {
                r = tr.find(r + 1, (int)p);
                end = tr.row_end(r);
                op.row(r);
            }
            op.entry(r, p, c[k], 4 * j + k);
        }
    }
}

// ------------------------------------------------------------------ row intersections (dot.hip, lcc.hip) ---
// The common elements of two strictly ascending rows.  An entry whose shorter row has at most T elements is intersected by
// its lane inside the walk (isect_lane); a longer one goes to a list {p, row} (IsectHeavy) that a second kernel walks, one
// wave per entry (IsectHeavyList, isect_wave).  What a hit is worth is the caller's: f(hit, place in x, place in y, column).
constexpr int kIsectWaves = kSelThreads / 64;
constexpr int kIsectDeep = 4;               // 64-element steps of the shorter row in flight per trip (kColDeep of color.hip)
constexpr int kIsectHeavyGrid = 2048;       // workgroups of a heavy kernel: 8192 waves (eight per SIMD of 256 CUs) share the list
constexpr int kIsectEntries = 4 * kSelSteps;   // entries a lane walks in sel_walk_entries

// One lane walks x[0, m) and searches y[0, ylen) from a lower bound that only advances; it ends when y is used up.
template <typename F>
__device__ __forceinline__ void isect_lane(const int *__restrict__ x, int m, const int *__restrict__ y, int ylen, F &&f)
{
    int lo = 0;
    for (int q = 0; q < m; q++) {
        const int c = x[q];
        lo = sel_lower_bound(y, lo, ylen, c);
        if (lo >= ylen) break;
        f(y[lo] == c, q, lo, c);
    }
}

// One wave: the lanes stride over x[0, xlen) 64 elements per step, DEEP steps in flight.  EVERY lane calls f for every slot
// of a trip, with hit == false (and nothing else of meaning) past the end of x, so f may ballot.  Wave-uniform control flow.
template <int DEEP, typename F>
__device__ __forceinline__ void isect_wave(const int *__restrict__ x, int xlen, const int *__restrict__ y, int ylen, int lane,
                                           F &&f)
{
    int from = 0;                                            // the lane's lower bound: its elements ascend from trip to trip
    // (ylen == 0 only with xlen == 0: the loop does not run and y is never read)
    for (int b = 0; b < xlen; b += 64 * DEEP) {
        int c[DEEP], lo[DEEP], hi[DEEP];
        bool in[DEEP];
#pragma unroll
        for (int q = 0; q < DEEP; q++) {
            in[q] = b + 64 * q + lane < xlen;
            c[q] = in[q] ? x[b + 64 * q + lane] : 0;
            lo[q] = from;
            hi[q] = in[q] ? ylen : from;
        }
        // the DEEP lower bounds in lockstep: one load each per round, all in flight together
        for (;;) {
            int mid[DEEP], v[DEEP];
            bool any = false;
#pragma unroll
            for (int q = 0; q < DEEP; q++) {
                mid[q] = lo[q] + ((hi[q] - lo[q]) >> 1);
                any |= lo[q] < hi[q];
                v[q] = lo[q] < hi[q] ? y[mid[q]] : 0;
            }
            if (!any) break;
#pragma unroll
            for (int q = 0; q < DEEP; q++) {
                if (lo[q] < hi[q]) {
                    if (v[q] < c[q]) lo[q] = mid[q] + 1;
                    else hi[q] = mid[q];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < DEEP; q++) {
            f(in[q] && lo[q] < ylen && y[lo[q]] == c[q], b + 64 * q + lane, lo[q], c[q]);
            if (in[q]) from = lo[q];
        }
    }
}

// The heavy entries of a lane of sel_walk_entries: an op notes them in entry(), the kernel appends them behind the walk.
struct IsectHeavy {
    unsigned mask;                      // bit s: the lane's s-th entry is heavy
    int row[kIsectEntries];             // its row
    __device__ __forceinline__ void note(int s, int r) { mask |= 1u << s, row[s] = r; }
    // {p, row} of every noted entry to list[*counter ...] (wave_append: ballot, one atomicAdd per wave, rank by popcount).
    // An entry is appended at most once, so the list never passes E entries; the store is bounded all the same.
    __device__ __forceinline__ void append(int2 *list, int *counter, long long E) const
    {
        if (__ballot(mask != 0u) == 0) return;                           // (wave-uniform)
        const int lane = lane_id(), w = threadIdx.x >> 6;
        const long long w0 = (long long)blockIdx.x * kSelTile + w * kSelWaveSpan;
#pragma unroll
        for (int s = 0; s < kIsectEntries; s++) {
            const long long p = w0 + (s >> 2) * kSelGroup + 4 * lane + (s & 3);  // the lane's s-th entry (sel_walk_entries)
            wave_append((mask >> s) & 1u, int2{(int)p, row[s]}, list, counter, E, lane);
        }
    }
};

// The list as a heavy kernel reads it: its length comes from device memory (the launch follows the count kernel on the
// stream, nothing in between appends), clamped to cap.
struct IsectHeavyList {
    const int2 *__restrict__ list;
    long long n, cap;
    int rows;
    __device__ __forceinline__ IsectHeavyList(const int2 *__restrict__ l, const int *counter, long long c, int r)
        : list(l), n(*counter > c ? c : *counter), cap(c), rows(r) {}
    // slot h < n: the wave-uniform entry p and its row i; false: skip the slot (the count kernel wrote neither)
    __device__ __forceinline__ bool entry(long long h, int &p, int &i) const
    {
        const int2 e = list[h];
        p = wave_first(e.x), i = wave_first(e.y);
        return (unsigned long long)p < (unsigned long long)cap && (unsigned)i < (unsigned)rows;
    }
};

// The two words that every graph sweep reports, at the head of the algorithm's flag block (CcFlags, SccFlags)
struct SweepFlags {
    unsigned changed;       // op.changed of any lane
    unsigned bad;           // a column outside [0, n)
};

// The walk over the entries of a graph (n x n): op.row(u) when the lane enters row u, op.edge(u, v) for every stored entry
// (u, v) with v in [0, n) and v != u.  A column outside [0, n) is tested BEFORE it reaches op, sets the `bad` word and is
// skipped.  op.changed ends up in the `changed` word.  Called by every thread of the workgroup.
template <typename Op>
struct SelGraphWalk {
    Op &op;
    int n;
    bool bad;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int u) { op.row(u); }
    __device__ __forceinline__ void entry(int u, long long, int v, int)
    {
        if ((unsigned)v >= (unsigned)n) bad = true;                      // before v indexes anything
        else if (v != u) op.edge(u, v);
    }
};

template <typename Op>
__device__ __forceinline__ void sel_sweep_graph(const int *__restrict__ row_ptr, const int *__restrict__ col, int n, long long E,
                                                bool vec, const int *__restrict__ tile_row, SweepFlags *__restrict__ flags,
                                                Op &op)
{
    SelGraphWalk<Op> g = {op, n, false};
    sel_walk_entries<true>(row_ptr, col, n, E, vec, tile_row, g);
    const u64 any_changed = __ballot(op.changed), any_bad = __ballot(g.bad);
    if (lane_id() == 0) {                                                // one lane per wave
        if (any_changed) flags->changed = 1u;
        if (any_bad) flags->bad = 1u;
    }
}

}  // namespace bsp
