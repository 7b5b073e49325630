// wave_rows.inc -- the hot kernel: one wavefront per A-row, rank-bitmap accumulator in LDS.
// Compiled once per (LEVELS, mode) pair by the Makefile (parallel builds); wave_rows.hip dispatches to those objects.
//
// Replaces the body of SpGEMM_bigslice (final/SpGEMM_mpi_omp.c:24-52) for rows whose product
// count F_i fits one wave's capacity (<= 2048):
//     reference                                      here
//     xb[k] dense byte flags, one per column (:21)   hierarchy of 32-bit bitmaps in LDS
//     test-and-set + unsorted append (:38-42)        ds_or_b32 on the bitmaps (set union)
//     quickSort of the row (:47)                     none: slots are addressed by RANK, so the
//                                                    emit pass walks them in ascending order
//     sparse reset of xb (:48-50)                    slots/top words cleared as they are consumed
//
// Accumulator ("rank bitmap", an order-preserving perfect hash of the row's columns):
//   A column c is split into 5-bit digits.  The TOP bitmap is addressed directly by the high
//   digits (<= 256 32-bit words).  Every set bit of a level owns one 32-bit slot of the level
//   below; the slot index is the bit's rank = prefix popcount, so slots are dense (<= F_i of
//   them: LDS use is proportional to the row and independent of n) and in ascending column
//   order.  Level 0 slots are the 32-column masks of the result row.  Building it takes LEVELS
//   sweeps over the row's products, which stay in registers (col[], rank[]).
//   Per product: one B.col_idx load, LEVELS ds_or_b32, LEVELS-1 (ds_read_b32 + ds_read_u16);
//   rank = v_bcnt_u32_b32(word & below, prefix) -- popcount and add in one instruction.
//   32-bit words (not 64): every mask op is a single full-rate VALU instruction and the slot
//   arrays take 14 B of LDS per product of capacity, which is what sets the occupancy.
//
// Gather: the F_i products of a row are the concatenation of the B rows selected by A's row.
//   The prepass left ab[jj] = (start, length) of the B row behind every A-nonzero, so lanes read
//   the extents coalesced; a wave scan turns lengths into product offsets, a "starts" bitmap
//   marks where each B row begins in product order, and product p finds its source by popcount
//   of the starts below p -- all 64 lanes load B.col_idx every step whatever the B row lengths.
//
// Latency: a wave owns 16 consecutive records of its capacity class.  The records (row, A
//   offset, |A_i|, output offset) are loaded once, coalesced; the (start,length) pairs of row
//   k+1 are prefetched while row k is processed; what stays exposed per row is the single
//   B.col_idx gather (covered by the other waves of the CU).  LDS arrays are separate
//   __shared__ objects so the compiler may batch the reads of all chunks ahead of the atomics;
//   lanes past the end of the row in the last chunk are masked off for every LDS atomic/store
//   (parking them on a spare slot serialises up to 63 same-address atomics per instruction).
//
// Output: row i's sorted columns go to tmp[Fprefix[i] ..), its count to cnt[i]; the compaction
// kernel squeezes the rows together once C.row_ptr is known.
//
// Roofline: HBM (gather of B.col_idx, 4 B per product, + 4 B per output written).  No MFMA.
#include "kernels.hpp"
#include "wave.hpp"

namespace bsp {

// waves resident per CU for a workgroup of `w` waves using `bytes` of LDS per wave
constexpr int waves_per_cu(int w, int bytes) { return (w * bytes > 64 * 1024) ? 0 : (160 * 1024 / (w * bytes)) * w; }

// chunks of the class below the one with `chunks` chunks (0 below the first)
constexpr int prev_wave_chunks(int chunks)
{
    int prev = 0;
    for (int b = 1; b <= kWaveBins; b++) {
        if (kWaveChunks[b] == chunks) return prev;
        prev = kWaveChunks[b];
    }
    return 0;
}

template <int LEVELS, int CHUNKS, int TWP>   // TWP = top-bitmap words per lane (top = 64*TWP words)
struct WaveCfg {
    static constexpr int CAP = 64 * CHUNKS;                        // products (and outputs) per row
    // slot words per lane of the blocked scans/clears/emit: a multiple of 4 so that every lane's run
    // is whole 16-byte vectors whatever CHUNKS is (the classes step by one chunk)
    static constexpr int SW = (CHUNKS <= 2) ? CHUNKS : ((CHUNKS + 3) & ~3);
    static constexpr int SLOTS = 64 * SW;
    static constexpr int TOPW = 64 * TWP;
    static constexpr int bytes_per_wave = 4 * TOPW + 2 * TOPW + 8 * CHUNKS + 4 * SLOTS         // top, topPre, starts, L0w
                                          + (LEVELS >= 2 ? 4 * SLOTS : 16)                       // SA
                                          + (LEVELS >= 3 ? 4 * SLOTS + 2 * SLOTS : 32)           // SB, preB
                                          + (LEVELS >= 4 ? 2 * SLOTS : 16);                      // preA
    // workgroup size that keeps the most waves resident (LDS is what limits occupancy here)
    static constexpr int w4 = waves_per_cu(4, bytes_per_wave), w2 = waves_per_cu(2, bytes_per_wave);
    static constexpr int WAVES = (w4 >= w2 && w4 > 0) ? 4 : (w2 > 0 ? 2 : 1);
    // consecutive class-list rows per wave: the big classes have few rows, shorter runs fill the chip
    static constexpr int RPW = (CHUNKS >= 16) ? kRowsPerWave / 2 : kRowsPerWave;
    // chunks that are full for EVERY row of the class: the classes are exact segments of F (bin_of,
    // prepass.hip), so a row here has more products than the class below holds -- no tail-lane mask,
    // no exec save/restore around the atomics of those chunks
    static constexpr int FULL = prev_wave_chunks(CHUNKS);
};

// Streams the staged row (n <= 64*CHUNKS words of LDS) to `out` with EXACTLY `CHUNKS` store
// instructions whatever n is: the buffer descriptor's range check drops lanes past the end
// instead of an exec mask + branch.  gfx9 counts stores in vmcnt, in issue order with the loads; a
// static number of stores after the next row's prefetch lets the compiler wait for that
// prefetch with vmcnt(CHUNKS) rather than vmcnt(0), i.e. without waiting for these stores to be
// acknowledged by L2 at the top of every row.  The stores are NON-TEMPORAL (aux bit 1 = nt on gfx940+): a row is
// written once and read once, by the compaction or by the caller, and is never re-read from L2 -- streamed, it leaves
// the B rows in the cache (numeric phase 3.58 -> 3.40 ms, `profiles/r03_ab_cache_hints.log`; only for full-wave
// coalesced stores: the heavy-row kernels' scattered 4-byte stores get 2.5x slower with the same hint).
template <int CHUNKS, bool SWZ>
__device__ __forceinline__ void store_row(int *out, int n, const u32 *stage, int lane)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)out, (short)0, n * 4, 0x00020000);
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        const int t = c * 64 + lane;
        __builtin_amdgcn_raw_buffer_store_b32(stage[SWZ ? stage_swz(t) : t], rs, t * 4, 0, 2);
    }
}

// an extent is read exactly once per pass: streamed past L2, it leaves the B rows in the cache
__device__ __forceinline__ int2 load_extent(const int2 *p)
{
    const long long v = __builtin_nontemporal_load(reinterpret_cast<const long long *>(p));
    return make_int2((int)(u32)v, (int)(u32)((u64)v >> 32));
}

// EXCL: drops the columns of F's row (Fcol[f0 .. f0 + mlen): unsorted, repeats and columns outside the row allowed) from
// the staged sorted row -- n >= 1 columns, position p at stage[SWZ ? stage_swz(p) : p] -- and squeezes it together in place;
// returns the kept count.  Lane l takes mask columns l, l + 64, ... (coalesced, 64 * kDropBatch per trip) and finds each by a
// branch-free binary search of the staging (<= 12 LDS reads at 2048 entries); a hit sets the position's bit in `hit` (>= n / 32
// words, all zero; left all zero).  One pass over the staging, 64 positions per step, then moves every kept column down by
// the hits before it: a position is only ever written after it was read (kept columns move down, never up).
constexpr int kDropBatch = 4;
template <int CHUNKS, bool SWZ>
__device__ __forceinline__ int drop_mask_cols(u32 *stage, int n, u32 *hit, const int *__restrict__ Fcol, int f0, int mlen, int lane)
{
    auto at = [](int p) { return SWZ ? stage_swz(p) : p; };
    const u32 lo = stage[at(0)], hi = stage[at(n - 1)];            // the row's column range
    const int top = 1 << (31 - __builtin_clz((u32)n));             // largest power of two <= n
    bool any = false;
    for (int k0 = 0; k0 < mlen; k0 += 64 * kDropBatch) {           // (wave-uniform)
        u32 mc[kDropBatch];
#pragma unroll
        for (int u = 0; u < kDropBatch; u++) {
            const int k = k0 + u * 64 + lane;
            mc[u] = k < mlen ? (u32)Fcol[f0 + k] : 0xffffffffu;   // (a negative or absent column is above every column)
        }
        bool in[kDropBatch], some = false;
#pragma unroll
        for (int u = 0; u < kDropBatch; u++) {
            in[u] = mc[u] >= lo && mc[u] <= hi;
            some |= in[u];
        }
        if (!__ballot(some)) continue;                             // (wave-uniform) nothing of this batch within the row's range
        int pos[kDropBatch];
#pragma unroll
        for (int u = 0; u < kDropBatch; u++) pos[u] = 0;           // lower bound: staged columns below mc[u]
        for (int st = top; st > 0; st >>= 1) {
#pragma unroll
            for (int u = 0; u < kDropBatch; u++) {
                const int q = pos[u] + st;
                const u32 v = stage[at((q <= n ? q : n) - 1)];
                pos[u] = (q <= n && v < mc[u]) ? q : pos[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kDropBatch; u++) {
            if (in[u] && stage[at(pos[u])] == mc[u]) {             // (in range: pos < n)
                atomicOr(&hit[pos[u] >> 5], 1u << (pos[u] & 31));
                any = true;
            }
        }
    }
    if (!__ballot(any)) return n;                                  // (wave-uniform) no column of the row is masked
    wave_lds_fence();
    const u64 *hit64 = reinterpret_cast<const u64 *>(hit);
    int kept = 0;
    for (int c = 0; c * 64 < n; c++) {                             // (wave-uniform)
        const int left = n - c * 64;
        const u64 valid = left >= 64 ? ~0ull : mask_lt(left);
        const u64 keep = valid & ~hit64[c];
        if (keep != valid || kept != c * 64) {                     // else: nothing moves in this step
            const u32 v = stage[at(c * 64 + lane)];                // (c * 64 + lane < CAP: n <= CAP, a multiple of 64)
            if ((keep >> lane) & 1ull) stage[at(kept + __popcll(keep & mask_lt(lane)))] = v;
        }
        kept += __popcll(keep);
    }
    wave_lds_fence();
    if (lane * 32 < n) hit[lane] = 0u;
    wave_lds_fence();
    return kept;
}

// COUNT instances, round 4: a HASH FILTER in front of the sweeps.  The count pass only has to answer "how many of the row's
// products repeat an earlier column", and on most inputs the answer is none (98 % of the rows of the bench matrix).  Every
// product test-and-sets ONE bit of a hash bitmap (all of SA: 32 bits per product of capacity; one returning ds_or): a product
// that finds its bit clear is the first with its column for certain.  The few that find it set ("ambiguous": a true repeat or
// a hash collision, ~F/64 of them) are settled exactly, one by one, by comparing their column with every product of the
// row in registers: an ambiguous product repeats an earlier column iff an equal product exists that is not ambiguous (it
// set the bit) or is ambiguous and earlier in (chunk, lane) order.  No sweep, no scan, no ranked level: 1 LDS access per
// product instead of 4.  A row with more than kMaxAmbiguous of them (many repeats: the comparisons would cost more than
// the sweeps) takes the sweeps below.
constexpr int kMaxAmbiguous = 12;
constexpr int wr_floor_log2(int x) { int k = 0; while ((2 << k) <= x) k++; return k; }

// COUNT: the symbolic twin -- the same sweeps, nothing emitted: a row whose products all sit alone in their
// 32-column slots (known after the scan of the level above: nslots0 == F) has |C_i| = F_i without its
// level-0 masks being touched; only the others run the level-0 ORs and count their bits.  cnt[] is the result.
// Body: wave_rows_body.inc
template <int LEVELS, int CHUNKS, int TWP, bool COUNT>
__global__ __launch_bounds__((64 * WaveCfg<LEVELS, CHUNKS, TWP>::WAVES))
void k_wave_rows(const int2 *__restrict__ ab, const int *__restrict__ Bcol,
                 const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                 const long long *__restrict__ row_ptr,
                 int nrows, int rpw, int row_begin, int *__restrict__ tmp, int *__restrict__ cnt,
                 unsigned *__restrict__ err)
{
    constexpr bool EXCL = false, ACC = false;
    const int *Frow = nullptr, *Fcol = nullptr;
    const int cols = 0;
#define BSP_WAVE_GATHER(c, g) Bcol[g]
#define BSP_WAVE_OK(x, c) x
#include "wave_rows_body.inc"
}

// C = !F .* (A*B) for the rows of one class: the numeric kernel above with the columns of F's row (Frow / Fcol, absolute
// row ids) dropped before each row is stored; placed at its upper-bound offset (recpre), |C_i| to cnt
template <int LEVELS, int CHUNKS, int TWP>
__global__ __launch_bounds__((64 * WaveCfg<LEVELS, CHUNKS, TWP>::WAVES))
void k_wave_rows_excl(const int2 *__restrict__ ab, const int *__restrict__ Bcol,
                      const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                      int nrows, int rpw, int row_begin, int *__restrict__ tmp, int *__restrict__ cnt,
                      unsigned *__restrict__ err, const int *__restrict__ Frow, const int *__restrict__ Fcol)
{
    constexpr bool COUNT = false, EXCL = true, ACC = false;
    const long long *row_ptr = nullptr;
    const int cols = 0;
#define BSP_WAVE_GATHER(c, g) Bcol[g]
#define BSP_WAVE_OK(x, c) x
#include "wave_rows_body.inc"
}

// C = D | (A*B) for the rows of one class (Drow / Dcol: D's CSR, absolute row ids): the numeric kernel above with D's row
// as one more source of the gather, after the B rows -- its columns below `cols` are accumulated like products, the others
// lose their valid bit; placed at its upper-bound offset (recpre), |C_i| to cnt
template <int LEVELS, int CHUNKS, int TWP>
__global__ __launch_bounds__((64 * WaveCfg<LEVELS, CHUNKS, TWP>::WAVES))
void k_wave_rows_acc(const int2 *__restrict__ ab, const int *__restrict__ Bcol,
                     const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                     int nrows, int rpw, int row_begin, int *__restrict__ tmp, int *__restrict__ cnt,
                     unsigned *__restrict__ err, const int *__restrict__ Drow, const int *__restrict__ Dcol, int cols)
{
    constexpr bool COUNT = false, EXCL = false, ACC = true;
    const long long *row_ptr = nullptr;
    const int *Frow = Drow, *Fcol = Dcol;
#define BSP_WAVE_GATHER(c, g) (dsrc[c] ? Dcol : Bcol)[g]
#define BSP_WAVE_OK(x, c) ((x) && !dsrc[c])
#include "wave_rows_body.inc"
}

// MODE Drop: the complemented-mask twin, Insert: the accumulate twin (Frow / Fcol: F's or D's CSR; numeric, upper-bound
// placement only)
template <int LEVELS, int CHUNKS, int TWP, MaskMode MODE>
static void launch_cfg(const int2 *ab, const int *Bcol, int cols, const RowRec *rec,
                       const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                       unsigned *err, hipStream_t s, bool count, const int *Frow, const int *Fcol)
{
    using Cfg = WaveCfg<LEVELS, CHUNKS, TWP>;
    // rows per wave: the class maximum when the class has rows to spare; a class with few rows is
    // spread over (at least) kSpreadWaves waves so that its launch is not a handful of long-running waves
    constexpr int kSpreadWaves = 256 * 8;
    int rpw = (int)((nrows + kSpreadWaves - 1) / kSpreadWaves);
    if (rpw > Cfg::RPW) rpw = Cfg::RPW;
    if (rpw < 1) rpw = 1;
    const long long rows_per_wg = (long long)Cfg::WAVES * rpw;
    const int grid = (int)((nrows + rows_per_wg - 1) / rows_per_wg);
    if constexpr (MODE == MaskMode::Drop)
        hipLaunchKernelGGL((k_wave_rows_excl<LEVELS, CHUNKS, TWP>), dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                           ab, Bcol, rec, recpre, nrows, rpw, row_begin, tmp, cnt, err, Frow, Fcol);
    else if constexpr (MODE == MaskMode::Insert)
        hipLaunchKernelGGL((k_wave_rows_acc<LEVELS, CHUNKS, TWP>), dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                           ab, Bcol, rec, recpre, nrows, rpw, row_begin, tmp, cnt, err, Frow, Fcol, cols);
    else if (count)
        hipLaunchKernelGGL((k_wave_rows<LEVELS, CHUNKS, TWP, true>), dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                           ab, Bcol, rec, recpre, row_ptr, nrows, rpw, row_begin, tmp, cnt, err);
    else
        hipLaunchKernelGGL((k_wave_rows<LEVELS, CHUNKS, TWP, false>), dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                           ab, Bcol, rec, recpre, row_ptr, nrows, rpw, row_begin, tmp, cnt, err);
}

template <int LEVELS, int CHUNKS, MaskMode MODE>
static void launch_one(const int2 *ab, const int *Bcol, int cols, int topw, const RowRec *rec,
                       const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                       unsigned *err, hipStream_t s, bool count, const int *Frow, const int *Fcol)
{
    // the top bitmap is sized to what the column count needs: 128 or 256 words; 512 at three
    // levels (wave_levels_for_cols)
    if (topw <= 128) launch_cfg<LEVELS, CHUNKS, 2, MODE>(ab, Bcol, cols, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol);
    else if (topw <= 256) launch_cfg<LEVELS, CHUNKS, 4, MODE>(ab, Bcol, cols, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol);
    else if constexpr (LEVELS == 3) launch_cfg<LEVELS, CHUNKS, 8, MODE>(ab, Bcol, cols, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol);
}

// one class of rows (MODE None, Drop: the complemented-mask twin, Insert: the accumulate twin; Frow / Fcol: F's or D's CSR);
// wave_rows.hip picks LEVELS
template <int LEVELS, MaskMode MODE>
void launch_wave_levels(int bin, const int2 *ab, const int *Bcol, int cols, int topw, const RowRec *rec,
                        const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                        unsigned *err, const int *Frow, const int *Fcol, hipStream_t s, bool count)
{
    switch (bin) {
#define BSP_CASE(b) case b: launch_one<LEVELS, kWaveChunks[b], MODE>(ab, Bcol, cols, topw, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol); break;
    BSP_CASE(1) BSP_CASE(2) BSP_CASE(3) BSP_CASE(4) BSP_CASE(5) BSP_CASE(6) BSP_CASE(7) BSP_CASE(8)
    BSP_CASE(9) BSP_CASE(10) BSP_CASE(11) BSP_CASE(12) BSP_CASE(13) BSP_CASE(14) BSP_CASE(15) BSP_CASE(16)
#undef BSP_CASE
    static_assert(kWaveBins == 16, "one case per capacity class");
    default: break;
    }
}

// the Makefile builds one object per (LEVELS, mode) pair, -DBSP_WAVE_LEVELS=1..5 -DBSP_WAVE_MODE=None|Drop|Insert, so that
// they compile in parallel
#ifdef BSP_WAVE_LEVELS
template void launch_wave_levels<BSP_WAVE_LEVELS, MaskMode::BSP_WAVE_MODE>(int, const int2 *, const int *, int, int, const RowRec *,
                                                                           const long long *, const long long *, int, int, int *, int *,
                                                                           unsigned *, const int *, const int *, hipStream_t, bool);
#endif

}  // namespace bsp
