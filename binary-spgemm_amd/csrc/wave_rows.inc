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
//   arrays take 10 B of LDS per product of capacity, which is what sets the occupancy: ONE slot buffer S holds every
//   ranked level in turn -- a level is dead once its words and prefixes are in registers, so its child is built in place.
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
                                          + (LEVELS >= 2 ? 4 * SLOTS : 16)                       // S
                                          + (LEVELS >= 3 ? 2 * SLOTS : 16);                      // pre
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
// product test-and-sets ONE bit of a hash bitmap (all of S: 32 bits per product of capacity; one returning ds_or): a product
// that finds its bit clear is the first with its column for certain.  The few that find it set ("ambiguous": a true repeat or
// a hash collision, ~F/64 of them) are settled exactly, one by one, by comparing their column with every product of the
// row in registers: an ambiguous product repeats an earlier column iff an equal product exists that is not ambiguous (it
// set the bit) or is ambiguous and earlier in (chunk, lane) order.  No sweep, no scan, no ranked level: 1 LDS access per
// product instead of 4.  A row with more than kMaxAmbiguous of them (many repeats: the comparisons would cost more than
// the sweeps) takes the sweeps below.
constexpr int kMaxAmbiguous = 12;
constexpr int wr_floor_log2(int x) { int k = 0; while ((2 << k) <= x) k++; return k; }

// The one kernel of the family.  MODE (what a second operand, Frow / Fcol with absolute row ids, does to the rows):
//   None    nothing (Frow, Fcol, cols unused).  row_ptr != NULL: a row goes to its final place tmp + row_ptr[row - row_begin]
//           (tmp is C.col_idx then), else to its upper-bound offset recpre[k]
//   Drop    C = !F .* (A*B): the columns of F's row are dropped from each staged row before it is stored (drop_mask_cols)
//   Insert  C = D | (A*B): D's row is one more source of the gather, after the B rows -- its columns below `cols` are
//           accumulated like products, the others lose their valid bit (class and capacity were sized by F_B + |D_i|)
//   Drop and Insert rows are placed at their upper-bound offset (recpre), |C_i| to cnt; row_ptr is not looked at.
// COUNT (MODE None only): the symbolic pass -- the same sweeps, nothing emitted: a row whose products all sit alone in
//   their 32-column slots (known after the scan of the level above: nslots0 == F) has |C_i| = F_i without its level-0
//   masks being touched; only the others run the level-0 ORs and count their bits.  cnt[] is the result.
// The modes are template constants and the body is written once, here.  Where an expression differs between the modes it
// is a conditional on the constant, `ACC ? a : b`, which the front end folds before any code is emitted: every instance
// compiles to the instructions of the separate kernel it replaced (tools/isa_diff.py; DESIGN.md 4.5).  Two forms that do
// NOT keep the schedule: `bool ok = ...; if constexpr (ACC) ok = ok && !dsrc[c];`, and row_ptr at the end of the arguments.
template <int LEVELS, int CHUNKS, int TWP, MaskMode MODE, bool COUNT>
__global__ __launch_bounds__((64 * WaveCfg<LEVELS, CHUNKS, TWP>::WAVES))
void k_wave_rows(const int2 *__restrict__ ab, const int *__restrict__ Bcol,
                 const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                 const long long *__restrict__ row_ptr,
                 int nrows, int rpw, int row_begin, int *__restrict__ tmp, int *__restrict__ cnt,
                 unsigned *__restrict__ err, const int *__restrict__ Frow, const int *__restrict__ Fcol, int cols, int shared_max)
{
    constexpr bool EXCL = MODE == MaskMode::Drop, ACC = MODE == MaskMode::Insert;
    constexpr bool FEW = !COUNT && LEVELS >= 2 && CHUNKS <= 16;    // the few-shared-slots emit exists (else shared_max is unused)
    static_assert(!COUNT || MODE == MaskMode::None, "the symbolic pass has no masked form");
    using Cfg = WaveCfg<LEVELS, CHUNKS, TWP>;
    constexpr int TOPW = Cfg::TOPW, WAVES = Cfg::WAVES, SW = Cfg::SW, SLOTS = Cfg::SLOTS, FULL = Cfg::FULL;
    // separate objects: no false LDS dependencies between the arrays of one sweep
    __shared__ __attribute__((aligned(16))) u32 s_top[WAVES][TOPW];
    __shared__ __attribute__((aligned(16))) unsigned short s_topPre[WAVES][TOPW];
    __shared__ __attribute__((aligned(16))) u64 s_starts[WAVES][CHUNKS];
    __shared__ __attribute__((aligned(16))) u32 s_L0w[WAVES][SLOTS];       // also the gather's delta[] and the emit staging
    // the ranked levels, one after the other: level `lev` is built in the words that held level lev + 1 (see the descent)
    __shared__ __attribute__((aligned(16))) u32 s_S[WAVES][LEVELS >= 2 ? SLOTS : 4];
    __shared__ __attribute__((aligned(16))) unsigned short s_pre[WAVES][LEVELS >= 3 ? SLOTS : 8];

    const int lane = lane_id();
    // product slot of this lane inside a 64-product chunk: bit-reversed, so that neighbouring
    // lanes hold products of different B rows -- their ranks are then spread over the LDS banks
    // instead of marching through the slot arrays at a near-constant stride
    const int plane = (int)(__brev((unsigned)lane) >> 26);
    const int wave_in_wg = threadIdx.x >> 6;
    const long long wave_global = (long long)blockIdx.x * WAVES + wave_in_wg;
    const long long k0 = wave_global * rpw;                        // rpw <= Cfg::RPW <= 16 rows per wave
    if (k0 >= nrows) return;                                       // wave-uniform; no barriers used
    const int nmine = (nrows - k0 < rpw) ? (int)(nrows - k0) : rpw;

    // this wave's row records: one coalesced round trip for 16 rows
    int r_row = 0, r_a0 = 0, r_alen = 0;
    long long r_pre = 0;
    if (lane < nmine) {
        const RowRec q = rec[k0 + lane];
        r_row = q.row;
        r_a0 = q.a0;
        r_alen = q.alen;
        // numeric pass after an exact symbolic pass: the row goes to its final place in C.col_idx
        // (`tmp` is C.col_idx then); otherwise to its upper-bound offset in the workspace
        // (the masked kernels are placed at the upper bound only: they never look at row_ptr)
        if (!COUNT) r_pre = (EXCL || ACC) ? recpre[k0 + lane] : (row_ptr ? row_ptr[q.row - row_begin] : recpre[k0 + lane]);
    }

    u32 *top = s_top[wave_in_wg];
    unsigned short *topPre = s_topPre[wave_in_wg];
    u64 *starts = s_starts[wave_in_wg];
    u32 *L0w = s_L0w[wave_in_wg];
    int *delta = reinterpret_cast<int *>(s_L0w[wave_in_wg]);      // dead before L0w lives
    u32 *S = s_S[wave_in_wg];
    unsigned short *Spre = s_pre[wave_in_wg];

    // zero the structures that must be all-zero at the start of a row (kept so by every row)
    constexpr int TW = TOPW / 64;                                  // top words per lane
    clear_blocked<TW>(top, lane);
    if (lane < CHUNKS) starts[lane] = 0ull;
    if (LEVELS >= 2) clear_blocked<SW>(S, lane);
    wave_lds_fence();

    // prefetch of the first row's B-row extents
    int2 ab_next = make_int2(0, 0);
    {
        const int a0 = wave_bcast(r_a0, 0), alen = wave_bcast(r_alen, 0);
        if (lane < alen) ab_next = load_extent(ab + a0 + lane);
    }
    // CHUNKS stores through an EMPTY descriptor (all dropped by the range check): they put the same
    // number of younger vmcnt events behind the first prefetch as every later prefetch has, so
    // the wait at the top of the row loop is vmcnt(CHUNKS) on both the entry and the back edge
    if (!COUNT) store_row<CHUNKS, false>(tmp, 0, L0w, lane);

    int my_cnt = 0;
    for (int kk = 0; kk < nmine; kk++) {
        const int a0 = wave_bcast(r_a0, kk);
        const int alen = wave_bcast(r_alen, kk);
        const u32 pre_lo = (u32)wave_bcast((int)(u32)r_pre, kk);
        const u32 pre_hi = (u32)wave_bcast((int)(u32)((unsigned long long)r_pre >> 32), kk);
        int *out = tmp + (long long)(((u64)pre_hi << 32) | pre_lo);
        int f0 = 0, mlen = 0;                                      // EXCL: F's row, ACC: D's row (absolute row id)
        if constexpr (EXCL || ACC) {
            const int i = wave_bcast(r_row, kk);
            f0 = Frow[i];
            mlen = Frow[i + 1] - f0;
        }

        // ---- gather plan: product offsets of the selected B rows ------------------------
        int F = 0, nsrc = 0;
        for (int ab0 = 0; ab0 < alen; ab0 += 64) {                 // usually one trip
            int2 e = ab_next;
            if (ab0 > 0) {
                e = make_int2(0, 0);
                if (ab0 + lane < alen) e = load_extent(ab + a0 + ab0 + lane);
            }
            const int bs = e.x, len = e.y;
            const int inc = wave_incl_scan(len);
            const int excl = F + inc - len;
            const u64 bal = __ballot(len > 0);
            // (a row always fits its class -- bin_of sized it from these very extents -- so the bound below only
            // trips when an operand was rewritten under the library; then the row is cut off, not LDS overrun)
            if (len > 0 && (unsigned)excl < (unsigned)Cfg::CAP) {
                const int sidx = nsrc + __popcll(bal & mask_lt(lane));
                delta[sidx] = bs - excl;                           // B address = delta + product index
                atomicOr(&starts[excl >> 6], 1ull << (excl & 63));
            }
            F += wave_bcast(inc, 63);
            nsrc += __popcll(bal);
        }
        // ACC: D's row is the last source, products F_B .. F_B + |D_i| (class and capacity were sized by F_B + |D_i|)
        const int nsrcB = nsrc;
        if constexpr (ACC) {
            if (mlen > 0) {
                if ((unsigned)F < (unsigned)Cfg::CAP && lane == 0) {
                    delta[nsrc] = f0 - F;                          // D address = delta + product index
                    atomicOr(&starts[F >> 6], 1ull << (F & 63));
                }
                F += mlen;
                nsrc += 1;
            }
        }
        if (F > Cfg::CAP || F < 0) {                               // wave-uniform, never taken on consistent operands
            if (lane == 0) atomicOr(err, kErrCapacity);
            F = F < 0 ? 0 : Cfg::CAP;
        }
        wave_lds_fence();
        // starts words -> registers (lane c holds word c), then cleared for the next row
        u64 sw = 0ull;
        if (lane < CHUNKS) { sw = starts[lane]; starts[lane] = 0ull; }
        const int sinc = wave_incl_scan(__popcll(sw));
        const int sbefore = sinc - __popcll(sw);

        // ---- gather B.col_idx: all lanes busy, products kept in registers ---------------
        // The loads of all chunks are issued back to back and nothing consumes them here: lanes
        // past the end of the row load Bcol[0] and are masked later by their product index, so
        // the compiler has no reason to wait between the gathers.
        int col[CHUNKS];
        int rank[CHUNKS];
        int gaddr[CHUNKS];
        bool dsrc[CHUNKS];                                         // ACC: the product is one of D's row (tail lanes: source 0's kind)
                                                                   // until sweep 1, then: one of D's row outside [0, cols)
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            {
                const int p = c * 64 + plane;
                const u64 M = wave_bcast64(sw, c);
                const int before = wave_bcast(sbefore, c);
                int s = before + __popcll(M & mask_le(plane)) - 1;
                s = (c < FULL || p < F) ? s : 0;
                if constexpr (ACC) dsrc[c] = s == nsrcB;
                // unconditional LDS read (tail lanes read source 0 and load its first column): a
                // select on the loaded value makes the compiler wait after every single read
                gaddr[c] = delta[s];                               // consumed in the next loop: the
            }                                                      // LDS reads of all chunks overlap
        }
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            {
                const int p = c * 64 + plane;
                const int g = gaddr[c] + ((c < FULL || p < F) ? p : 0);
                col[c] = ACC ? (dsrc[c] ? Fcol : Bcol)[g] : Bcol[g];
            }
        }
        // prefetch the next row's extents: in flight while this row is accumulated
        ab_next = make_int2(0, 0);
        if (kk + 1 < nmine) {
            const int na0 = wave_bcast(r_a0, kk + 1), nalen = wave_bcast(r_alen, kk + 1);
            if (lane < nalen) ab_next = load_extent(ab + na0 + lane);
        }
        wave_lds_fence();   // delta (aliases L0w) is dead from here on

        bool row_counted = false;   // wave-uniform: the hash filter has settled |C_i|
        int running = 0;            // |C_i|
        if constexpr (COUNT && LEVELS >= 2 && CHUNKS <= 16) {       // (beyond 16 chunks the per-chunk masks spill: the sweeps stay)
            constexpr int HB = wr_floor_log2(32 * SLOTS);          // bits of the hash bitmap (S, all zero between rows)
            u32 *hb = S;
            bool amb[CHUNKS];
            u64 am[CHUNKS];
            int namb = 0;
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
                const bool ok = c < FULL || c * 64 + plane < F;
                const u32 cc = (u32)col[c];
                const u32 h = (cc ^ (cc >> HB) ^ (2 * HB < 32 ? cc >> ((2 * HB) & 31) : 0u)) & ((1u << HB) - 1u);
                u32 old = 0u;
                if (ok) old = atomicOr(&hb[h >> 5], 1u << (h & 31));
                amb[c] = ok && ((old >> (h & 31)) & 1u);
            }
            wave_lds_fence();
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
                am[c] = __ballot(amb[c]);
                namb += __popcll(am[c]);
            }
            clear_blocked<SW>(hb, lane);                           // S is all zero again, whichever way the row goes
            wave_lds_fence();
            if (namb <= kMaxAmbiguous) {
                int dups = 0;
                if (namb > 0) {
#pragma unroll
                    for (int c = 0; c < CHUNKS; c++) {
                        u64 m = am[c];
                        while (m) {                                // (wave-uniform: m is a ballot)
                            const int l = (int)__builtin_ctzll(m);
                            m &= m - 1ull;
                            const u32 x = (u32)__builtin_amdgcn_readlane(col[c], l);
                            u64 hit = 0ull;                        // equal products that settle it: not ambiguous, or ambiguous and earlier
#pragma unroll
                            for (int c2 = 0; c2 < CHUNKS; c2++) {
                                const bool ok2 = c2 < FULL || c2 * 64 + plane < F;
                                const u64 e = __ballot(ok2 && (u32)col[c2] == x);
                                hit |= e & ~am[c2];
                                if (c2 < c) hit |= e & am[c2];
                                if (c2 == c) hit |= e & am[c2] & mask_lt(l);
                            }
                            dups += hit != 0ull ? 1 : 0;
                        }
                    }
                }
                running = F - dups;
                row_counted = true;
            }
        }
        if (!row_counted) {
        // ---- sweep 1: top bitmap, addressed directly by the high digits -----------------
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            {
                if constexpr (ACC) dsrc[c] = dsrc[c] && (u32)col[c] >= (u32)cols;   // from here on: a column of D that is dropped
                const bool ok = ACC ? ((c < FULL || c * 64 + plane < F) && !dsrc[c]) : (c < FULL || c * 64 + plane < F);
                const u32 cc = ok ? (u32)col[c] : 0u;
                col[c] = (int)cc;                                  // tail lanes: column 0, never OR-ed
                const u32 tw = cc >> (5 * LEVELS);
                // tail lanes are masked off: parking them on one spare word instead makes up to 63
                // same-address atomics, which the LDS serialises (measured: -12 % kernel time)
                if (ok) atomicOr(&top[tw], 1u << ((cc >> (5 * (LEVELS - 1))) & 31));
                rank[c] = (int)tw;
            }
        }
        wave_lds_fence();

        u32 *S0;                     // level-0 slots (32-column masks) of this row
        int nslots0 = 0;             // how many of them the row uses (LEVELS >= 2)
        bool few = false;            // wave-uniform: 1 .. shared_max products more than level-0 slots (FEW instances)
        int nlose = 0;               // few: the distinct columns that share a slot and are not the one left beside it
        if (LEVELS == 1) {
            S0 = top;
        } else {
            // number of slots of the level below the one just scanned; after the last scan it is
            // the number of level-0 slots of the row
            nslots0 = scan_blocked<TW>(top, topPre, lane);         // ranks of the level LEVELS-2 slots
            wave_lds_fence();
            const u32 *P = top;
            const unsigned short *Ppre = topPre;
            bool parent_is_top = true;
#pragma unroll
            for (int lev = LEVELS - 2; lev >= 0; lev--) {
                // as many level-0 slots as products: every product sits alone in its 32-column slot
                // (wave-uniform; nslots0 counts the slots of level `lev` here)
                const bool sparse = lev == 0 && nslots0 == F;
                // nearly sparse: the row never touches its masks either, and is put in order from the columns alone (below)
                if constexpr (FEW) few = lev == 0 && nslots0 != F && F - nslots0 <= shared_max;
                // Level `lev` goes to S, all zero here.  Below the first ranked level its parent is in S too: the parent is
                // dead once every chunk's word and prefix are in px[] / ppre[], so it is cleared between those reads and the
                // first OR, and the child is built in its place (DS operations of one wave execute in issue order).
                u32 px[CHUNKS];
                int ppre[CHUNKS];
#pragma unroll
                for (int c = 0; c < CHUNKS; c++)                   // all parent reads first ...
                    {
                        px[c] = P[rank[c]];
                        ppre[c] = Ppre[rank[c]];
                    }
                if (!parent_is_top) {
                    wave_lds_fence();
                    clear_blocked<SW>(S, lane);                    // parent level is consumed
                    wave_lds_fence();
                }
#pragma unroll
                for (int c = 0; c < CHUNKS; c++)                   // ... then all the ORs
                    {
                        const bool ok = ACC ? ((c < FULL || c * 64 + plane < F) && !dsrc[c]) : (c < FULL || c * 64 + plane < F);
                        const u32 cc = (u32)col[c];
                        const u32 b = (cc >> (5 * (lev + 1))) & 31;
                        const int r2 = ppre[c] + __popc(__builtin_amdgcn_ubfe(px[c], 0u, b));   // bits below b
                        const u32 bit = 1u << ((cc >> (5 * lev)) & 31);
                        if (ok) {                                  // tail lanes: no LDS traffic at all
                            if (lev == 0) {
                                // a sparse row -- known since the scan of the level above -- never reads
                                // its masks: only the column beside the mask is kept
                                if (!sparse && !few) atomicOr(&S[r2], bit);
                                if (!COUNT) L0w[r2] = cc;          // any product of the slot: same cc >> 5
                            } else {
                                atomicOr(&S[r2], bit);
                            }
                        }
                        rank[c] = r2;
                    }
                wave_lds_fence();
                if (parent_is_top) clear_blocked<TW>(top, lane);   // parent level is consumed
                parent_is_top = false;
                if (lev > 0) {
                    nslots0 = scan_blocked<SW>(S, Spre, lane);
                    P = S;
                    Ppre = Spre;
                }
                wave_lds_fence();
            }
            S0 = S;
        }

        // ---- few shared slots: F - nslots0 <= shared_max products more than slots.  Such a row is a sparse row but for
        // a slot or two that hold several columns; the mask level (OR, blocked reads, clear, expansion) is not needed to
        // sort it.  L0w[r2] holds the column of ONE product of the slot, the winner; the other products of a slot with m
        // distinct columns read back a column that is not theirs: its losers, m - 1 distinct columns.  Slots ascend with
        // the columns, so the place of product x among the row's distinct columns is its slot, plus one if it lost to a
        // smaller column, plus the distinct loser columns below its own -- a handful of wave-uniform broadcasts, as in the
        // count pass's settle loop.  A repeat reads back what its first copy reads: alone in its slot it is no loser, and
        // as a loser it is passed over when an earlier loser (chunk, lane) has its column -- every product of a loser's
        // column is a loser of the same slot.  Either way the copies get one place and one value.  S0 is never touched.
        if constexpr (FEW) {
            if (few) {
                u32 v[CHUNKS];                                     // the winner's column
                u64 lm[CHUNKS];                                    // the losers of each chunk
#pragma unroll
                for (int c = 0; c < CHUNKS; c++) v[c] = L0w[rank[c]];   // (every lane: tail lanes read slot 0)
#pragma unroll
                for (int c = 0; c < CHUNKS; c++) {
                    const bool ok = ACC ? ((c < FULL || c * 64 + plane < F) && !dsrc[c]) : (c < FULL || c * 64 + plane < F);
                    lm[c] = __ballot(ok && v[c] != (u32)col[c]);
                    rank[c] += v[c] < (u32)col[c] ? 1 : 0;         // (tail lanes: column 0, never placed)
                }
                wave_lds_fence();                                  // every winner is read: L0w becomes the row
#pragma unroll
                for (int c = 0; c < CHUNKS; c++) {
                    u64 m = lm[c];
                    while (m) {                                    // (wave-uniform: m is a ballot)
                        const int l = (int)__builtin_ctzll(m);
                        m &= m - 1ull;
                        const u32 x = (u32)__builtin_amdgcn_readlane(col[c], l);
                        u64 earlier = __ballot((u32)col[c] == x) & lm[c] & mask_lt(l);
#pragma unroll
                        for (int c2 = 0; c2 < c; c2++) earlier |= __ballot((u32)col[c2] == x) & lm[c2];
                        if (earlier == 0ull) {
                            nlose++;
#pragma unroll
                            for (int c2 = 0; c2 < CHUNKS; c2++) rank[c2] += (u32)col[c2] > x ? 1 : 0;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < CHUNKS; c++) {
                    const bool ok = ACC ? ((c < FULL || c * 64 + plane < F) && !dsrc[c]) : (c < FULL || c * 64 + plane < F);
                    if (ok) L0w[rank[c]] = (u32)col[c];
                }
                wave_lds_fence();
            }
        }

        // ---- emit: lane l expands its own W consecutive level-0 slots (ascending columns) into
        // the LDS staging row at the rank given by one wave scan, then the wave streams the
        // staged row to memory fully coalesced.
        constexpr int W0 = (LEVELS == 1) ? TW : SW;
        if (LEVELS >= 2 && (nslots0 == F || few)) {
            // Sparse row (the common case when cols >> F_i): every level-0 slot holds ONE column,
            // so slot index = output position and L0w already is the sorted row.  A row of few shared slots was
            // brought into the same form above.
            running = nslots0 + (few ? nlose : 0);                 // (the masks were never written)
            if constexpr (EXCL)
                if (running > 0 && mlen > 0) running = drop_mask_cols<CHUNKS, false>(L0w, running, top, Fcol, f0, mlen, lane);
            if (!COUNT) store_row<CHUNKS, false>(out, running, L0w, lane);
        } else if (COUNT) {
            u32 m[W0];
#pragma unroll
            for (int k = 0; k < W0; k++) m[k] = S0[lane * W0 + k];
            clear_blocked<W0>(S0, lane);
            int mine = 0;
#pragma unroll
            for (int k = 0; k < W0; k++) mine += __popc(m[k]);
            running = wave_bcast(wave_incl_scan(mine), 63);
        } else {
            u32 m[W0], wv[W0];
#pragma unroll
            for (int k = 0; k < W0; k++) {
                m[k] = S0[lane * W0 + k];
                wv[k] = (LEVELS == 1) ? (u32)(lane * W0 + k) : (L0w[lane * W0 + k] >> 5);
            }
            clear_blocked<W0>(S0, lane);
            int mine = 0;
#pragma unroll
            for (int k = 0; k < W0; k++) mine += __popc(m[k]);
            const int inc = wave_incl_scan(mine);
            running = wave_bcast(inc, 63);
            wave_lds_fence();                                      // L0w reads are done: reuse it as staging
            {
                u32 *stage = L0w;
                int pos = inc - mine;
#pragma unroll
                for (int k = 0; k < W0; k++) {
                    u32 mk = m[k];
                    const u32 base = wv[k] << 5;
                    while (mk) {
                        stage[stage_swz(pos)] = base | (u32)__builtin_ctz(mk);
                        pos++;
                        mk &= mk - 1u;
                    }
                }
            }
            wave_lds_fence();
            if constexpr (EXCL)
                if (running > 0 && mlen > 0) running = drop_mask_cols<CHUNKS, true>(L0w, running, top, Fcol, f0, mlen, lane);
            store_row<CHUNKS, true>(out, running, L0w, lane);
        }
        }   // !row_counted
        my_cnt = (lane == kk) ? running : my_cnt;                  // lane kk keeps |C_i| of row kk
        wave_lds_fence();
    }
    if (cnt && lane < nmine) cnt[r_row - row_begin] = my_cnt;
}

// MODE Drop, Insert: Frow / Fcol are F's or D's CSR (numeric pass, upper-bound placement only)
template <int LEVELS, int CHUNKS, int TWP, MaskMode MODE>
static void launch_cfg(const int2 *ab, const int *Bcol, int cols, const RowRec *rec,
                       const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                       unsigned *err, hipStream_t s, bool count, const int *Frow, const int *Fcol, int shared_max)
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
    // (the symbolic pass exists for the unmasked product only: launch_wave_rows refuses the other combinations)
    auto kernel = k_wave_rows<LEVELS, CHUNKS, TWP, MODE, false>;
    if constexpr (MODE == MaskMode::None)
        if (count) kernel = k_wave_rows<LEVELS, CHUNKS, TWP, MODE, true>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                       ab, Bcol, rec, recpre, row_ptr, nrows, rpw, row_begin, tmp, cnt, err, Frow, Fcol, cols, shared_max);
}

template <int LEVELS, int CHUNKS, MaskMode MODE>
static void launch_one(const int2 *ab, const int *Bcol, int cols, int topw, const RowRec *rec,
                       const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                       unsigned *err, hipStream_t s, bool count, const int *Frow, const int *Fcol, int shared_max)
{
    // the top bitmap is sized to what the column count needs: 128 or 256 words; 512 at three
    // levels (wave_levels_for_cols)
    if (topw <= 128) launch_cfg<LEVELS, CHUNKS, 2, MODE>(ab, Bcol, cols, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol, shared_max);
    else if (topw <= 256) launch_cfg<LEVELS, CHUNKS, 4, MODE>(ab, Bcol, cols, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol, shared_max);
    else if constexpr (LEVELS == 3) launch_cfg<LEVELS, CHUNKS, 8, MODE>(ab, Bcol, cols, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol, shared_max);
}

// one class of rows (MODE None, Drop, Insert; Frow / Fcol: F's or D's CSR); wave_rows.hip picks LEVELS
template <int LEVELS, MaskMode MODE>
void launch_wave_levels(int bin, const int2 *ab, const int *Bcol, int cols, int topw, const RowRec *rec,
                        const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                        unsigned *err, const int *Frow, const int *Fcol, hipStream_t s, bool count, int shared_max)
{
    switch (bin) {
#define BSP_CASE(b) case b: launch_one<LEVELS, kWaveChunks[b], MODE>(ab, Bcol, cols, topw, rec, recpre, row_ptr, nrows, row_begin, tmp, cnt, err, s, count, Frow, Fcol, shared_max); break;
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
                                                                           unsigned *, const int *, const int *, hipStream_t, bool, int);
#endif

}  // namespace bsp
