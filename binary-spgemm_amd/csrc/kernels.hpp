// kernels.hpp -- launch wrappers of the HIP kernels behind bspgemm_multiply (host-callable).
// Kernels: prepass.hip (row work, scans, class records), wave_rows.inc (k_wave_rows; one object per (LEVELS, mask mode) pair,
// dispatched by wave_rows.hip), wave_masked.hip (k_wave_masked), dense_rows.hip (k_dense_rows, k_dense_rows_count,
// k_rank_rows) over the heavy rows' gather in heavy_gather.hpp, compact.hip (compaction, heavy-row moves),
// small.hip, transpose.hip, select.hip, setop.hip, bfs.hip, cc.hip, kcore.hip, dot.hip, bfs_tree.hip (the launches of the last six stay in their files).  A family is ONE template kernel with the mask mode as a template parameter.
// Tuning constants are compile-time constants, not switches: what was tried against them is in profiles/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace bsp {

// capacity classes of a row by its product count F_i:
//   0          : empty
//   1..16      : one wavefront per row, capacity 64*kWaveChunks[b] products.  The kernel body is
//                straight-line over its CHUNKS 64-product chunks (exact s_waitcnt counts, no
//                branches), so a row costs what its CLASS costs: the classes step by one chunk up
//                to 512 products, by two up to 1024, then by four/eight
//   kRankBin   : 2048 < F_i <= rank_cap_for_cols(cols) (0 = no such class for this column count; 6144 for 2^18 < cols <= 2^24):
//                a 512-thread workgroup with a two-level rank bitmap -- LDS and read-out proportional to the row (dense_rows.hip)
//   kMidBin    : dense-window rows, up to mid_cap_for_cols(cols) products: 512-thread workgroups, four per CU
//   kDenseBin  : dense-window rows, above that: one 1024-thread workgroup per row
// what a second operand does to a product's rows: none, keep only its columns (C = F .* (A*B)), drop its columns
// (C = !F .* (A*B)), insert its columns (C = D | (A*B), the OR-accumulating product), keep only its columns and count the
// products of each (C = F .* (A*B) with path counts: the values go to a second workspace at the columns' offsets)
enum class MaskMode { None, Keep, Drop, Insert, Count };

constexpr int kWaveBins = 16;
constexpr int kNumBins = kWaveBins + 4;
constexpr int kRankBin = kWaveBins + 1;
constexpr int kMidBin = kWaveBins + 2;
constexpr int kDenseBin = kWaveBins + 3;
constexpr int kRankCap = 6144;          // products (= slots) of a rank-class row
int rank_cap_for_cols(long long cols);  // kRankCap, or 0 where the class is not used (dense_rows.hip)
constexpr int kMaxBins = 20;            // size of the per-class arrays in bspgemm_stats
constexpr int kWaveChunks[kWaveBins + 1] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32};
constexpr int kMaxWaveCap = 64 * kWaveChunks[kWaveBins];   // 2048 products
// products up to which a heavy row takes the small (512-thread) shape: its 32 KiB window covers 2^18
// columns, so the row's products are gathered ceil(cols / 2^18) times -- the fewer passes, the larger
// the rows it is good for.  Swept with BSPGEMM_MID_CAP on the round-2 build (numeric phase, ms):
// Graph500-skew scale 18 (one pass) 131072: 6.47, 524288: 5.87, 4194304: 6.18; power-law n = 2^20 (four
// passes) 8192: 13.18, 32768: 12.88, 131072: 12.59, 262144: 12.96 -- i.e. 524288 / passes in both cases.
constexpr int kMidCap = 524288;
inline int mid_cap_for_cols(long long cols)
{
    const long long passes = (cols + (1ll << 18) - 1) >> 18;
    if (passes <= 1) return kMidCap;
    const long long c = kMidCap / passes;
    return c < kMaxWaveCap ? kMaxWaveCap : (int)c;      // (== kMaxWaveCap: no row takes the small shape)
}
constexpr int kRowsPerWave = 16;        // consecutive list entries handled by one wave

constexpr int kWaveTopWords = 256;      // 32-bit words of the directly addressed top bitmap

// number of 5-bit levels of the rank bitmap for `cols` columns: the smallest L whose top bitmap
// ceil(cols / 32^L) fits kWaveTopWords words
//   L=1: cols <= 8192 (the top bitmap IS the column bitmap)   L=2: <= 2^18   L=3: <= 2^23
//   L=4: <= 2^28                                              L=5: any int32 column count
inline int levels_for_cols(int64_t cols)
{
    for (int L = 1; L < 5; L++)
        if (cols <= ((int64_t)kWaveTopWords << (5 * L))) return L;
    return 5;
}

// k_wave_rows trades a fourth level for a larger top bitmap up to 2^24 columns (512 top words at
// three levels): one ranked level costs two LDS reads, an atomic and a blocked scan per product
// chunk, the larger top only a longer scan/clear per row (measured at 2^24 columns: -6 % kernel
// time; 1024 words at 2^25 columns loses to four levels: too few resident waves).
constexpr int kWaveTopWordsWide = 512;
inline int wave_levels_for_cols(int64_t cols)
{
    const int L = levels_for_cols(cols);
    if (L == 4 && cols <= ((int64_t)kWaveTopWordsWide << 15)) return 3;
    return L;
}

// one record per non-empty row, grouped by capacity class (written by the prepass)
struct RowRec {
    int row;    // absolute row id
    int a0;     // A.row_ptr[row]
    int alen;   // |A_row|
    int f;      // F_row (clamped to INT_MAX)
};

// F_i = sum_{j in A_i} |B_j| for rows [row_begin,row_end)  ->  F[i-row_begin];
// ab[jj] = (start of B row A.col_idx[jj], |B_j|) for every A-nonzero of those rows.  What is gathered per A-nonzero:
//   Bblk16 != NULL   B's blocked extents table (launch_blk16); with Bpad (the padded row_ptr) its bases and the starts are
//                   positions in the PADDED copy of B.col_idx
//   else Bext       the per-row table {start in the padded copy, length}
//   else            a B.row_ptr pair (starts in B.col_idx itself)
// With Bblk16 the pass is flat, in tiles of kRowWorkTile merged positions (each row's nonzeros and one end item):
// nnz_bound (host) bounds the range's nonzeros, tile_row has room for (nnz_bound + rows) / kRowWorkTile + 2 ints.
constexpr int kRowWorkTile = 4096;
void launch_row_work(const int *Arow, const int *Acol, const int *Brow, const int *Bblk16, const int *Bpad, const int2 *Bext,
                     int row_begin, int row_end, long long nnz_bound, int *tile_row, long long *F, int2 *ab, hipStream_t s);
// blk[4g..4g+3] = {start_ptr[16g] (NULL: row_ptr), lengths of rows 16g..16g+15 clamped to 63, six bits each}: 16-byte aligned
// *clamped_nnz (device, zeroed by the caller) += nonzeros in rows of 63 or more
void launch_blk16(const int *row_ptr, const int *start_ptr, int n, int *blk, unsigned long long *clamped_nnz, hipStream_t s);
// padded copy of an operand's col_idx (rows on 64-byte boundaries): plen[j] = ceil(len_j / 16) * 16; then, with pad_ptr =
// its exclusive scan, the rows copied to col_pad and (ext != NULL) ext[j] = {pad_ptr[j], len_j}
void launch_pad_lengths(const int *row_ptr, int n, int *plen, hipStream_t s);
void launch_pad_copy(const int *row_ptr, const int *col_idx, const int *pad_ptr, int n, int *col_pad, int2 *ext, hipStream_t s);

// deg8[i] = min(|row i|, 255): the per-operand byte table behind launch_row_products
void launch_deg8(const int *row_ptr, int n, unsigned char *deg8, hipStream_t s);
// F only (no extents), through B's byte table of row lengths
void launch_row_products(const int *Arow, const int *Acol, const int *Brow, const unsigned char *Bdeg8,
                         int row_begin, int row_end, long long *F, hipStream_t s);

// exclusive scan of F (int64) into prefix[0..n] and, fused, classification of every row into
// the capacity classes: rec[] holds the non-empty rows grouped by class (class b starts at
// sum(bin_count[1..b-1])), recpre[] their output offsets; bin_count[8] on the device.
// bound_cols > 0: rows are CLASSIFIED by F_i but PLACED by min(F_i, bound_cols) (prefix[] and recpre[]
// are offsets of that bound: a row cannot have more outputs than B has columns -- what keeps the
// upper-bound workspace of a skewed product near nnz(C) instead of near F).
// heavy_cols > 0: the heavy rows (class kDenseBin) get their own workspace offsets in recpre --
// exclusive prefix of min(F_i, heavy_cols) over the heavy rows -- and hpartials[ceil(n/2048)]
// holds that workspace's total size; one-wave rows are then placed by the symbolic counts.
// `scal` (device, may be NULL): everything the host reads back after the prepass in one struct --
// without a heavy-row workspace (heavy_cols <= 0) also the product count, summed from `true_F` when
// the rows are sized by something else than their products (masked multiply), else from F.
struct PrepScalars {
    long long totalF;
    long long heavy_total;
    long long products;
    int a_lo, a_hi;
    int bin_count[kNumBins];
    unsigned long long max_f;   // the counting product's largest F_i (launch_mask_lengths_count; that flow zeroes it)
};
void launch_scan_and_bin(const long long *F, int n, int row_begin, const int *Arow, long long *prefix,
                         long long *partials, int *bin_tiles, int *bin_count, RowRec *rec,
                         long long *recpre, int *cnt, int heavy_cols, long long *hpartials, int mid_cap, int rank_cap, int bound_cols,
                         hipStream_t s, PrepScalars *scal = nullptr, const long long *true_F = nullptr);

// prefix[0..n] = *base + exclusive scan of the int32 counts (base NULL = 0; may alias prefix[0])
// `chunk_row` (may be NULL; needs base == NULL): chunk_row[c] = the row that holds output c * kCompactGran, for every
// such output below the total, and chunk_row[ceil(total / kCompactGran)] = the row of the last output -- the
// compaction's row look-up, left behind by the scan that knows every row's range anyway
constexpr int kCompactGran = 4096;
inline size_t compact_chunk_rows(long long max_out) { return (size_t)((max_out + kCompactGran - 1) / kCompactGran) + 2; }
void launch_scan_counts(const int *cnt, int n, long long *prefix, long long *partials,
                        const long long *base, hipStream_t s, int *chunk_row = nullptr);

// numeric phase, one wave per row (rank-bitmap accumulator).  row_ptr != NULL: row i is written at
// tmp + row_ptr[i - row_begin] (tmp = C.col_idx, sizes known from the symbolic phase, cnt may be
// NULL); row_ptr == NULL: at its upper-bound offset tmp + recpre[k], |C_i| to cnt (masked product)
// count_only: the COUNT instances of the same kernel -- nothing is emitted (tmp, recpre, row_ptr unused), cnt[i] = |C_i|
// mode Drop: the Drop instances (C = !F .* (A*B), upper-bound placement only): the columns of F's row (Frow / Fcol,
// absolute row ids) are dropped from every row before it is stored.  Keep has no one-wave kernel here (launch_wave_masked),
// and count_only needs None: both return hipErrorInvalidValue.  mode Insert: the Insert instances (C = D | (A*B), upper-bound
// placement only): the columns of D's row (passed as Frow / Fcol) within [0, cols) join the row's gather as one more source.
// Count has no kernel here either (launch_wave_masked, launch_dense_rows): hipErrorInvalidValue
// err (device, never NULL): bit 0 is set when a row's gathered product count exceeds its class capacity -- impossible
// for consistent operands (the classes come from the same extents), seen only when an operand was rewritten under
// the library; the row is then truncated to its capacity instead of overrunning LDS
// shared_slots (BSPGEMM_OPT_SHARED_SLOTS; the emitting instances of 2+ levels and up to 16 chunks): a row with 1 .. shared_max
// products more than level-0 slots -- a sparse row but for a few slots that hold several columns -- is put in order from
// its columns alone and never builds its level-0 masks.  -1: shared_max from the per-class table (wave_shared_max),
// 0: no such rows, k: shared_max = min(k, kSharedSlotsMax) in every class.  The result is the same for every value.
constexpr int kSharedSlotsMax = 16;
int wave_shared_max(int bin, int shared_slots);
constexpr unsigned kErrCapacity = 1u;     // a row gathered more products than its capacity class holds
constexpr unsigned kErrStaleTable = 2u;   // an operand's derived tables do not match its row_ptr (bspgemm_matrix_invalidate)
hipError_t launch_wave_rows(int bin, int levels, const int2 *ab, const int *Bcol, int cols,
                            const RowRec *rec, const long long *recpre, const long long *row_ptr, int nrows,
                            int row_begin, int *tmp, int *cnt, unsigned *err, MaskMode mode, const int *Frow, const int *Fcol,
                            hipStream_t s, bool count_only = false, int shared_slots = 0);
// debug check (BSPGEMM_OPT_CHECK): deg8[] / blk16[] / the padded row_ptr (each may be NULL) against row_ptr; sets kErrStaleTable in *err
void launch_check_tables(const int *row_ptr, int rows, const unsigned char *deg8, const int *blk16, const int *pad_ptr, unsigned *err,
                         hipStream_t s);

// heavy rows: workspace -> final place (one workgroup per heavy row)
void launch_place_heavy(const int *tmp, const RowRec *rec, const long long *recpre, int nrows,
                        const long long *row_ptr, int row_begin, int *col_idx, hipStream_t s);

// numeric phase, one workgroup per heavy row (windowed dense LDS bitmap); mid: the 512-thread shape, rank: the rank bitmap.
// F's row (Frow / Fcol, absolute row ids): Drop clears its bits from each column window (rank class: from each span's slots)
// before it is read out, in every shape; Keep admits only its columns, and every row of any class, `bin` ignored, goes through
// the 1024-thread window kernel; Insert sets the columns of D's row (passed as Frow / Fcol) within [0, cols) in each window
// (rank class: in each span's top bits and slots); Count, like Keep for every row and class, runs the counting window kernel
// (F's columns ranked per window, one counter each) and writes each row's counts to vals at the offsets of its columns in tmp
hipError_t launch_dense_rows(int bin, const int2 *ab, const int *Bcol, long long nnzB, int cols,
                             const RowRec *rec, const long long *recpre, int nrows, int row_begin,
                             int *tmp, int *cnt, MaskMode mode, const int *Frow, const int *Fcol, hipStream_t s,
                             int *vals = nullptr);

// the heavy rows' records in order of decreasing products (n <= kHeavySortMax), into rec_out / pre_out
constexpr int kHeavySortMax = 8192;
void launch_order_heavy(const RowRec *rec, const long long *recpre, int n, RowRec *rec_out, long long *pre_out, hipStream_t s);

// mask-first one-wave path of the masked product (mask rows <= 2048 entries, cols <= 2^23); vals != NULL: the counting
// instances (k_wave_masked<.., true>), every kept column's product count to vals at the column's offset in tmp
bool wave_masked_supported(int cols);
void launch_wave_masked(int bin, const int2 *ab, const int *Bcol, int cols, const int *Frow, const int *Fcol,
                        const RowRec *rec, const long long *recpre, int nrows, int row_begin,
                        int *tmp, int *cnt, int *vals, hipStream_t s);
// the rows of class `bin` (upper-bound placement at tmp + recpre[k], |C_i| to cnt), whichever kernel family the class and
// the mask mode take: one-wave classes launch_wave_rows, heavy classes launch_dense_rows; Keep: a one-wave class takes
// launch_wave_masked where wave_masked_supported(cols), every other row the 1024-thread window kernel.  count_only (the
// exact flow's count pass, mode None): the one-wave rows only count, the heavy rows are accumulated into the workspace.
// Count routes like Keep, to the counting kernels, with the values workspace `vals`
hipError_t launch_class(int bin, const int2 *ab, const int *Bcol, long long nnzB, int cols, const RowRec *rec,
                        const long long *recpre, int nrows, int row_begin, int *tmp, int *cnt, unsigned *err, MaskMode mode,
                        const int *Frow, const int *Fcol, hipStream_t s, bool count_only = false, int *vals = nullptr,
                        int shared_slots = 0);
// mlen[i] = |F's row i| when row i has products, else 0: what the masked product bins and offsets by
void launch_mask_lengths(const long long *F, const int *Frow, int row_begin, int n, long long *mlen, hipStream_t s);
// the same for the counting product, and *maxF (device, zeroed by the caller) = the largest F_i of the rows
void launch_mask_lengths_count(const long long *F, const int *Frow, int row_begin, int n, long long *mlen,
                               unsigned long long *maxF, hipStream_t s);
// size[i] = F[i] + |D's row row_begin + i|: what the accumulating product (C = D | (A*B)) bins and offsets by
void launch_insert_lengths(const long long *F, const int *Drow, int row_begin, int n, long long *size, hipStream_t s);

// rows [row_lo,row_hi): tmp[Fprefix[r] .. +cnt[r])  ->  col_idx[row_ptr[r] ..).  The output range
// is read from row_ptr on the device; `max_out` (an upper bound of its length, e.g. the rows'
// product count) only sizes the grid.
void launch_compact(const int *tmp, const long long *Fprefix, const long long *row_ptr,
                    int row_lo, int row_hi, long long max_out, int *col_idx, hipStream_t s, const int *chunk_row = nullptr);

// ---- single-round-trip path for small products (small.hip) ----------------------------------------
constexpr int kSmallMaxProducts = 65536;   // products (and entries of C.col_idx / the workspace) the path is sized for
constexpr int kSmallMaxRow = 2048;         // products of one row (one wave sorts them in LDS)
constexpr int kSmallMaxRows = 1 << 17;     // rows multiplied (one workgroup scans them)
constexpr int kSmallMaxNnzA = 32768;       // A-nonzeros in the multiplied rows (host-side eligibility)
struct SmallScalars {                      // what the host reads back, once, at the end
    long long totalF;                      // products
    long long nnzC;
    int bail;                              // 1: the product does not fit this path (nothing was written): take the general flow
    int nonempty;                          // rows with products
    int a_lo, a_hi;                        // A.row_ptr at the ends of the row range
};
struct SmallTiles {                        // device scratch of the path's two scans (per 32 rows / per 256 rows)
    long long f32[kSmallMaxRows / 32];     // products
    int nz32[kSmallMaxRows / 32];          // non-empty rows
    int mx32[kSmallMaxRows / 32];          // largest row
    int c256[kSmallMaxRows / 256];         // outputs
};
// list[] (ints, >= nrows), F / Fprefix (nrows + 1), cnt (nrows), tmp and col_idx (kSmallMaxProducts each), row_ptr (nrows + 1)
void launch_small(const int *Arow, const int *Acol, const int *Brow, const int *Bcol, int row_begin, int nrows,
                  long long *F, long long *Fprefix, int *list, int *cnt, int *tmp, long long *row_ptr, int *col_idx,
                  SmallTiles *tl, SmallScalars *sc, hipStream_t s);

// int64 row_ptr -> int32 (operand form of a product)
void launch_narrow_row_ptr(const long long *src, int *dst, int n, hipStream_t s);
// T = A or I as CSR: row i gets column i appended (duplicates are legal in operands)
void launch_add_diagonal(const int *Arow, const int *Acol, int n, int *Trow, int *Tcol, hipStream_t s);

// ---- stable select of CSR entries and the reduction of values (select.hip) --------------------------
// A select over nnz entries works in tiles of kSelTile entries and keeps, per 64 entries, one flag word (bit b of word w:
// entry 64 w + b is kept) and its popcount: select_words(nnz) of each, whole tiles (the words past the last entry are 0).
constexpr int kSelTile = kRowWorkTile;     // the structural select borrows the flat prepass's tile_row (ensure_tile_rows(nnz))
inline int select_tiles(long long nnz) { return (int)((nnz + kSelTile - 1) / kSelTile); }   // the grid of an entry-parallel pass
inline size_t select_words(long long nnz) { return (size_t)select_tiles(nnz) * (kSelTile / 64); }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }   // 16-byte loads are allowed
// the grid of a row pass: one thread of a 256-thread workgroup per r in [0, rows]
inline dim3 row_pass_grid(int rows) { return dim3((unsigned)(((long long)rows + 1 + 255) / 256)); }
// pass 1, structural: entry (r, c) is kept when c < r (op 1, BSPGEMM_SELECT_TRIL), c > r (2, TRIU), c != r (3, OFFDIAG);
// tile_row: nnz / kSelTile + 1 ints of scratch
void launch_select_flags_struct(const int *row_ptr, const int *col_idx, int rows, long long nnz, int op, int *tile_row,
                                unsigned long long *flags, int *cnt, hipStream_t s);
// tile_row[t] = the row that holds entry t * kSelTile, for every such entry below row_ptr[rows] (rows > 0)
void launch_select_tile_rows(const int *row_ptr, int rows, int *tile_row, hipStream_t s);
// pass 1, by value: entry e is kept when vals[e] cmp threshold (cmp: a bspgemm_compare)
void launch_select_flags_value(const int *vals, long long nnz, int cmp, int threshold, unsigned long long *flags, int *cnt,
                               hipStream_t s);
// pass 2: out[prefix[w] + (kept entries of word w before e)] = src[e] for every kept entry; prefix = the exclusive scan
// of cnt (launch_scan_counts), select_words(nnz) + 1 entries
void launch_select_scatter(const int *src, long long nnz, const unsigned long long *flags, const long long *prefix, int *out,
                           hipStream_t s);
// out[r] = kept entries before position row_ptr[r], r in [0, rows]; the unfiltered row_ptr is row_ptr32, or (NULL) row_ptr64
void launch_select_row_ptr(const int *row_ptr32, const long long *row_ptr64, int rows, long long nnz,
                           const unsigned long long *flags, const long long *prefix, int *out, hipStream_t s);
// *sum (device, zeroed by the caller) += vals[0 .. nnz), exact in 64 bits
void launch_values_sum(const int *vals, long long nnz, unsigned long long *sum, hipStream_t s);

// ---- the canonical-form check of setop.hip, alone (k_set_flags<false>; also dot.hip's) ----------------------------
constexpr unsigned kSetErrRange = 1u;      // a column outside [0, cols)
constexpr unsigned kSetErrOrder = 2u;      // a row that is not strictly ascending
// *err |= (kSetErrRange | kSetErrOrder as found in the operand) << err_shift; nothing else is written.  tile_row: nnz /
// kSelTile + 1 ints of scratch
void launch_canonical_check(const int *row_ptr, const int *col_idx, int rows, int cols, long long nnz, int err_shift,
                            int *tile_row, unsigned *err, hipStream_t s);

// ---- the submatrix extraction (extract.hip; tests/extract_ref.py mirrors the three) ------------------------------------
constexpr int kExHubChunk = 4096;          // the longest row of A left to one group of lanes; entries per chunk of a longer one
constexpr int kExSortWave = 256;           // the longest out row that one wave sorts in its LDS segment
constexpr int kExSortBlock = 4096;         // the longest out row that a workgroup sorts in 16 KiB of LDS

// row_ptr rebasing helper for interior-pointer uploads
void launch_rebase_i32(int *row_ptr, int n, int base, hipStream_t s);

}  // namespace bsp
