/*
 * bspgemm.h -- C ABI of libbspgemm.so: boolean (pattern-only) SpGEMM  C = A*B  on MI355X.
 *
 * This is the drop-in boundary for the reference's row-wise Gustavson path
 * (pavlidic/Binary-SpGEMM, final/SpGEMM_mpi_omp.c).  The reference has no plugin or FFI
 * registry: its boundary is a handful of plain C functions on raw `int*` CSR arrays plus the
 * command line.  Every entry point below names the reference interface it
 * replaces (file:line, relative to the reference checkout).  Plain pointers and sizes only; no
 * C++/torch types.  All functions are callable from C (the host side of this project is C).
 *
 * Conventions shared with the reference:
 *   - CSR, 0-based; `row_ptr[rows+1]` ascending; `col_idx[nnz]`; pattern only (no values).
 *   - argument order "col before row" in the drop-in signatures (final/SpGEMM_mpi_omp.c:15-18).
 *   - inputs need not have sorted or duplicate-free rows; outputs always have strictly
 *     ascending col_idx per row (the reference sorts every row, :47).
 * Differences: the native API returns C.row_ptr as int64 (the reference's
 * `int` overflows above 2^31-1 output nonzeros); the int32 drop-ins REFUSE (status
 * BSPGEMM_ERR_OVERFLOW, nothing written) instead of wrapping.
 */
#ifndef BSPGEMM_H
#define BSPGEMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status ------------- */
typedef enum bspgemm_status {
    BSPGEMM_OK            = 0,
    BSPGEMM_ERR_INVALID   = 1,   /* bad argument (null pointer, negative size, row range)        */
    BSPGEMM_ERR_ALLOC     = 2,   /* host or device allocation failed                            */
    BSPGEMM_ERR_HIP       = 3,   /* a HIP runtime call failed (see bspgemm_last_error)          */
    BSPGEMM_ERR_NO_DEVICE = 4,   /* no usable gfx950 device: the product has NO CPU fallback    */
    BSPGEMM_ERR_OVERFLOW  = 5,   /* result does not fit the int32 drop-in interface             */
    BSPGEMM_ERR_IO        = 6,   /* file open / parse failure                                   */
    BSPGEMM_ERR_FORMAT    = 7,   /* Matrix Market banner rejected                               */
    BSPGEMM_ERR_COMM      = 8,   /* RCCL failure in the multi-GPU exchange                      */
    BSPGEMM_ERR_SIZE      = 9    /* Matrix Market size line or an entry rejected (the reference
                                    exits without a message there, final/utils.c:60-61)         */
} bspgemm_status;

const char *bspgemm_status_string(bspgemm_status s);
/* text of the last failure on this thread (HIP error string, file:line) */
const char *bspgemm_last_error(void);
/* what this build of the library contains (one line of text).  The shipped library has no
 * timing-only ablation paths: tests/test_abi.py asserts "BSP_ABLATE=0" here.                 */
const char *bspgemm_build_info(void);

/* ---------------------------------------------------------------- native handle API ---
 * Replaces, with device-resident operands and int64 row_ptr, the call
 *     SpGEMM_mpi(Acol,Arow,An, Acol,Arow,An, &nCcol,nCrow,tBlock)   final/SpGEMM_mpi_omp.c:322
 * and the functions under it: SpGEMM_omp :71-143, SpGEMM_bigslice :15-58 (+ quickSort,
 * final/utils.c:159-173, which has no GPU counterpart: rows are emitted in order).
 * Upload once, multiply `times` times, download if wanted -- the reference's timed region
 * (:320-324) likewise excludes I/O and CSR construction.                                     */
/* Threads: a bspgemm_context is NOT thread-safe -- it owns one set of workspaces, one pinned block
 * of read-back scalars and the timing slots of its last 16 multiplies; calls on one context must
 * be serialised by the caller (different contexts, also on one device, are independent).  The
 * int32 drop-ins share one process-wide context behind a mutex.
 * Memory: results freed with bspgemm_result_free go to a per-context cache (at most 8 buffers and a
 * quarter of the device memory) and are handed to the next multiply instead of hipMalloc; the
 * default flow additionally keeps a workspace of F entries (F = products), i.e. about 2F ints live
 * per context after a multiply (10.7 GB for BASELINE config 3).  bspgemm_destroy releases all.
 * Environment (read once, in bspgemm_create; every knob also has a setter, bspgemm_set_option / _set_flow /
 * _set_class_timing, which is what a running program uses): BSPGEMM_FLOW=auto|upper-bound|exact,
 * BSPGEMM_CLASS_STREAMS=1..3, BSPGEMM_CLASS_TIMING=0|1, BSPGEMM_RW_BLK=0|1, BSPGEMM_CHECK, BSPGEMM_SMALL=0|1, BSPGEMM_PAD_ROWS=-1|0|1,
 * BSPGEMM_SHARED_SLOTS=-1|0|k,
 * BSPGEMM_DEBUG_ALLOC, BSPGEMM_DROPIN_TIMING, BSPGEMM_KCORE_TIMING, BSPGEMM_SCC_TIMING, BSPGEMM_COLOR_TIMING, BSPGEMM_BFS_TREE_TIMING, BSPGEMM_LP_TIMING, BSPGEMM_LCC_TIMING=1|2, BSPGEMM_PR_TIMING, BSPGEMM_BC_TIMING, BSPGEMM_EXTRACT_TIMING, BSPGEMM_MATCH_TIMING, BSPGEMM_SSSP_TIMING; BSPGEMM_DEVICE picks the drop-ins' device.  (BSPGEMM_RANK_ROWS=0|1|2 is a
 * development switch of the rank class, read once per process: 0 none, 1 default, 2 also for single-window column counts.)        */
typedef struct bspgemm_context bspgemm_context;   /* one per GPU: device, stream, workspaces  */
typedef struct bspgemm_matrix  bspgemm_matrix;    /* device-resident CSR operand, int32 row_ptr */
typedef struct bspgemm_result  bspgemm_result;    /* device-resident CSR product, int64 row_ptr */

int            bspgemm_device_count(void);       /* visible HIP devices (0 without a GPU)      */
bspgemm_status bspgemm_create(int device, bspgemm_context **ctx);
void           bspgemm_destroy(bspgemm_context *ctx);
/* run on an existing HIP stream (hipStream_t passed as void*; NULL = the context's own) */
bspgemm_status bspgemm_set_stream(bspgemm_context *ctx, void *hip_stream);
bspgemm_status bspgemm_synchronize(bspgemm_context *ctx);

/* Copy a host CSR to the device.  `row_ptr` may be an interior pointer into a larger matrix
 * (values absolute into `col_idx`, like &Arow[rank*tasksize] at final/SpGEMM_mpi_omp.c:171);
 * only col_idx[row_ptr[0] .. row_ptr[rows]) is transferred and the pointers are rebased.     */
bspgemm_status bspgemm_matrix_upload(bspgemm_context *ctx, int rows, int cols,
                                     const int *row_ptr, const int *col_idx,
                                     bspgemm_matrix **out);
/* Adopt device arrays the caller owns (not freed by bspgemm_matrix_free), row_ptr[0] == 0.
 * An operand is IMMUTABLE while the handle lives: the library keeps tables derived from row_ptr and col_idx
 * (row lengths by the byte, blocked extents, a copy of col_idx with every row on a 64-byte boundary) and builds them
 * on first use.  A caller that rewrites
 * the wrapped arrays in place must call bspgemm_matrix_invalidate before the next multiply; a
 * stale table would size rows from old lengths.                                                */
bspgemm_status bspgemm_matrix_wrap_device(bspgemm_context *ctx, int rows, int cols, int64_t nnz,
                                          const int *d_row_ptr, const int *d_col_idx,
                                          bspgemm_matrix **out);
/* drops the derived tables of an operand (they are rebuilt on the next use); synchronises the
 * context's stream first                                                                        */
bspgemm_status bspgemm_matrix_invalidate(bspgemm_matrix *m);
void    bspgemm_matrix_free(bspgemm_matrix *m);
/* Copy an operand to the host as stored: row_ptr[rows+1] (row_ptr[0] = 0) and col_idx[nnz]; either pointer may be
 * NULL to skip that array (like bspgemm_result_download).  m must belong to ctx.  Synchronises the context's stream. */
bspgemm_status bspgemm_matrix_download(bspgemm_context *ctx, const bspgemm_matrix *m,
                                       int *row_ptr /* rows+1, [0] = 0 */, int *col_idx /* nnz */);
/* AT = pattern(A)^T on the device: AT has A.cols rows and A.rows columns, and row k of AT is
 * { i : (i,k) in pattern(A) }, strictly ascending and free of duplicates.  nnz(AT) is the number of distinct pairs
 * (at most nnz(A)); transposing twice gives A with its rows sorted and deduplicated.  The result is deterministic: the
 * pattern of scipy's A.T.tocsr() after sum_duplicates() and sort_indices(), bit for bit.  The reference converts COO
 * to CSC on the host (final/coo2csc.c) and its loader hands back the transpose of the file's matrix that way
 * (final/utils.c:77): a directed graph loaded by bspgemm_readCOO arrives as in-edges, and this call flips it back on
 * the GPU.
 *   - A may come from upload (interior row_ptr included), wrap_device, matrix_from_result or an earlier transpose; its
 *     rows may be unsorted and hold duplicates; any shape, rows == 0, cols == 0 and nnz == 0 included.
 *   - A column outside [0, A.cols) anywhere in A: BSPGEMM_ERR_INVALID, *AT = NULL, bspgemm_last_error names the cause
 *     (the kernels check every column; the context stays usable).  More than 2^31 - 8193 nonzeros: BSPGEMM_ERR_OVERFLOW.
 *   - AT is an owned operand with the layout of an uploaded one (its derived tables as after upload): usable in every
 *     multiply, masked product and closure; release it with bspgemm_matrix_free.  Its col_idx holds nnz(A) + 1 ints.
 *   - Runs on the context's stream and returns when AT is complete, after ONE synchronisation (nnz(AT) is known only
 *     after deduplication).  It does not touch the multiply statistics (bspgemm_last_stats / bspgemm_stats_at).
 *   - Memory: a stable radix sort of the (column, row) pairs by column, 8 bits per pass, in the context's workspace
 *     (kept, like the multiply's): 8 bytes per nonzero of A for one key/value array pair, two pairs when A.cols > 256,
 *     plus 12 bytes per 16 nonzeros for the per-tile digit counts and their scan.  An allocation failure returns
 *     BSPGEMM_ERR_ALLOC and leaks nothing.                                                                              */
bspgemm_status bspgemm_matrix_transpose(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_matrix **AT);
int     bspgemm_matrix_rows(const bspgemm_matrix *m);
int     bspgemm_matrix_cols(const bspgemm_matrix *m);
int64_t bspgemm_matrix_nnz(const bspgemm_matrix *m);

/* Rows [row_begin,row_end) of C = A*B, the job of SpGEMM_bigslice(..., start_row, end_row)
 * (final/SpGEMM_mpi_omp.c:15-58): result row_ptr is slice-local (row_ptr[0] = 0, :26).
 * B.rows must be >= A.cols.  Asynchronous up to the internal size read-backs; the result is
 * complete on the context's stream when the call returns.                                    */
bspgemm_status bspgemm_multiply(bspgemm_context *ctx,
                                const bspgemm_matrix *A, const bspgemm_matrix *B,
                                int row_begin, int row_end, bspgemm_result **C);

/* How bspgemm_multiply gets from row sizes to C.col_idx.  Both give the same CSR, bit for bit.
 *   UPPER_BOUND  rows are placed by their product count F_i (an upper bound of |C_i|) in a workspace
 *                of F entries and squeezed into C.col_idx once the counts are scanned -- the GPU
 *                form of the reference's append-then-concatenate (final/SpGEMM_mpi_omp.c:38-42,
 *                110-131); holds 2F entries.
 *   EXACT        a symbolic pass sizes every row exactly first (the accumulate kernels without their emit half), C.row_ptr
 *                is their scan, and the numeric pass emits every row at its final place: nnz(C)
 *                entries, no F-sized workspace.
 *   AUTO         (default, or env BSPGEMM_FLOW=auto|upper-bound|exact) UPPER_BOUND, and EXACT when its
 *                buffers cannot be allocated.
 * (Round 3 also shipped a third, row-ordered single-pass flow, "FUSED"; it was 4x slower on large products
 * and was taken out in round 4 -- DESIGN.md section 2.1 keeps its measurements.)                  */
#define BSPGEMM_FLOW_AUTO        0
#define BSPGEMM_FLOW_UPPER_BOUND 1
#define BSPGEMM_FLOW_EXACT       2
bspgemm_status bspgemm_set_flow(bspgemm_context *ctx, int flow);

/* Per-class launch brackets (bspgemm_stats: ms_bin, ms_bin_count, t_bin, t_bin_count).  OFF by default (or env
 * BSPGEMM_CLASS_TIMING=1): an event pair around each of a multiply's ~17 class launches keeps consecutive
 * launches of a stream apart (measured: +0.06 ms on BASELINE config 3).  The phase times (ms_prepass ..
 * ms_stitch) are always recorded.  A profiling pass switches this on for the multiplies it wants itemised. */
bspgemm_status bspgemm_set_class_timing(bspgemm_context *ctx, int on);

/* The remaining tuning knobs as calls (the environment variables of the same names are only their initial
 * values).  None of them changes a result, only which kernels produce it -- and bspgemm_stats says which did
 * (prepass_kernel, class_streams, flow, small_path), so that a test can tell that the path it asked for ran.
 *   CLASS_STREAMS    1..3  HIP streams the capacity-class launches of a phase alternate over (default 2)
 *   BLOCKED_EXTENTS  -1 decide per operand (default: B of 2^21 rows or more and not dominated by rows of
 *                    63+ nonzeros), 0 never, 1 always: whether the prepass gathers B's blocked extents table
 *                    instead of B.row_ptr pairs.  Decided when an operand is first used as B, so set it
 *                    before that (or call bspgemm_matrix_invalidate on the operand).
 *   CHECK            0/1   debug checks: the exact flow never emits on unverified sizes, and the accumulate
 *                    kernels verify each row's gathered product count against its capacity class (a stale
 *                    derived table -- see bspgemm_matrix_invalidate -- then fails the multiply with
 *                    BSPGEMM_ERR_INVALID instead of overrunning LDS)
 *   PADDED_ROWS      0 never (default), 1 always, -1 decide per operand (B of 2^20 nonzeros or more with a mean row length
 *                    of 8 or more): the accumulate kernels gather B's rows from a derived copy of B.col_idx in which every
 *                    row starts on a 64-byte boundary (a row then costs ceil(len / 16) 64-byte sectors instead of one
 *                    more; +1.4 x nnz(B) ints of device memory on the bench matrix).  Opt-in: measured worth 8-9 % of the
 *                    numeric phase on matrices whose rows all have 16 entries and nothing on the R-MAT bench matrix
 *                    (DESIGN.md 4.2).  Decided on first use as B, like BLOCKED_EXTENTS.
 *   SMALL_PATH       -1 automatic (default), 0 never, 1 whenever the product may fit: the single-read-back path of few
 *                    launches is tried when the flow is not EXACT (never under it), the range has 1 .. 2^17 rows and the
 *                    WHOLE of A has at most 32768 nonzeros; -1 also needs nnz(A) x B's mean row length <= 32768.  The
 *                    device then checks that the product fits (at most 65536 products, 2048 in any row) and otherwise
 *                    hands it to the general flow (bspgemm_stats.small_path = 0).  No result-cache condition.
 *   SHARED_SLOTS     -1 per capacity class (default), 0 off, k: k in every class (at most 16): the one-wave kernel emits a
 *                    row that has up to that many products more than 32-column slots -- a row whose products sit alone in
 *                    their slots but for a few -- from its columns alone, without building the slots' masks (env
 *                    BSPGEMM_SHARED_SLOTS).  Read at every multiply.
 *   DOT_LIGHT        T >= 0 (default 32): bspgemm_multiply_masked_dot intersects a mask entry whose shorter row has at most T
 *                    entries by one lane, a longer one by a whole wave.  0: every entry with two non-empty rows goes to the
 *                    wave kernel; a very large value: none does (bspgemm_dot_info.heavy_entries says how many did).  Read
 *                    at every call.
 *   BFS_ALPHA, BFS_BETA (>= 1; defaults 15 and 18) and BFS_PUSH_LANES (0 automatic, or 4, 16, 64): the direction rule and the
 *                    lanes per frontier vertex of bspgemm_bfs_tree, described there.  Read at every call.
 *   LP_MIN_CLASS     0 (default) .. 3: the smallest degree class that bspgemm_label_propagation gives a vertex to (0 lane, 1 wave,
 *                    2 workgroup, 3 hub), described there.  It changes no result.  Read at every call.
 *   PR_MIN_CLASS     0 (default) .. 3: the smallest in-degree class that bspgemm_pagerank gives a vertex to under PULL (0 lane,
 *                    1 wave, 2 workgroup, 3 hub), described there.  It changes no result.  Read at every call.
 *   BC_LANES         0 (default): the lanes per vertex of every launch of bspgemm_betweenness follow a quarter of the
 *                    level's mean out-degree; or 4, 16, 64 for every launch of both sweeps.  It changes no result.  Read at
 *                    every call.
 *   EXTRACT_LANES    0 (default): the lanes per out row of the count and the emit of bspgemm_matrix_extract follow a quarter
 *                    of the mean length of the rows read; or 4, 16, 64.  It changes no result.  Read at every call.
 *   MATCH_LANES      0 (default): the lanes per live vertex of the point launches of bspgemm_maximal_matching follow a
 *                    quarter of the mean degree of the vertices that have one; or 4, 16, 64.  It changes no result.  Read at
 *                    every call.  */
typedef enum bspgemm_option {
    BSPGEMM_OPT_CLASS_STREAMS   = 1,
    BSPGEMM_OPT_BLOCKED_EXTENTS = 2,
    BSPGEMM_OPT_CHECK           = 3,
    BSPGEMM_OPT_SMALL_PATH      = 4,
    BSPGEMM_OPT_PADDED_ROWS     = 5,
    BSPGEMM_OPT_SHARED_SLOTS    = 6,
    BSPGEMM_OPT_DOT_LIGHT       = 7,
    BSPGEMM_OPT_BFS_ALPHA       = 8,
    BSPGEMM_OPT_BFS_BETA        = 9,
    BSPGEMM_OPT_BFS_PUSH_LANES  = 10,
    BSPGEMM_OPT_LP_MIN_CLASS    = 11,
    BSPGEMM_OPT_PR_MIN_CLASS    = 12,
    BSPGEMM_OPT_BC_LANES        = 13,
    BSPGEMM_OPT_EXTRACT_LANES   = 14,
    BSPGEMM_OPT_MATCH_LANES     = 15
} bspgemm_option;
bspgemm_status bspgemm_set_option(bspgemm_context *ctx, bspgemm_option opt, int value);
/* current value of a knob (INT32_MIN for an unknown option or a NULL context) */
int            bspgemm_get_option(const bspgemm_context *ctx, bspgemm_option opt);
/* 1 if products with `m` as B gather its blocked extents table, 0 if they gather B.row_ptr pairs, -1 if
 * that has not been decided yet (the operand has not been used as B since it was created / invalidated) */
int            bspgemm_matrix_uses_blocked_table(const bspgemm_matrix *m);
/* the same for the padded copy of col_idx (BSPGEMM_OPT_PADDED_ROWS) */
int            bspgemm_matrix_uses_padded_rows(const bspgemm_matrix *m);

/* C = F .* (A*B), complement convention of SpGEMM_masked (final/SpGEMM_mpi_omp.c:232-288):
 * a column k is admitted to row i only if (i,k) is in F's pattern.
 *   - F is indexed by ABSOLUTE row: F.rows >= row_end and F in ctx, else BSPGEMM_ERR_INVALID with *C = NULL.
 *   - F may have any number of columns, fewer or more than B.cols.  Entries of F at or above B.cols (read as
 *     unsigned: a negative entry too) have no effect: no product can land on them, and no kernel indexes
 *     anything with them.  (The reference indexes a flag array of Bm entries with them; the drop-in
 *     SpGEMM_hip_masked takes them like this call.)
 *   - F's rows may be unsorted and hold repeats; C's rows are ascending and duplicate-free all the same.
 *   - Rows are binned and placed by the mask row's length AS STORED (|C_i| <= |F_i|): repeats and entries at or
 *     above B.cols count towards the class of a row (bspgemm_stats.rows_per_bin, bin_cap).  A row without
 *     products is in class 0, a row of more than 8192 products in a heavy class whatever its mask.
 *   - Flow: always upper-bound placement + compaction (no small path, no EXACT flow).                          */
bspgemm_status bspgemm_multiply_masked(bspgemm_context *ctx,
                                       const bspgemm_matrix *A, const bspgemm_matrix *B,
                                       const bspgemm_matrix *F,
                                       int row_begin, int row_end, bspgemm_result **C);

/* The mask's other half, C = !F .* (A*B) (GraphBLAS C<!M> = A*B): flags = BSPGEMM_MASK_COMPLEMENT keeps the
 * columns of the product that are NOT in F's row -- the inverse of SpGEMM_masked (final/SpGEMM_mpi_omp.c:232-288),
 * which presets its flag array and then clears it on F's columns; here F's columns are the ones cleared.  For rows
 * [row_begin, row_end): C_i = { c in (A*B)_i : (i, c) not in pattern(F) }, ascending and free of duplicates.
 *   - F is indexed by ABSOLUTE row, as in bspgemm_multiply_masked, with the same checks: F.rows >= row_end and
 *     F in ctx, else BSPGEMM_ERR_INVALID.  F's rows may be unsorted, hold duplicates and columns >= B.cols (no effect).
 *   - An empty F gives bspgemm_multiply's result; F = pattern(A*B) an empty one.  For any F, the results of
 *     flags 0 and BSPGEMM_MASK_COMPLEMENT are disjoint and their union is A*B.
 *   - Flow: always upper-bound placement + compaction, like the masked product (no small path, no EXACT flow).
 *     Rows are binned, placed and ordered by their PRODUCT count exactly like the unmasked product (the mask bounds
 *     nothing: |C_i| <= min(products_i, cols)); every class runs the drop twin of its kernel.  BSPGEMM_OPT_PADDED_ROWS,
 *     _BLOCKED_EXTENTS, _CHECK and _CLASS_STREAMS act as on the unmasked upper-bound product.  bspgemm_stats:
 *     flow = BSPGEMM_FLOW_UPPER_BOUND, small_path = 0, rows_per_bin / bin_cap the product classes, products = F.
 * flags = 0 is bspgemm_multiply_masked itself; any other bit is BSPGEMM_ERR_INVALID.                            */
#define BSPGEMM_MASK_COMPLEMENT 1u
bspgemm_status bspgemm_multiply_masked_ex(bspgemm_context *ctx,
                                          const bspgemm_matrix *A, const bspgemm_matrix *B,
                                          const bspgemm_matrix *F, unsigned flags,
                                          int row_begin, int row_end, bspgemm_result **C);

/* C = D | (A*B), the OR-accumulating product of old/BSpGEMM.c:75-126 (SpGEMM_dor; GraphBLAS accum = LOR): a product
 * added to a matrix already held, the step that closures, visited-set BFS and k-hop reachability repeat.  For rows
 * [row_begin, row_end): C_i = { c : (i, c) in pattern(D) and 0 <= c < B.cols } | (A*B)_i, ascending and free of duplicates.
 *   - D is indexed by ABSOLUTE row, like a mask; C.row_ptr is slice-local, as in every multiply.  D's rows may be unsorted
 *     and hold repeats; its entries outside [0, B.cols) are dropped.  Rows with no products still output D's row.
 *   - An empty D gives bspgemm_multiply's result, and so does D = pattern(A*B).  The result equals the plain product of
 *     the stacked operands [A | I] * [B ; D].
 *   - BSPGEMM_ERR_INVALID with *C = NULL: a NULL argument, D from another context, D.rows < row_end, D.cols > B.cols, and
 *     the operand and row-range errors of bspgemm_multiply.
 *   - Flow: always upper-bound placement + compaction (no small path, no EXACT flow, whatever the context asks for).
 *     Rows are binned and placed by products + |D_i|; every class runs the accumulate twin of its kernel, D's row
 *     gathered like one more B row.  bspgemm_stats: flow = BSPGEMM_FLOW_UPPER_BOUND, small_path = 0, products = F (D's
 *     entries not included), rows_per_bin / bin_cap the classes of products + |D_i|, nnz_c = nnz(C).               */
bspgemm_status bspgemm_multiply_accumulate(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                           const bspgemm_matrix *D, int row_begin, int row_end, bspgemm_result **C);

/* C = F .* (A*B) with path counts: the masked product under the PLUS_PAIR semiring (GraphBLAS C<M> = A plus.pair B), the
 * counting form of SpGEMM_masked (final/SpGEMM_mpi_omp.c:232-288), which keeps whether a product lands on a column of F's
 * row and not how many do.  For rows [row_begin, row_end):
 *     C_ij = #{ (p, q) : p indexes a stored entry (i, k) of A, q indexes a stored entry (k, j) of B }
 *            for j in pattern(F_i) and 0 <= j < B.cols, stored only where C_ij > 0.
 *   - Pattern: exactly bspgemm_multiply_masked's on the same arguments (row_ptr, ascending duplicate-free col_idx).  The
 *     values are int32, one per entry of col_idx (bspgemm_result_values_device, bspgemm_result_download_values).
 *   - Repeats: repeated entries of A's or B's rows count as stored (scipy's A1 @ B1 with a 1 per stored entry, duplicates
 *     not merged).  For duplicate-free operands C_ij is the number of k with (i,k) in A and (k,j) in B -- every transpose,
 *     product and bspgemm_matrix_from_result is duplicate-free.  Repeats in F change nothing (a column is a mask column
 *     once); F's columns at or above B.cols have no effect.  Triangles: sum(L .* (L*L)) for L the strictly lower triangle.
 *   - F is indexed by ABSOLUTE row, C.row_ptr is slice-local; F's rows may be unsorted and hold repeats.  The operand, range
 *     and F checks are bspgemm_multiply_masked's: BSPGEMM_ERR_INVALID with *C = NULL.
 *   - A count is at most its row's product count F_i: when any row of the range has F_i > 2^31 - 1 the call returns
 *     BSPGEMM_ERR_OVERFLOW and no result, decided from the prepass before the numeric phase.
 *   - Flow: always upper-bound placement + compaction, like the masked product (no small path, no EXACT flow); rows are
 *     binned and placed by mask-row length and every class runs the counting twin of its kernel.  bspgemm_stats reads as for
 *     the masked product: the same rows_per_bin and bin_cap, flow = BSPGEMM_FLOW_UPPER_BOUND, small_path = 0, products = F,
 *     nnz_c.  The knobs act as on the masked product and change no result.
 * bspgemm_result_free releases the values with the pattern; bspgemm_matrix_from_result takes the pattern only. */
bspgemm_status bspgemm_multiply_masked_count(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                             const bspgemm_matrix *F, int row_begin, int row_end, bspgemm_result **C);

int            bspgemm_result_rows(const bspgemm_result *C);
int64_t        bspgemm_result_nnz(const bspgemm_result *C);
const int64_t *bspgemm_result_row_ptr_device(const bspgemm_result *C);   /* rows+1 entries  */
const int     *bspgemm_result_col_idx_device(const bspgemm_result *C);   /* nnz entries     */
const int     *bspgemm_result_values_device(const bspgemm_result *C);    /* nnz entries; NULL for a pattern-only result */
/* copy to host; either pointer may be NULL to skip that array                                */
bspgemm_status bspgemm_result_download(bspgemm_context *ctx, const bspgemm_result *C,
                                       int64_t *row_ptr, int *col_idx);
/* values[nnz] of a counted result (bspgemm_multiply_masked_count); BSPGEMM_ERR_INVALID for a pattern-only result */
bspgemm_status bspgemm_result_download_values(bspgemm_context *ctx, const bspgemm_result *C, int *values /* nnz */);
void           bspgemm_result_free(bspgemm_result *C);

/* A product becomes the next operand without leaving the GPU (int32 row_ptr copy; fails with
 * BSPGEMM_ERR_OVERFLOW above 2^31-1 nonzeros).  `cols` = number of columns of C (= B.cols).      */
bspgemm_status bspgemm_matrix_from_result(bspgemm_context *ctx, const bspgemm_result *C, int cols,
                                          bspgemm_matrix **out);

/* A stable filter of an operand's entries by their place: out = the entries (r, c) of A that `op` keeps, in A's shape.
 *   - Stable: the kept entries of each row keep their order and repeats are kept -- neither a sort nor a dedup
 *     (transposing twice does that).  The pattern is scipy's tril(A, -1) / triu(A, 1) / both, entry for entry as stored.
 *   - A may come from upload (interior row_ptr included), wrap_device, matrix_from_result, transpose or an earlier select;
 *     any shape, rows == 0 and nnz == 0 included.
 *   - out is an owned operand with the layout of an uploaded one (its derived tables as after upload, nnz + 1 ints of
 *     col_idx): usable in every product; release it with bspgemm_matrix_free.
 *   - Runs on the context's stream with ONE synchronisation (the kept count is known only after the count pass); out is
 *     complete on that stream when the call returns.  It does not touch the multiply statistics.
 *   - Work is spread over entries, not rows (a hub row costs what its entries cost).  Scratch: 12 bytes per 64 entries
 *     of A and the 8-byte scan of the counts, in the context's workspace (kept, like the transpose's).  An allocation
 *     failure returns BSPGEMM_ERR_ALLOC and leaks nothing.
 *   - BSPGEMM_ERR_INVALID with *out = NULL: an unknown op, a NULL argument, A from another context.                     */
typedef enum bspgemm_select { BSPGEMM_SELECT_TRIL = 1,      /* col <  row  (strictly lower) */
                              BSPGEMM_SELECT_TRIU = 2,      /* col >  row  (strictly upper) */
                              BSPGEMM_SELECT_OFFDIAG = 3 }  /* col != row                   */ bspgemm_select;
bspgemm_status bspgemm_matrix_select(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_select op, bspgemm_matrix **out);

/* bspgemm_matrix_from_result with a filter on the values of a counted result (bspgemm_multiply_masked_count): out = the
 * pattern of the entries of C with  value cmp threshold, rows still ascending.  GE with threshold <= 1 gives exactly
 * bspgemm_matrix_from_result's operand (a counted result stores only counts > 0).  `cols` = number of columns of C.
 *   - The int32 limit applies to the KEPT count, not to nnz(C): a result above 2^31 - 1 entries whose selection fits is
 *     accepted (positions are 64-bit inside the kernels); more than INT_MAX kept entries: BSPGEMM_ERR_OVERFLOW, nothing
 *     is leaked.
 *   - BSPGEMM_ERR_INVALID with *out = NULL: a pattern-only result (bspgemm_result_values_device(C) == NULL), an unknown
 *     comparison, a NULL argument, C from another context.
 *   - Stream, synchronisation, scratch, statistics and the finished operand: as bspgemm_matrix_select.                   */
typedef enum bspgemm_compare { BSPGEMM_CMP_GE = 1, BSPGEMM_CMP_GT, BSPGEMM_CMP_LE, BSPGEMM_CMP_LT, BSPGEMM_CMP_EQ, BSPGEMM_CMP_NE } bspgemm_compare;
bspgemm_status bspgemm_matrix_from_result_where(bspgemm_context *ctx, const bspgemm_result *C, int cols,
                                                bspgemm_compare cmp, int threshold, bspgemm_matrix **out);

/* Entry-wise set operations on the PATTERNS of two operands of one shape: row i of out is pattern(A_i) op pattern(B_i).
 *   - out's rows are strictly ascending and duplicate-free, whatever the inputs look like: A and B may come from upload
 *     (interior row_ptr included), wrap_device (arrays that are not 16-byte aligned included), matrix_from_result,
 *     transpose, select or an earlier setop, and their rows may be unsorted and hold repeats.  A == B (one handle) is
 *     allowed.  Any shape, rows == 0, cols == 0 and nnz == 0 on either or both sides included.
 *   - out is an owned operand with the layout of an uploaded one (its derived tables as after upload, nnz + 1 ints of
 *     col_idx): usable in every product, transpose, select and closure; release it with bspgemm_matrix_free.
 *   - Runs on the context's stream; out is complete on that stream when the call returns.  It does not touch the multiply
 *     statistics.  When both operands have sorted duplicate-free rows -- every product, transpose and from_result* has,
 *     and select preserves them -- the call costs ONE synchronisation, the result's size.  The kernels check that form
 *     together with the columns' range; an operand that fails it is first transposed twice (bspgemm_matrix_transpose,
 *     with its synchronisations and workspace) and the passes run again.
 *   - Work is spread over entries, not rows (a hub row costs what its entries cost): each entry is searched in the other
 *     operand's row.  Scratch, in the context's workspace (kept, like the select's): 12 bytes per 64 entries and the 8-byte
 *     scan of the counts for A (OR and XOR: for B too), and for OR and XOR 4 bytes per entry of A and B.
 *   - BSPGEMM_ERR_INVALID with *out = NULL, bspgemm_last_error naming the function and the cause: a NULL argument, an
 *     unknown op, an operand of another context, operands of different shapes, a column outside [0, cols) anywhere in
 *     either operand (the kernels check every column, as the transpose does).  BSPGEMM_ERR_OVERFLOW: the RESULT has more
 *     than INT_MAX entries (OR, XOR; positions are 64-bit inside the kernels).  BSPGEMM_ERR_ALLOC: an allocation failed.
 *     Nothing is leaked and the context stays usable.                                                                     */
typedef enum bspgemm_setop { BSPGEMM_SETOP_OR = 1,      /* A | B:  in A or in B          */
                             BSPGEMM_SETOP_AND = 2,     /* A & B:  in both               */
                             BSPGEMM_SETOP_ANDNOT = 3,  /* A \ B:  in A, not in B        */
                             BSPGEMM_SETOP_XOR = 4 }    /* (A \ B) | (B \ A)             */ bspgemm_setop;
bspgemm_status bspgemm_matrix_setop(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, bspgemm_setop op, bspgemm_matrix **out);

/* *equal = 1 when the two patterns are equal as sets (order and repeats inside a row do not matter), else 0: the answer of
 * nnz(A XOR B) == 0 without a result -- the check and count pass of bspgemm_matrix_setop over A alone, 12 bytes read
 * back.  Shapes, column range, contexts and the treatment of unsorted rows as there; *equal is untouched on failure.      */
bspgemm_status bspgemm_matrix_equal(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, int *equal);

/* out = A | A^T for a square A, rows sorted and duplicate-free; with BSPGEMM_SYMMETRIZE_DROP_DIAGONAL without the
 * diagonal: the simple undirected graph that bspgemm_triangle_count and bspgemm_ktruss expect, e.g. from the in-edges that
 * bspgemm_readCOO hands back for a `general` file.  Composed of bspgemm_matrix_select (OFFDIAG), bspgemm_matrix_transpose
 * and bspgemm_matrix_setop (OR); every intermediate is freed on every path.  BSPGEMM_ERR_INVALID with *out = NULL: a
 * non-square A, any other flag bit, a NULL argument, A from another context; otherwise the errors of the three calls.    */
#define BSPGEMM_SYMMETRIZE_DROP_DIAGONAL 1u
bspgemm_status bspgemm_matrix_symmetrize(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags, bspgemm_matrix **out);

/* Submatrix extraction, GraphBLAS' GrB_extract for patterns: out = A[I, J], on the device, without a product -- a filtered
 * copy that reads every selected row of A once, keeps the entries whose column is selected and writes the new column number.
 *
 * Host lists (bspgemm_matrix_extract).  I (ni entries) and J (nj entries) are host arrays; NULL means "all, in order", and
 * then ni or nj is ignored.
 *   - Default (relabelling) mode: out is ni x nj, and (r, c) in out  <=>  (I[r], J[c]) in pattern(A).  I may be unsorted and
 *     may name a row more than once: the row is then copied that many times.  J may be unsorted.  J must not name a column
 *     twice: BSPGEMM_ERR_INVALID.  So extract(A, p, p) with a permutation p is the relabelled graph, and extract(A, V, V) is the
 *     induced subgraph on V, renumbered by position in V.
 *   - BSPGEMM_EXTRACT_KEEP_SHAPE: out has A's shape, and (i, j) in out  <=>  (i, j) in A, i in set(I) and j in set(J): this is
 *     D_I * A * D_J.  Repeats and order inside either list are harmless.
 *   - Both modes: every row of out is strictly ascending and duplicate-free, whatever A looks like (an upload with an
 *     interior row_ptr, wrapped device arrays off 16-byte alignment, any derived operand; rows unsorted or with repeats).  An A
 *     that fails the canonical check is first canonicalised (transposed twice, as bspgemm_matrix_setop does with its
 *     operands), and info.canonicalised = 1.  out is an owned operand with the layout of an uploaded one: usable in every
 *     product, transpose, select, setop and graph call; release it with bspgemm_matrix_free.  ni == 0, nj == 0, A.rows == 0,
 *     A.cols == 0, nnz == 0 and rectangular A are all valid.  Both lists NULL gives the canonical copy of A.
 *
 * Device lists (bspgemm_matrix_extract_rows_of).  The row list is the stored col_idx of row ri of MI, the column list the same
 * of row rj of MJ; ri == -1 (rj == -1) means the whole col_idx of the operand in storage order, which is what a diagonal
 * selector from bspgemm_matrix_from_result_where holds.  A NULL operand means "all".  The lists never leave the device: only
 * their lengths are read back.  MI and MJ need not have A's shape; their entries must lie in [0, A.rows) and [0, A.cols).
 * Typical uses: row c of the transpose of an assignment operand P is the member list of component, colour or community c;
 * from_result_where(cores, GE, k) with ri = -1 is the k-core's vertex set.  The result is bit for bit that of the host-list
 * call with the same lists.
 *
 * info (may be NULL): kept = nnz(out); scanned = the entries of A that the call looked at, the sum of len(A row I[r]) over r
 * (under KEEP_SHAPE over the distinct rows that I names); hub_chunks = the chunk records written, ceil(len / 4096) for every
 * row read that is longer than 4096 entries; lanes = the lane width that ran; cols_monotone = 1 when the column map
 * preserves order (J NULL, no J[c] < J[c - 1], or KEEP_SHAPE); sorted_by = 0 when no sort was needed (cols_monotone, or
 * nothing kept), 1 when the out rows were sorted in LDS (a wave for rows of up to 256 kept entries, a workgroup for rows of
 * up to 4096), 2 when an out row had more than 4096 kept entries and out went once through two transposes; canonicalised.
 *   - BSPGEMM_OPT_EXTRACT_LANES (0 default, 4, 16, 64), read at every call: the lanes per out row.  It changes no result.
 *     Environment BSPGEMM_EXTRACT_TIMING=1 (read in bspgemm_create): the stage split on stderr (maps and checks, count, hub
 *     launches, scan, read-back two, emit, sort); every stage is then synchronised.
 *   - Runs on the context's stream; out is complete on that stream when the call returns.  It does not touch the multiply
 *     statistics.  Synchronisations: TWO with host lists -- the error bits, scanned and the chunk count; the kept total -- plus
 *     one length read-back for _rows_of (none where ri and rj are -1 or their operand is NULL).  An untidy A adds the
 *     transposes' and one more round.  State: the context's workspace, 4 bytes per column of A (the map), per row of A
 *     (KEEP_SHAPE with a row list), per list entry, and 20 bytes per out row.  No kernel waits for another workgroup.
 *   - BSPGEMM_ERR_INVALID with *out = NULL, a zeroed info and bspgemm_last_error naming the function and the cause: a NULL
 *     ctx, A or out; an unknown flag bit; an operand of another context; ni < 0 or nj < 0 with a list; a list entry outside
 *     its range (the message says which list); a column named twice in J in relabelling mode; ri or rj outside [-1, rows);
 *     a column of A outside [0, A.cols).  Argument errors on host lists are found before anything is launched.
 *     BSPGEMM_ERR_OVERFLOW: more than INT_MAX kept entries, or A above INT_MAX entries.  BSPGEMM_ERR_ALLOC: an allocation
 *     failed.  Nothing is leaked and the context stays usable.                                                            */
#define BSPGEMM_EXTRACT_KEEP_SHAPE 1u
typedef struct bspgemm_extract_info { int64_t kept; int64_t scanned; int64_t hub_chunks; int lanes; int cols_monotone;
                                      int sorted_by; int canonicalised; } bspgemm_extract_info;
bspgemm_status bspgemm_matrix_extract(bspgemm_context *ctx, const bspgemm_matrix *A, int ni, const int *I, int nj,
                                      const int *J, unsigned flags, bspgemm_matrix **out, bspgemm_extract_info *info);
bspgemm_status bspgemm_matrix_extract_rows_of(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *MI,
                                              int ri, const bspgemm_matrix *MJ, int rj, unsigned flags,
                                              bspgemm_matrix **out, bspgemm_extract_info *info);

/* *sum = the exact int64 sum of the values of a counted result, reduced on the device (integer addition: the order does
 * not matter); 8 bytes come back.  A pattern-only result: BSPGEMM_ERR_INVALID, *sum untouched.                           */
bspgemm_status bspgemm_result_values_sum(bspgemm_context *ctx, const bspgemm_result *C, int64_t *sum);

/* Triangles of the undirected simple graph whose edges are the {i, j} with i > j and (i, j) stored in A (A square; for a
 * symmetric A that is A's graph).  The diagonal and the upper triangle are not read, repeated entries count once.
 * L = the strictly lower triangle (bspgemm_matrix_select) with sorted duplicate-free rows (transposed twice),
 * C = L .* (L*L) with counts (bspgemm_multiply_masked_count), *triangles = the sum of C's values: everything stays on the
 * device except the final 8 bytes.  bspgemm_last_stats afterwards describes that counted product.
 * BSPGEMM_ERR_INVALID: a non-square A, a NULL argument, A from another context.                                           */
bspgemm_status bspgemm_triangle_count(bspgemm_context *ctx, const bspgemm_matrix *A, int64_t *triangles);

/* k-truss, everything device-resident (the loop that bspgemm_closure is for squaring): S0 = A without its diagonal, rows
 * sorted and duplicate-free; a step is C = S .* (S*S) with counts over all rows, then S' = the entries of C with a count
 * of k - 2 or more (bspgemm_matrix_from_result_where; the counted product stores only counts > 0 and k - 2 >= 1, so edges
 * without support drop out by themselves).  S' is a subset of S, so equal nnz means equal sets.  A must be square.
 *   - k == 2: T = S0, *iterations = 0, *converged = 1.
 *   - k >= 3: the loop ends when a step removes nothing (*converged = 1, T = that S), when a step leaves nothing
 *     (*converged = 1, T empty, no further product), or after max_iter steps when max_iter > 0 (*converged = 0, T = the
 *     last S').  max_iter <= 0: no cap -- every step but the last removes an entry, so the loop ends.
 *   - *iterations = counted products computed.  iterations and converged may be NULL.
 *   - A symmetric A: T is the k-truss in the usual convention, the maximal subgraph in which every edge lies in at least
 *     k - 2 triangles: symmetric, rows sorted and duplicate-free, nnz(T) = 2 x edges.  A non-symmetric A: T is simply the
 *     fixpoint of the iteration above (symmetry is not checked).
 *   - T is an owned operand (bspgemm_matrix_free).  Any failure inside the loop frees every intermediate.
 *   - BSPGEMM_ERR_INVALID with *T = NULL: k < 2, a non-square A, a NULL argument, A from another context.               */
bspgemm_status bspgemm_ktruss(bspgemm_context *ctx, const bspgemm_matrix *A, int k, int max_iter,
                              bspgemm_matrix **T, int *iterations, int *converged);

/* C = F .* (A * B^T) with counts, the masked DOT product: every mask entry (i, j) gets one intersection of two sorted rows,
 *     C_ij = | pattern(A_i) n pattern(B_j) |   for (i, j) in pattern(F) with 0 <= j < B.rows, stored only where C_ij > 0.
 * The second algorithm of a masked SpGEMM beside the row-wise product of bspgemm_multiply_masked_count: its cost follows
 * the MASK, sum over (i, j) in F of min(|A_i|, |B_j|) searches of log max(|A_i|, |B_j|) steps, not the product count, and
 * B's ROWS are intersected as they are stored -- no transpose when the caller holds them already (L with L for triangles,
 * a symmetric S with itself for the k-truss).
 *   - C has A.rows rows; all of them are computed (no row range).  Its rows are ascending and duplicate-free, its row_ptr
 *     is int64, its values int32.  It is an ordinary counted result, allocated as a product's is: bspgemm_result_download,
 *     _download_values, _values_device, _values_sum and _free work on it unchanged, bspgemm_matrix_from_result and
 *     bspgemm_matrix_from_result_where take it.  It is complete on the context's stream when the call returns.
 *   - For duplicate-free A and B the result is bit for bit that of bspgemm_multiply_masked_count(ctx, A, transpose(B), F,
 *     0, A.rows, &C): row_ptr, col_idx and values.  Counts are taken on PATTERNS: repeats in A, B or F count once (the
 *     counting product counts them as stored).  A == B == F as one handle is allowed.
 *   - Columns of F at or above B.rows (tested unsigned, before they index anything) have no effect.  Columns of A and B
 *     are only compared, never used as an index.
 *   - flags: reserved, must be 0.  info (may be NULL): what ran, below; zeroed on failure.
 *   - Runs on the context's stream with ONE synchronisation when the three operands have sorted duplicate-free rows --
 *     every product, transpose and from_result* has, and select preserves them: the read-back of the checks' error word,
 *     the wave kernel's entry count and nnz(C).  The kernels check that form together with the columns' range, each
 *     distinct handle once; an operand that fails it is first transposed twice (bspgemm_matrix_transpose, with its
 *     synchronisations and workspace), the passes run again and the operand's bit is set in info.canonicalised.
 *   - The mask is walked entry-parallel (a hub row of F costs what its entries cost).  An entry whose shorter row has at
 *     most T = BSPGEMM_OPT_DOT_LIGHT entries is intersected by one lane; a longer one by ONE wave, 64 elements of the
 *     shorter row per step: a hub-hub mask entry is a serial tail of min(|A_i|, |B_j|) / 64 steps of log-deep searches.
 *     One entry is never split across waves.  T changes no result.  Scratch, in the context's workspace (kept, like the
 *     select's): 12 bytes per entry of F (a count and the wave kernel's list) and the select's 12 bytes per 64 entries
 *     with its scan.  It does not touch the multiply statistics.
 *   - BSPGEMM_ERR_INVALID with *C = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A, B, F or C;
 *     flags != 0; an operand of another context; A.cols != B.cols; F.rows != A.rows; a column of F outside [0, F.cols),
 *     or of A or B outside [0, cols) (the check reports them, as bspgemm_matrix_setop does).  BSPGEMM_ERR_ALLOC: an
 *     allocation failed; nothing is leaked and the context stays usable.                                                */
typedef struct bspgemm_dot_info {
    int64_t entries;        /* nnz of the (canonical) mask that was walked                                          */
    int64_t heavy_entries;  /* of them, handled by the one-wave-per-entry kernel                                    */
    int64_t kept;           /* nnz(C)                                                                               */
    int     canonicalised;  /* bit 0 / 1 / 2: A / B / F had to be brought to sorted duplicate-free form first       */
} bspgemm_dot_info;
bspgemm_status bspgemm_multiply_masked_dot(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                           const bspgemm_matrix *F, unsigned flags, bspgemm_result **C,
                                           bspgemm_dot_info *info);

/* bspgemm_triangle_count and bspgemm_ktruss with the way the support is counted as an argument.  BSPGEMM_SUPPORT_PRODUCT
 * is the function without _ex, called through.  BSPGEMM_SUPPORT_DOT counts with bspgemm_multiply_masked_dot:
 *   - triangles: L as there, *triangles = sum(masked_dot(L, L, L)) -- a triangle i > j > k is the entry (i, j) of L together
 *     with k in L_i n L_j, so rows of L meet rows of L and nothing is transposed;
 *   - k-truss: S0 as there; whether S0 equals its transpose is decided once (bspgemm_matrix_transpose,
 *     bspgemm_matrix_equal); a step is C = masked_dot(S, S, S) for a symmetric S0 (S then stays symmetric: the support of
 *     (i, j) is that of (j, i)), else masked_dot(S, transpose(S), S), followed by the same filter and the same stopping
 *     rules.  T, *iterations and *converged equal bspgemm_ktruss's for every A, symmetric or not.
 * Composed of public calls; every intermediate is freed on every path.  The errors of the functions without _ex, and
 * BSPGEMM_ERR_INVALID for an unknown method.  Which method is faster depends on the graph: DESIGN.md 4.17.               */
typedef enum bspgemm_support_method { BSPGEMM_SUPPORT_PRODUCT = 0, BSPGEMM_SUPPORT_DOT = 1 } bspgemm_support_method;
bspgemm_status bspgemm_triangle_count_ex(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_support_method method,
                                         int64_t *triangles);
bspgemm_status bspgemm_ktruss_ex(bspgemm_context *ctx, const bspgemm_matrix *A, int k, int max_iter,
                                 bspgemm_support_method method, bspgemm_matrix **T, int *iterations, int *converged);

/* Multi-source breadth-first search with a level per reached vertex, everything device-resident: the loop the complemented
 * mask is for.  A is square, row u lists the out-neighbours of u; its rows may be unsorted and hold repeats, as for any
 * product operand.  sources: a HOST array of nsources >= 1 vertex ids in [0, A.rows); repeats are allowed and give equal rows.
 *   - *levels is a result object of nsources rows: row s holds the vertices reachable from sources[s], the source itself
 *     included, ascending and duplicate-free like every result; the int32 value of entry (s, v) is the level of v, the
 *     number of edges on a shortest path from sources[s] (0 for the source).  It is an ordinary counted result, allocated as
 *     a product's is: bspgemm_result_download, _download_values, _values_device, _values_sum and _free work on it unchanged,
 *     bspgemm_matrix_from_result gives the reachability rows, bspgemm_matrix_from_result_where the frontier of level d
 *     (BSPGEMM_CMP_EQ, d) or the k-hop neighbourhood (BSPGEMM_CMP_LE, k).  It is complete on the context's stream when the
 *     call returns.
 *   - The loop: V0 = F0 = the nsources x n operand with the one entry (s, sources[s]) per row, level 0.  Level d = 1, 2, ...:
 *     N = !V .* (F*A) (bspgemm_multiply_masked_ex with BSPGEMM_MASK_COMPLEMENT over all rows), the next frontier F = N as an
 *     operand (bspgemm_matrix_from_result), V = V u N with the value d on N's entries.  Cost per level: one complement
 *     product, one bspgemm_matrix_from_result, one merge, and the frees of what they replace.  The merge adds no
 *     synchronisation: V and N are disjoint and sorted by construction, so its size is known before it runs and it needs
 *     no flags, no scan and no read-back -- two entry-parallel launches (a hub row costs what its entries cost) that read
 *     each operand once and search each entry in the other operand's row, and an O(1)-per-row pass for the row_ptr.
 *   - max_depth <= 0: no cap.  max_depth > 0: at most that many products; the result then holds exactly the vertices at
 *     distance <= max_depth.  *depth = the largest level stored.  *complete = 1 when the search ended by itself -- a
 *     frontier came back empty, or every source had reached every vertex (then no further product runs) -- and 0 when the
 *     cap ended it.  depth and complete may be NULL.
 *   - bspgemm_last_stats afterwards describes the last complement product.  The knobs act on the products as always and
 *     change no result.  With BSPGEMM_OPT_CHECK the merge also verifies that N and V are disjoint (one more
 *     synchronisation per level) and fails with BSPGEMM_ERR_HIP if they are not.
 *   - BSPGEMM_ERR_INVALID with *levels = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A, sources
 *     or levels, nsources < 1, a source out of range (its index is reported), a non-square A, A from another context.
 *     BSPGEMM_ERR_OVERFLOW: the visited set would pass INT_MAX entries (it is an int32 operand while the loop runs).  On
 *     every failure path every intermediate is freed and the context stays usable.                                        */
bspgemm_status bspgemm_bfs(bspgemm_context *ctx, const bspgemm_matrix *A, int nsources, const int *sources,
                           int max_depth, bspgemm_result **levels, int *depth, int *complete);

/* Single-source direction-optimising breadth-first search that returns the BFS tree (parents and levels, the Graph500
 * search kernel), everything device-resident and without a product (csrc/bfs_tree.hip).  A is square, row u
 * lists the out-neighbours of u, as for bspgemm_bfs; its rows may be unsorted and hold repeats and self-loops, and it may come
 * from any source of operands.  AT is the transpose of A as bspgemm_matrix_transpose returns it (in-edge rows, ascending and
 * duplicate-free); for a symmetric canonical A the same handle may be passed as AT.  AT == NULL under AUTO or PULL: the call
 * transposes A itself before the first pull launch and frees that transpose on every path (info.transposed).  Under PUSH, AT
 * is ignored and may be NULL.  The library does not check that AT really is the transpose of A: one that is not gives some
 * result, memory-safely.  Its sorted duplicate-free form IS checked, with the check of bspgemm_multiply_masked_dot; an AT that
 * fails it is canonicalised the way that call does it (transposed twice) and info.canonicalised is set.
 *   - *tree is an ordinary counted result of n rows.  Row v of a reached vertex holds exactly one entry: column parent(v)
 *     with the value level(v); the source's row holds (source, source) with the value 0, the Graph500 convention.  Rows of
 *     unreached vertices are empty.  bspgemm_result_download, _download_values, _values_device, _values_sum and _free work on
 *     it unchanged; bspgemm_matrix_from_result gives the tree as a child -> parent operand, whose transpose lists every
 *     vertex's children, and bspgemm_matrix_from_result_where(BSPGEMM_CMP_EQ, d) the vertices of level d with their parents.
 *   - level(v) is the shortest-path distance from the source.  parent(v) is the SMALLEST u with level(u) == level(v) - 1 and
 *     (u, v) stored in A.  Both are unique, so the result is bit for bit the same on every run, for every `direction` and for
 *     every value of the knobs below: this equality is what the tests rest on.
 *   - max_depth as in bspgemm_bfs: <= 0 no cap, else at most that many levels; info.complete = 1 when an empty frontier ended
 *     the search, 0 when the cap did.
 *   - The scheme: level[], parent[], two frontier lists and a counter block in the context's workspace (about 4 n ints, grown
 *     once, before anything is launched).  Level d is ONE launch over the frontier (the vertices of level d - 1; n_f of them
 *     with m_f stored out-edges, both known to the host) and one read-back.  A push launch walks the frontier's rows of A with
 *     W lanes per vertex and claims a neighbour with a device-scope atomicMin on parent[]; a pull launch scans the in-row of
 *     every unreached vertex for its first member of level d - 1.  Both keep all the arrays, so changing direction costs
 *     nothing.  No kernel waits for another workgroup.
 *   - The direction under AUTO, in 64-bit integers, decided before every level from what the host knows: m_u = nnz(A) minus
 *     the out-degrees of every vertex reached so far (frontier included), alpha and beta the options below.  The search
 *     starts in PUSH.  In PUSH it switches to PULL when  m_f * alpha > m_u  and  n_f > the previous level's n_f  (0 before
 *     level 1; without the growth clause the rule flips back to pull on the shrinking tail).  In PULL it switches to PUSH
 *     when  n_f * beta < n.  A host model of this rule predicts info.pull_mask exactly (tests/bfs_tree_ref.py).
 *   - Options, read at every call, none changes a result: BSPGEMM_OPT_BFS_ALPHA (>= 1, default 15), BSPGEMM_OPT_BFS_BETA
 *     (>= 1, default 18), BSPGEMM_OPT_BFS_PUSH_LANES (W: 0 = per level, the smallest of 4, 16, 64 at or above m_f / n_f; or 4,
 *     16 or 64 for every push launch).  Environment BSPGEMM_BFS_TREE_TIMING=1 (read in bspgemm_create): the stage split of
 *     every call on stderr (transpose, push launches, pull launches, read-backs, read-out, the longest launch with its level
 *     and frontier size); it then synchronises twice per launch.
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *tree = NULL, *info zeroed and bspgemm_last_error naming the function and the cause: a NULL
 *     ctx, A or tree (info may be NULL), an unknown direction, a non-square A, source outside [0, n) (which covers n == 0),
 *     an AT of another shape than n x n, an operand of another context, a column of A or AT outside [0, n) (every column is
 *     tested on the device before it indexes anything; the context stays usable).  BSPGEMM_ERR_OVERFLOW: more than INT_MAX
 *     entries in A or AT.  BSPGEMM_ERR_ALLOC: an allocation failed.  Nothing is leaked on any failure path.                */
typedef enum bspgemm_bfs_direction { BSPGEMM_BFS_AUTO = 0, BSPGEMM_BFS_PUSH = 1, BSPGEMM_BFS_PULL = 2 } bspgemm_bfs_direction;
typedef struct bspgemm_bfs_tree_info {
    int64_t  reached;        /* nnz of the result: vertices reached, the source included                    */
    int64_t  edges_pushed;   /* entries of A walked by the push launches (the sum of their m_f)             */
    uint64_t pull_mask;      /* bit d-1 set: level d was produced by a pull launch (levels above 64: none)  */
    int      depth;          /* largest level stored                                                        */
    int      complete;       /* 1: an empty frontier ended the search; 0: max_depth did                     */
    int      push_levels, pull_levels;   /* launches of each kind; their sum = levels attempted             */
    int      transposed;     /* 1: AT was NULL and the call computed (and freed) the transpose itself       */
    int      canonicalised;  /* 1: the AT passed in had unsorted rows or repeats and was brought to form    */
} bspgemm_bfs_tree_info;
bspgemm_status bspgemm_bfs_tree(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT, int source,
                                bspgemm_bfs_direction direction, int max_depth, bspgemm_result **tree,
                                bspgemm_bfs_tree_info *info);

/* Connected components with min-vertex labels, everything device-resident and without a product.  A is square and its
 * entries are read as UNDIRECTED edges: the components are the weakly connected components of the directed graph stored in
 * A (for a symmetric A: its connected components), so no symmetrize is needed and the in-edges that bspgemm_readCOO hands
 * back give the same answer as the file's orientation.  A's rows may be unsorted and hold repeats and self-loops; any n,
 * n == 0 and nnz == 0 included.
 *   - *P is the n x n assignment operand: row v holds exactly one entry, the column label(v) = the smallest vertex id of
 *     v's component.  P.row_ptr = 0, 1, ..., n and P.col_idx[v] = label(v), so bspgemm_matrix_download gives the label
 *     array as col_idx; bspgemm_matrix_transpose(P) holds the ascending member list of component c in row c (an empty row
 *     when c is no label; its row lengths are the component sizes); P^T * A * P by two multiplies is the quotient graph.
 *     It is an owned operand laid out like an uploaded one (bspgemm_matrix_free), complete on the context's stream when
 *     the call returns.
 *   - The labels are the deterministic min-id labelling: bit for bit the same on every run, independent of scheduling.
 *     *ncomponents = the number of v with label(v) == v, counted on the device.  *rounds = hook launches (below); 0 when
 *     nnz == 0 or n == 0.  ncomponents and rounds may be NULL.
 *   - The scheme: a label array parent[] (P.col_idx itself) with parent[x] <= x throughout, and rounds of two kernels.
 *     The hook is entry-parallel over A.col_idx (a hub row costs what its entries cost): an entry (u, v) with different
 *     parent[u] and parent[v] lowers the parent of the larger of the two to the smaller by a device-scope atomicMin.  The
 *     jump replaces every parent[v] by an ancestor a fixed number of steps up.  One read-back of three words per round; the
 *     loop ends with the first round that wrote nothing.  No kernel waits for another workgroup's store, and the result
 *     does not depend on when such stores become visible (csrc/cc.hip).  4 * nnz + 4 * (n + 1) + 8 * n bytes per round and
 *     the gathers of parent[]; a defensive cap of n + 2 rounds (BSPGEMM_ERR_HIP, "did not converge").
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *P = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or P, a
 *     non-square A, A from another context, a column outside [0, n) anywhere in A (every column is tested on the device
 *     before it is used as an index; the context stays usable).  BSPGEMM_ERR_ALLOC: an allocation failed.  Nothing is
 *     leaked on any failure path.                                                                                         */
bspgemm_status bspgemm_connected_components(bspgemm_context *ctx, const bspgemm_matrix *A,
                                            bspgemm_matrix **P, int *ncomponents, int *rounds);

/* k-core decomposition: the core number of every vertex, everything device-resident and without a product.  A is square and
 * its entries are read as UNDIRECTED edges, as bspgemm_connected_components reads them.  The graph is
 * S = bspgemm_matrix_symmetrize(A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL), computed inside the call and freed on every path, so
 * unsorted rows, repeats, self-loops, one-direction storage and the in-edges that bspgemm_readCOO hands back all give the
 * same answer; no flag skips it.  Any n, n == 0 and nnz == 0 included.
 *   - *cores is a counted result of n rows, allocated as a product's is: row v holds exactly one entry, (v, v), whose int32
 *     value is core(v) = the largest k such that v belongs to a subgraph of S in which every vertex has degree >= k; 0 for an
 *     isolated vertex.  bspgemm_result_download, _download_values, _values_device, _values_sum and _free work on it
 *     unchanged; bspgemm_matrix_from_result gives the identity, bspgemm_matrix_from_result_where(cores, n, BSPGEMM_CMP_GE, k)
 *     the diagonal selector D_k of the k-core's vertices and BSPGEMM_CMP_EQ that of the k-shell.  n == 0: a result without
 *     rows.  It is complete on the context's stream when the call returns.
 *   - Core numbers are unique: the result is bit for bit the same on every run, independent of scheduling.
 *     *degeneracy = the largest core number, 0 for n == 0 or a graph without edges.  *rounds = peel launches (below), 0 when
 *     S has no entries.  degeneracy and rounds may be NULL.
 *   - The scheme is level-synchronous peeling on residual degrees deg[] (from S.row_ptr), the result's values as core[]
 *     (-1 = unassigned) and two frontier lists; deg, the lists and four counters live in the context's workspace, about
 *     3 n ints.  Level k: a vertex-parallel scan gives every unassigned v with deg[v] <= k the core number k and appends it
 *     to the frontier (one atomic per wave), and reduces the smallest deg of the vertices it leaves -- exact, no degree
 *     changes in that launch; an empty frontier jumps k to that minimum.  A peel launch gives one wave to every frontier
 *     vertex, its lanes striding over the vertex's row of S: each neighbour's deg is lowered by a device-scope atomicSub, and
 *     the one decrement that returns k + 1 assigns k and appends the neighbour to the other list.  Peel launches swap the
 *     two lists until one comes back empty, then k + 1.  Decisions rest only on atomic return values and on values from
 *     before the launch; no kernel waits for another workgroup, and the result does not depend on when stores become
 *     visible (csrc/kcore.hip).
 *   - Cost: one synchronisation (4 to 16 bytes read back) per scan and per peel launch -- a path of n vertices takes n / 2
 *     peel launches -- at most two scans per distinct core value, every stored entry of S walked once with at most one
 *     atomic.  A frontier vertex's row is walked by ONE wave, 64 entries per step: a hub row in the frontier is a serial
 *     tail, not the "a hub costs what its entries cost" geometry of the entry-parallel passes.  Defensive caps of n peel
 *     launches and 2 n + 2 scans (BSPGEMM_ERR_HIP, "did not converge").
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *cores = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or cores,
 *     a non-square A, A from another context.  Otherwise the errors of bspgemm_matrix_symmetrize: BSPGEMM_ERR_INVALID for a
 *     column outside [0, n) anywhere in A (its transpose tests every column on the device; the context stays usable),
 *     BSPGEMM_ERR_OVERFLOW for more than INT_MAX entries in S, BSPGEMM_ERR_ALLOC.  Nothing is leaked on any path.           */
bspgemm_status bspgemm_core_numbers(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_result **cores, int *degeneracy, int *rounds);

/* The k-core as an operand: T = the subgraph of S (above) induced by {v : core(v) >= k}, n x n, symmetric, rows sorted and
 * duplicate-free, no diagonal; the vertex-side companion of bspgemm_ktruss and the usual filter in front of it.  Composed of
 * public calls on the core numbers: D_k = bspgemm_matrix_from_result_where(cores, n, BSPGEMM_CMP_GE, k), then D_k * S * D_k
 * by two bspgemm_multiply calls with bspgemm_matrix_from_result between them; every intermediate is freed on every path.
 *   - k == 0: T = S.  k > degeneracy: T is the empty n x n operand (D_k itself) and no product runs.
 *   - *degeneracy as bspgemm_core_numbers gives it; may be NULL.  bspgemm_last_stats afterwards describes the last product
 *     that ran.  T is an owned operand (bspgemm_matrix_free), usable in every product.
 *   - BSPGEMM_ERR_INVALID with *T = NULL: k < 0, a NULL ctx, A or T, a non-square A, A from another context; otherwise the
 *     errors of bspgemm_core_numbers and of the calls above.                                                            */
bspgemm_status bspgemm_kcore(bspgemm_context *ctx, const bspgemm_matrix *A, int k, bspgemm_matrix **T, int *degeneracy);

/* Strongly connected components with min-vertex labels, everything device-resident, without a product and without a
 * transpose.  A is square and row u lists the OUT-neighbours of u; two vertices share a component when each reaches the
 * other.  SCCs are invariant under transposition, so the in-edges that bspgemm_readCOO hands back give the same labels as
 * the file's orientation and no bspgemm_matrix_transpose is needed.  A's rows may be unsorted and hold repeats and
 * self-loops (a self-loop is ignored: a vertex is always in its own component); any n, n == 0 and nnz == 0 included.
 *   - *P is the n x n assignment operand, exactly as bspgemm_connected_components returns it: P.row_ptr = 0, 1, ..., n and
 *     P.col_idx[v] = label(v) = the smallest vertex id of v's strongly connected component.  bspgemm_matrix_transpose(P)
 *     holds the ascending member list of component c in row c; P^T * A * P by two multiplies is the condensation, a DAG
 *     apart from its diagonal.  It is an owned operand laid out like an uploaded one (bspgemm_matrix_free), usable in
 *     every product, transpose and select, complete on the context's stream when the call returns.
 *   - The labels are bit for bit the same on every run, independent of scheduling.  *ncomponents = the number of v with
 *     label(v) == v, counted on the device.  *rounds = colouring rounds (below): deterministic, 0 when trimming alone
 *     assigns every vertex (a DAG, nnz == 0, n == 0).  *sweeps = entry-parallel launches in total: it depends on scheduling
 *     and is only bounded (by the caps below); at least 1 when nnz > 0.  ncomponents, rounds and sweeps may be NULL.
 *   - The scheme is trimming plus min-colour propagation (Orzan's colouring, the "Multistep" family), on label[] (P.col_idx
 *     itself, -1 = unassigned) and, in the context's workspace, color[n], two mark arrays of n ints and eight counters.
 *     Trim: an entry-parallel sweep marks has_out[u] and has_in[v] for every entry (u, v), u != v, whose ends are both
 *     unassigned (plain stores); a vertex pass gives every unassigned v that lacks a mark label(v) = v; repeated until a
 *     pass removes nothing.  A colouring round on the rest: color[v] = v; forward sweeps lower color[v] to color[u] over
 *     every entry (u, v) by a device-scope atomicMin, each followed by one pointer jump color[v] = color[color[v]], until
 *     nothing changes -- color[v] is then the smallest vertex that reaches v; the vertices with color[v] == v are the
 *     minima of their components and get label(v) = v; backward sweeps give u the label color[u] over every entry (u, v)
 *     with color[u] == color[v] and v labelled, until a sweep stores nothing.  Trim again, next round.  No kernel waits
 *     for another workgroup's store, and the result does not depend on when such stores become visible (csrc/scc.hip).
 *   - Cost: every sweep is one launch that reads all of A (4 * nnz bytes, the tile's window of row_ptr and the gathers of
 *     the per-vertex arrays) and every repetition ends in one synchronisation with 32 bytes read back.  A directed path of
 *     n vertices takes about n / 2 trim passes, a directed cycle of n vertices n backward sweeps, a chain of k small
 *     components whose ids descend along the edges k rounds.  Defensive caps of n + 2 repetitions of every inner loop and
 *     n rounds (BSPGEMM_ERR_HIP, "did not converge").
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *P = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or P, a
 *     non-square A, A from another context, a column outside [0, n) anywhere in A (every column is tested on the device
 *     before it is used as an index; the context stays usable).  BSPGEMM_ERR_OVERFLOW: more than INT_MAX entries.
 *     BSPGEMM_ERR_ALLOC: an allocation failed.  Nothing is leaked on any failure path.                                    */
bspgemm_status bspgemm_strongly_connected_components(bspgemm_context *ctx, const bspgemm_matrix *A,
                                                     bspgemm_matrix **P, int *ncomponents, int *rounds, int *sweeps);

/* Greedy graph colouring with deterministic colours, everything device-resident and without a product: a partition of
 * the vertices into independent sets, whose first class is a maximal independent set.  A is square and its entries are
 * read as undirected edges exactly as bspgemm_core_numbers reads them: the graph is S = bspgemm_matrix_symmetrize(A,
 * BSPGEMM_SYMMETRIZE_DROP_DIAGONAL), computed inside the call and freed on every path, so unsorted rows, repeats,
 * self-loops, one-direction storage and the in-edges that bspgemm_readCOO hands back all give the same answer; any n,
 * n == 0 and nnz == 0 included.
 *   - The order.  Every vertex has a 64-bit key, key(v) = (hi << 32) | lo, and u PRECEDES v when (key(u), u) < (key(v), v)
 *     lexicographically.  With mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (all in
 *     uint32):
 *         BSPGEMM_COLOR_NATURAL        hi = 0, lo = v                             (seed is ignored)
 *         BSPGEMM_COLOR_RANDOM         hi = 0, lo = mix32((uint32)v ^ seed)
 *         BSPGEMM_COLOR_LARGEST_FIRST  hi = 0x7fffffff - deg_S(v), lo as for RANDOM
 *     The formula is part of the contract: the result is defined by it.
 *   - The result.  colour(v) is what sequential first fit gives when it visits the vertices in that order: the smallest
 *     colour >= 0 that no preceding neighbour of v has.  That is unique, so every run gives the same bits, independent of
 *     scheduling.  It follows that adjacent vertices differ in colour, that a vertex of colour c has a neighbour of every
 *     colour below c, that class 0 is the lexicographically first maximal independent set of the order, and that
 *     *ncolors <= maxdeg(S) + 1.
 *   - *P is the n x n assignment operand, exactly as bspgemm_connected_components returns it: P.row_ptr = 0, 1, ..., n and
 *     P.col_idx[v] = colour(v).  bspgemm_matrix_transpose(P) holds the ascending member list of class c in row c -- row 0
 *     is the maximal independent set -- and P^T * S * P by two multiplies is the class-adjacency matrix, whose diagonal is
 *     empty.  It is an owned operand laid out like an uploaded one (bspgemm_matrix_free), usable in every product,
 *     transpose and select, complete on the context's stream when the call returns.
 *   - *ncolors = 1 + the largest colour, reduced on the device: 0 for n == 0, 1 when S has no entries.  *rounds = frontier
 *     launches (below) = the number of vertices on the longest chain of strictly ascending (key, id) along edges of S:
 *     deterministic, 0 when S has no entries.  ncolors and rounds may be NULL.
 *   - The scheme is a Jones-Plassmann sweep with first fit, a level-synchronous peeling of the priority DAG, on colour[]
 *     (P.col_idx itself, -1 = uncoloured) and, in the context's workspace, key[n], cnt[n] (preceding neighbours not yet
 *     coloured), two frontier lists and four counters, about 5 n ints.  An entry-parallel pass over S counts cnt[]; the
 *     vertices with cnt == 0 seed the frontier (one atomic per wave).  A launch gives one wave to every frontier vertex u,
 *     its lanes striding over u's row of S: the colour of a preceding neighbour is marked in the wave's LDS bitmap of 2048
 *     colours, cnt of a following neighbour is lowered by a device-scope atomicSub and the one decrement that returns 1
 *     appends that neighbour to the other list; the first free bit is u's colour (a full window of 2048 moves the window
 *     up and walks the row again for the colours alone).  Launches swap the two lists until one comes back empty.  Every
 *     preceding neighbour of a frontier vertex was coloured by an EARLIER launch; decisions rest only on atomic return
 *     values and on values from before the launch; no kernel waits for another workgroup (csrc/color.hip).
 *   - Cost: one synchronisation (4 bytes read back) per launch -- a path stored in ascending order takes n launches under
 *     NATURAL -- every stored entry of S walked twice with one atomic each at most.  A frontier vertex's row is walked by
 *     ONE wave, 64 entries per step and once per window pass: a hub row in the frontier is a serial tail, not the "a hub
 *     costs what its entries cost" geometry of the counting pass.  Defensive cap of n launches (BSPGEMM_ERR_HIP, "did not
 *     converge").
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *P = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or P, an
 *     unknown order, a non-square A, A from another context.  Otherwise the errors of bspgemm_matrix_symmetrize:
 *     BSPGEMM_ERR_INVALID for a column outside [0, n) anywhere in A (its transpose tests every column on the device; the
 *     context stays usable), BSPGEMM_ERR_OVERFLOW for more than INT_MAX entries in S, BSPGEMM_ERR_ALLOC.  Nothing is leaked
 *     on any path.                                                                                                         */
typedef enum bspgemm_color_order { BSPGEMM_COLOR_NATURAL = 1, BSPGEMM_COLOR_RANDOM = 2,
                                   BSPGEMM_COLOR_LARGEST_FIRST = 3 } bspgemm_color_order;
bspgemm_status bspgemm_graph_coloring(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_color_order order,
                                      unsigned seed, bspgemm_matrix **P, int *ncolors, int *rounds);

/* Community detection by synchronous label propagation (CDLP as LDBC Graphalytics defines it), everything device-resident
 * and without a product.  A is square and its entries are read as undirected edges exactly as bspgemm_core_numbers and
 * bspgemm_graph_coloring read them: the graph is S = bspgemm_matrix_symmetrize(A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL), computed
 * inside the call and freed on every path, so unsorted rows, repeats, self-loops, one-direction storage and the in-edges
 * that bspgemm_readCOO hands back all give the same answer: an edge counts once however it is stored.
 *   - The definition.  L_0(v) = initial_labels[v], or v when initial_labels == NULL.  For t = 1 .. max_iter, synchronously
 *     (every vertex reads L_(t-1) only): L_t(v) = the smallest label among those that occur most often in the multiset
 *     { L_(t-1)(w) : w in S_v }, and L_t(v) = L_(t-1)(v) when S_v is empty.  The result is L after exactly max_iter
 *     iterations.  The call may stop early at the first iteration that changes no label: that is a fixpoint, so the bits
 *     are the same; it then reports converged = 1.  Counts are integers and the argmax with its tie rule is unique, so
 *     every run gives the same bits, independent of scheduling.
 *   - Synchronous propagation OSCILLATES with period 2 on bipartite components -- a single edge swaps its two labels
 *     forever -- and max_iter is what ends it: the result then depends on whether max_iter is even or odd.  The 2-cycle is
 *     not detected.
 *   - *P is the n x n assignment operand, exactly as bspgemm_connected_components returns it: P.row_ptr = 0, 1, ..., n and
 *     P.col_idx[v] = label(v).  bspgemm_matrix_transpose(P) holds the ascending member list of community c in row c, and
 *     P^T * S * P by two multiplies is the community graph.  It is an owned operand laid out like an uploaded one
 *     (bspgemm_matrix_free), usable in every product, transpose and select, complete on the context's stream when the call
 *     returns.
 *   - initial_labels is a HOST array of n ints in [0, n), or NULL: warm starts and seeded communities.  It is checked on
 *     the host before anything is launched; a value outside [0, n) is BSPGEMM_ERR_INVALID and the message names the
 *     function and the index.  The array is free again when the call returns.
 *   - max_iter == 0: P holds L_0, iterations 0, converged 0.  max_iter < 0: BSPGEMM_ERR_INVALID.  Any n, n == 0 and
 *     nnz == 0 included: when S has no entries (max_iter == 0 or not) the labels are L_0, iterations 0 and converged 1 --
 *     no label can ever change.
 *   - info may be NULL; it is zeroed on failure.  iterations = propagation iterations run, the one that changed nothing
 *     included; converged; communities = distinct labels in the result, counted on the device; changed = vertices whose
 *     label the last iteration changed (0 without an iteration); class_vertices: below.
 *   - The scheme.  S does not change, so its vertices are sorted once per call into four degree classes: lane (1 <= d <= 8,
 *     one lane per vertex, the row's labels in registers), wave (d <= 256, one wave per vertex: the labels gathered into
 *     LDS, sorted there, run lengths by a binary search from each run's last element, (count, label) reduced across the
 *     wave), workgroup (d <= 4096, the same at workgroup scope) and hub (longer: the row's entries are walked
 *     entry-parallel, so a hub costs what its entries cost, and inserted into the hub's own open-addressing table of 2 d
 *     slots in the context's workspace by a device-scope atomicCAS and atomicAdd; a second launch reduces every table to
 *     its argmax).  Every iteration launches each non-empty class over its list, reads the labels of the iteration before
 *     from one array and writes the new ones to another (P.col_idx and one workspace array), and reads back one counter
 *     (64 words that the host sums), its only synchronisation.  Isolated vertices are in no class.  No kernel waits for another workgroup
 *     (csrc/lp.hip).  Workspace: about 7 n ints, and 4 ints per stored entry of a hub's row.
 *   - BSPGEMM_OPT_LP_MIN_CLASS (0 default .. 3), read at every call: a vertex of degree >= 1 runs in the class max(its own,
 *     value) -- a row that fits a smaller class fits every larger one.  It changes no result; class_vertices reports what
 *     ran.  Environment BSPGEMM_LP_TIMING=1 (read in bspgemm_create): the stage split on stderr -- symmetrize, class lists,
 *     the iterations' launches and read-backs, and the longest iteration; it then synchronises twice per iteration.
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *P = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or P,
 *     max_iter < 0, a non-square A, A from another context, an initial label out of range.  Otherwise the errors of
 *     bspgemm_matrix_symmetrize: BSPGEMM_ERR_INVALID for a column outside [0, n) anywhere in A (the context stays usable),
 *     BSPGEMM_ERR_OVERFLOW for more than INT_MAX entries in S, BSPGEMM_ERR_ALLOC.  Nothing is leaked on any path.            */
typedef struct bspgemm_lp_info {
    int     iterations;         /* propagation launches run, the one that changed nothing included          */
    int     converged;          /* 1: an iteration changed no label; 0: max_iter ended it                    */
    int     communities;        /* distinct labels in the result, counted on the device                      */
    int     changed;            /* vertices whose label the last iteration changed                           */
    int64_t class_vertices[4];  /* vertices of S per degree class: [0] lane, [1] wave, [2] workgroup, [3] hub;
                                   isolated vertices are in none                                             */
} bspgemm_lp_info;
bspgemm_status bspgemm_label_propagation(bspgemm_context *ctx, const bspgemm_matrix *A, const int *initial_labels,
                                         int max_iter, bspgemm_matrix **P, bspgemm_lp_info *info);

/* The local clustering coefficient (LCC as LDBC Graphalytics defines it) with an integer count per vertex, everything
 * device-resident and without a product.  A is square and its entries are read exactly as bspgemm_core_numbers reads them:
 * S = bspgemm_matrix_symmetrize(A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL) is computed inside the call and freed on every path,
 * N(v) = S_v and d(v) = |S_v|, so unsorted rows, repeats, self-loops, one-direction storage and the in-edges that
 * bspgemm_readCOO hands back all give the same answer; any n, n == 0 and nnz == 0 included.
 *   - The numerator.  flags == 0 (undirected): num(v) = #{(u, w) : u, w in N(v), u != w, (u, w) in S} = 2 * triangles(v).
 *     flags == BSPGEMM_LCC_DIRECTED (Graphalytics' directed LCC): num(v) = #{(u, w) : u, w in N(v), u != w, (u, w) stored
 *     in A}; repeats count once, and N(v) is still the union of in- and out-neighbours.  The value is invariant under
 *     transposing A -- (u, w) is stored in A^T exactly when (w, u) is stored in A, and the pairs are ordered -- so the
 *     loader's in-edges give the file's answer and no bspgemm_matrix_transpose is needed.  For a symmetric A it equals the
 *     undirected value.  Any other flag bit is BSPGEMM_ERR_INVALID.
 *   - The coefficient.  lcc(v) = 0.0 when d(v) < 2, otherwise (double)num / ((double)d * (double)(d - 1)), computed on the
 *     host in plain C from the read-back integers: bit for bit numpy's num.astype(float64) / (d.astype(float64) *
 *     (d - 1).astype(float64)); no tolerance is involved anywhere.
 *   - The range.  num(v) counts distinct stored entries among v's neighbours, so num(v) <= nnz(S) (undirected) or <= the
 *     number of distinct off-diagonal entries of A (directed); both are <= INT_MAX, or the symmetrize has already failed with
 *     BSPGEMM_ERR_OVERFLOW.  An int32 per vertex is therefore exact, and every partial sum an atomic holds is bounded by
 *     the final value.  Integer addition commutes: every run gives the same bits, independent of scheduling.
 *   - *counts is a counted result of n rows laid out exactly like bspgemm_core_numbers' result: row v holds the one entry
 *     (v, v) with the int32 value num(v); zeros are stored.  bspgemm_result_download, _download_values, _values_device,
 *     _values_sum and _free work on it unchanged; bspgemm_matrix_from_result_where gives vertex selectors.  n == 0: a result
 *     without rows.  It is complete on the context's stream when the call returns.
 *   - degree_host (n ints, d(v)) and lcc_host (n doubles) are HOST arrays; each may be NULL.  info may be NULL; it is zeroed
 *     on failure.  triangles = the triangles of S, each once, summed on the device (= bspgemm_triangle_count(S)).
 *   - The scheme.  Every triangle is walked ONCE, on an oriented half T = bspgemm_matrix_select(S, TRIL) of S, and all three
 *     corners are credited: entry (i, j) of T and a common element k of T_i and T_j are the triangle i > j > k, and the
 *     corner opposite to an edge receives the number of directions that edge is stored in (always 2 when undirected;
 *     DIRECTED: a byte per entry of T, 2 when the entry is in R = A' and A'^T, A' = A without its diagonal, else 1, written
 *     by an entry-parallel search of T's entries in R).  The count is entry-parallel over T in select's geometry: an entry
 *     whose shorter row has at most BSPGEMM_OPT_DOT_LIGHT elements (the masked dot's option; it changes no result) is
 *     intersected by one lane, a longer one is appended to a list and walked by ONE wave in a second launch, 64 elements
 *     of the shorter row per step.  The credits of num[k], one per hit, are summed per workgroup in a cache of 1024 slots
 *     in LDS and reach num[k] by one device-scope atomicAdd per cached k and workgroup (a k whose slot another k holds:
 *     one per hit); num[j] gets one atomic per entry, num[i] one per row and lane; the counts accumulate in the result's
 *     values.  Which half is walked is internal and changes no result.
 *     One synchronisation reads the counters (and the degrees and counts where the caller asked for them).  No kernel
 *     waits for another workgroup (csrc/lcc.hip).  Workspace: 8 bytes per entry of T for the list, one byte per entry for
 *     the weights, in the context's workspace, grown before anything is launched.
 *   - Cost: sum over the entries (i, j) of T of min(|T_i|, |T_j|) searches and one credit per triangle to the counter of
 *     its lowest corner -- on a skewed graph the hubs' counters, which is what the cache is for.  A
 *     hub-hub entry is a serial tail of one wave.  nnz(S) == 0: all zeros, and no intersection kernel is launched.  Environment BSPGEMM_LCC_TIMING=1 (read in
 *     bspgemm_create): the stage split on stderr -- symmetrize and select, weights, count, heavy, finish; it then
 *     synchronises behind every stage (=2: the same on the other half, TRIU, for the comparison).
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *counts = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or
 *     counts, an unknown flag, a non-square A, A from another context.  Otherwise the errors of bspgemm_matrix_symmetrize:
 *     BSPGEMM_ERR_INVALID for a column outside [0, n) anywhere in A (the context stays usable), BSPGEMM_ERR_OVERFLOW for
 *     more than INT_MAX entries in S, BSPGEMM_ERR_ALLOC.  Nothing is leaked on any path.                                      */
#define BSPGEMM_LCC_DIRECTED 1u
typedef struct bspgemm_lcc_info {
    int64_t triangles;      /* triangles of S, each counted once (a by-product, summed on the device)     */
    int64_t entries;        /* entries of the oriented triangle of S that were walked (= nnz(S) / 2)      */
    int64_t heavy_entries;  /* of them, intersected by a whole wave                                       */
    int64_t reciprocal;     /* DIRECTED: edges {i,j} of S stored in both directions in A; else 0          */
} bspgemm_lcc_info;
bspgemm_status bspgemm_local_clustering(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags,
                                        bspgemm_result **counts, int *degree_host, double *lcc_host,
                                        bspgemm_lcc_info *info);

/* PageRank, exact in unsigned 64-bit fixed point, everything device-resident; no product.  Every graph call here promises
 * the same bits on every run, independent of scheduling, and floating-point sums cannot: their order changes the bits.
 * Integer addition commutes, so this definition gives the same bits under pull, under push with atomics, in every degree
 * class and for every split of a hub row, and a numpy model predicts them exactly.
 *   - The definition.  n = A.rows, A is square, row u of A lists the out-neighbours of u; the graph is the pattern of A:
 *     repeats count once, self-loops are kept as stored (a self-loop is an out-edge and an in-edge of its vertex).
 *     outdeg(u) = the number of distinct columns in row u; u is dangling when outdeg(u) == 0.  The constants:
 *         ONE = 2^62,  q = floor(ONE / n),  D = (uint64) floor(damping * 4294967296.0 + 0.5) with 0 <= damping <= 1,
 *         B = ((2^32 - D) * q) >> 32.
 *     r_0(v) = q.  For t = 1 .. max_iter, synchronously, all in uint64:
 *         c(u)   = floor(r_{t-1}(u) / outdeg(u)), and 0 for a dangling u
 *         share  = floor((sum of r_{t-1}(w) over dangling w) / n)
 *         s(v)   = share + sum of c(u) over the distinct u with (u, v) stored
 *         r_t(v) = B + floor(D * s(v) / 2^32)
 *     where D * s(v) / 2^32 is computed as D*(s>>32) + ((D*(s & 0xffffffff))>>32): exact, within 64 bits, no 128-bit
 *     arithmetic.
 *   - The range, an invariant: the sum of r_t over all vertices is at most ONE for every t (floors only lose mass), so every
 *     s(v), every partial sum an atomic holds and the L1 change below stay under 2^63.
 *   - delta_t = sum over v of |r_t(v) - r_{t-1}(v)|.  With tolerance > 0 the loop stops after the first iteration with
 *     delta_t <= floor(tolerance * 2^62), and converged = 1.  With tolerance == 0 it runs exactly max_iter iterations (the
 *     Graphalytics form).  max_iter == 0 gives r_0 with iterations 0.
 *   - rank_fixed_host[v] = r(v); rank_host[v] = ldexp((double) r(v), -62), bit for bit numpy's r.astype(np.float64) * 2.0**-62.
 *     Both are HOST arrays of n entries and each may be NULL.  info may be NULL; it is zeroed on failure.
 *   - Deviation from exact arithmetic: each floor loses less than 2^-62 absolute per contribution, per vertex, per
 *     iteration; nothing more is claimed.  Measured on a CPU against a plain float64 power iteration with the same quantised
 *     damping D / 2^32: the largest relative deviation was 2.0e-13 on R-MAT scale 14 (16384 vertices, 228k edges, 100
 *     iterations), 1.2e-14 on R-MAT scale 11 and 1.5e-14 on a uniform graph.  Graphalytics validates at 1e-4.
 *   - The operands follow bspgemm_bfs_tree.  A is required.  AT is the transpose as bspgemm_matrix_transpose returns it,
 *     or NULL; for a symmetric canonical A the same handle may be passed as AT.  AT is not verified to be the transpose:
 *     a wrong AT gives some result, memory-safely.  A's sorted duplicate-free form is checked with the canonical check of
 *     bspgemm_multiply_masked_dot and bspgemm_bfs_tree; an A that fails it is canonicalised inside the call and
 *     info.canonicalised bit 0 is set; a given AT likewise, bit 1 (the one handle passed as both: both bits).  outdeg(u) is
 *     then the row length of the canonical A.  PULL uses AT's rows and A's row lengths; with AT == NULL it transposes A
 *     before the first launch and frees that transpose on every path (info.transposed = 1).  PUSH uses A alone and
 *     ignores AT.  AUTO is PULL: no regime was measured in which PUSH wins, the transpose included.
 *   - n == 0 and nnz == 0 are valid; every vertex is then dangling and the ranks follow the definition (n == 0: nothing is
 *     written, every sum is empty).
 *   - The scheme (csrc/pagerank.hip).  PULL: the vertices are sorted once per call into four in-degree classes -- one lane
 *     per row of AT of up to 8 entries (0 included), one wave (or a quarter of one) up to 256, one workgroup up to 4096,
 *     and hubs, whose rows are cut into chunks of 4096 entries, one workgroup per chunk, each adding its partial sum to the hub's 64-bit accumulator
 *     by one device-scope atomicAdd, with a small finishing launch behind -- and an iteration is one launch per non-empty
 *     class.  Whoever finishes v computes r_t(v), stores it and c(v) for the next iteration, and feeds delta and the next
 *     dangling sum: there is no separate contribution pass.  PUSH: an entry-parallel walk of A adds c(u) to s(v) by a
 *     device-scope 64-bit atomicAdd, and a vertex-parallel pass finishes.  With tolerance == 0 the loop performs no
 *     read-back and no synchronisation: one synchronisation at the end reads the counters and the ranks.  With tolerance > 0
 *     there is one 8-byte read-back per iteration.  No kernel waits for another workgroup.  The state (r, two c arrays, the
 *     accumulators, the class lists, the counters) lives in the context's workspace, grown once before anything is launched.
 *   - BSPGEMM_OPT_PR_MIN_CLASS (0 default .. 3), read at every call: a vertex runs in the class max(its own, value) under
 *     PULL; a row of in-degree 0 is in the lane class under 0 and moves up like any other.  It changes no result;
 *     info.class_vertices says what ran.  Environment BSPGEMM_PR_TIMING=1 (read in bspgemm_create): the stage split on
 *     stderr -- canonical check, transpose, classify, iterations by class, read-out, the longest iteration; it then
 *     synchronises behind every class launch.
 *   - The multiply statistics (bspgemm_last_stats) are not touched.  The ranks come back in host arrays: a counted result
 *     holds int32 values and cannot hold 64-bit ones, and a device-resident 64-bit valued result type is deliberately out of
 *     scope.
 *   - BSPGEMM_ERR_INVALID, bspgemm_last_error naming the function and the cause, each refused before any operand is
 *     dereferenced: a NULL ctx or A, an unknown method, a damping outside [0, 1] or NaN, max_iter < 0, a tolerance < 0 or
 *     NaN; then a non-square A, an AT that is not n x n, an operand of another context; and a column outside [0, n) in A or
 *     AT, tested on the device before it indexes anything (the context stays usable).  BSPGEMM_ERR_OVERFLOW and
 *     BSPGEMM_ERR_ALLOC as in bspgemm_bfs_tree.  Nothing is leaked on any path.                                              */
typedef enum bspgemm_pr_method { BSPGEMM_PR_AUTO = 0, BSPGEMM_PR_PULL = 1, BSPGEMM_PR_PUSH = 2 } bspgemm_pr_method;
typedef struct bspgemm_pr_info {
    uint64_t mass;              /* sum of the final r(v), <= 2^62                                         */
    uint64_t delta;             /* L1 change of the last iteration run (0 without one)                     */
    int64_t  dangling;          /* vertices with outdeg 0                                                  */
    int64_t  class_vertices[4]; /* PULL: vertices per in-degree class, lane/wave/workgroup/hub; PUSH: 0    */
    int      iterations, converged;   /* converged = 1 only when tolerance > 0 ended the loop              */
    int      method;            /* BSPGEMM_PR_PULL or _PUSH: what ran                                      */
    int      transposed;        /* 1: AT was NULL and the call transposed (and freed) A itself             */
    int      canonicalised;     /* bit 0 / 1: A / AT had unsorted rows or repeats and was brought to form  */
} bspgemm_pr_info;
bspgemm_status bspgemm_pagerank(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT,
                                bspgemm_pr_method method, double damping, int max_iter, double tolerance,
                                uint64_t *rank_fixed_host, double *rank_host, bspgemm_pr_info *info);

/* Betweenness centrality (Brandes) from a list of sources, exact in 64-bit integers, everything device-resident; no product
 * and no transpose.  As with bspgemm_pagerank every contribution is an integer, so the sums are order-free: the same bits on
 * every run, for every lane width and every split of a hub row, and a numpy model predicts them exactly.  Path counts are
 * exact uint64, dependencies are 2^32-scaled integers, and every summand is a pure function of three per-vertex values.
 *   - The definition.  n = A.rows, A is square, row u of A lists the out-neighbours of u; the graph is the pattern of A:
 *     repeats count once, self-loops are stored but never lie on a shortest path.  sources is a HOST array of nsources
 *     vertex ids in [0, n); a vertex named twice counts twice.  ONE = 2^32.  For each source s, in the order given:
 *       forward, exact:  level(s) = 0, sigma(s) = 1; level(v) is the BFS distance from s over A; sigma(v) = the sum of
 *         sigma(u) over the distinct u with (u, v) stored and level(u) == level(v) - 1, in uint64.  If any sigma(v) >= 2^63
 *         the call returns BSPGEMM_ERR_OVERFLOW, writes nothing to the outputs and zeroes info; bspgemm_last_error names
 *         the function, the index of the source in sources, and the level.  (On the device: the atomicAdd on sigma[w]
 *         returns old, and a lane raises the level's flag when old + val has bit 63 set.  Every summand is below 2^63, so
 *         no sum can wrap before some add has raised the flag.)
 *       backward, for d = depth - 1 down to 0, every v with level(v) == d:
 *         c(w)     = (double)(ONE + delta(w)) / (double) sigma(w), computed once per vertex, when delta(w) is final
 *         delta(v) = the sum, over the distinct w with (v, w) stored and level(w) == d + 1, of
 *                    (uint64) floor( c(w) * (double) sigma(v) )
 *         Both conversions round to nearest even; the division and the product are single IEEE-754 double operations,
 *         correctly rounded, with nothing that could fuse.  numpy's astype(np.float64), /, *, np.floor and
 *         astype(np.uint64) give the same bits.  Vertices of the last level have delta = 0.
 *       bc(v) += delta_s(v) for every reached v != s, in uint64.
 *   - The range.  sigma(v) <= sigma(w) along every edge of the BFS DAG, so every summand is at most
 *     (ONE + delta(w)) * (1 + 2^-51), and delta_s(v) < n * ONE * (1 + 2^-40).  The call refuses nsources * n >= 2^31 with
 *     BSPGEMM_ERR_INVALID ("nsources"), which keeps every bc(v) under 2^64.
 *   - bc_fixed_host[v] = bc(v); bc_host[v] = ldexp((double) bc(v), -32), bit for bit numpy's
 *     bc.astype(np.float64) * 2.0**-32.  Both are HOST arrays of n entries and each may be NULL.  info may be NULL; it is
 *     zeroed on failure.
 *   - The meaning.  Brandes' unnormalised betweenness restricted to the given sources: endpoints are excluded, pairs
 *     without a path contribute nothing.  For a symmetric A and all n sources it is TWICE the undirected betweenness.
 *     There is no normalisation flag.
 *   - Deviation from exact rational arithmetic: each summand loses under 2^-32 absolute and about 3 * 2^-53 relative, so
 *     per source |delta_s(v) * 2^-32 - exact| <= m_s * 2^-32 + depth * 2^-50 * exact, m_s the stored edges of the BFS DAG.
 *     Measured on a CPU, the numpy model against networkx 3.4.2 (Brandes in float64), as |fixed * 2^-32 - ref| / max(ref, 1):
 *     2.2e-9 on a symmetrized R-MAT scale 9 (512 vertices, 4545 stored edges, all sources), 2.5e-10 on a directed G(n,p)
 *     (300 vertices, all sources), and from 8 sources 2.1e-9 on a powerlaw-cluster graph (4000 vertices, 47872 stored
 *     edges), 1.5e-9 on a directed R-MAT scale 11, 1.2e-9 on a Barabasi-Albert graph (2000 vertices) and 4.2e-10 on a 30x30
 *     grid; the largest |diff| was 5.2e-6 and every |diff| was at least two orders inside k * m * 2^-32 for k sources
 *     and m stored edges (tests/test_bc_abi.py prints them).
 *   - A's sorted, duplicate-free form is checked with the canonical check of bspgemm_pagerank; an A that fails it is
 *     canonicalised inside the call and info.canonicalised = 1.  Columns outside [0, n) are tested on the device before
 *     they index anything: BSPGEMM_ERR_INVALID, and the context stays usable.
 *   - nsources == 0, n == 0 and nnz == 0 are valid and give zeros.
 *   - The scheme (csrc/betweenness.hip).  The state -- level (int32), sigma, delta, c (double), bc, one order list of n
 *     ints that holds the levels of the current source back to back (Brandes' stack), a hub chunk list and a counter
 *     block, about 44 n bytes -- lives in the context's workspace, grown once before anything is launched; the host keeps
 *     the level offsets.  Forward: level d is one launch over the slice of the order list that holds level d - 1, with W
 *     lanes per vertex (4, 16 or 64, from a quarter of the level's mean out-degree): an unreached w is claimed by an
 *     atomicCAS on its level, the winner appends it behind the list with one atomic per wave, and every entry into level
 *     d does one device-scope 64-bit atomicAdd on sigma[w]; one read-back per level.  Backward: level d is one launch over the same
 *     slice; each lane sums its integer summands, an integer wave reduction follows, and the finishing lane stores
 *     delta[v] and c[v] and adds to bc[v]: no atomics and no read-backs.  A reached row of more than 4096 entries is not
 *     left to one wave: whoever appends such a vertex records its chunks of 4096 entries, a second launch of the level
 *     gives one workgroup per chunk (backward: one device-scope atomicAdd per chunk on delta[v] and a small finishing
 *     launch).  No kernel waits for another workgroup.
 *   - BSPGEMM_OPT_BC_LANES (0 default, 4, 16, 64), read at every call: the lanes per vertex of every launch of both
 *     sweeps.  It changes no result.  Environment BSPGEMM_BC_TIMING=1 (read in bspgemm_create): the stage split on stderr
 *     -- canonical check, forward launches, read-backs, backward launches, hub launches, read-out, the slowest source; it
 *     then synchronises behind every launch group.
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID, bspgemm_last_error naming the function and the cause, each refused before any operand is
 *     dereferenced: a NULL ctx or A, nsources < 0, NULL sources with nsources > 0, a negative source; then, after the
 *     first look at the operands, a non-square A, an operand of another context, a source at or above n, nsources * n >=
 *     2^31.  BSPGEMM_ERR_OVERFLOW also for more than INT_MAX entries, BSPGEMM_ERR_ALLOC when an allocation fails.
 *     Nothing is leaked on any path.                                                                                    */
typedef struct bspgemm_bc_info {
    uint64_t sigma_max;         /* largest path count seen over all sources                                */
    int64_t  reached;           /* sum over sources of vertices reached, the source included               */
    int64_t  edges_forward;     /* entries of A walked by the forward launches                             */
    int64_t  hub_chunks;        /* chunks launched for rows longer than the chunk size, both sweeps        */
    int      sources;           /* number of sources processed                                             */
    int      depth_max;         /* largest depth over all sources                                          */
    int      levels;            /* forward launches over all sources (a level and its hub chunks: one)     */
    int      canonicalised;     /* 1 when A was canonicalised inside the call                              */
} bspgemm_bc_info;
bspgemm_status bspgemm_betweenness(bspgemm_context *ctx, const bspgemm_matrix *A, int nsources, const int *sources,
                                   uint64_t *bc_fixed_host, double *bc_host, bspgemm_bc_info *info);

/* Maximal matching with deterministic mates, everything device-resident and without a product: the third of the colouring /
 * independent-set / matching trio, what multilevel partitioning coarsens a graph with.  A is square and its entries are
 * read as undirected edges exactly as bspgemm_graph_coloring reads them: the graph is S = bspgemm_matrix_symmetrize(A,
 * BSPGEMM_SYMMETRIZE_DROP_DIAGONAL), computed inside the call and freed on every path, so unsorted rows, repeats,
 * self-loops, one-direction storage and the in-edges that bspgemm_readCOO hands back all give the same answer; any n,
 * n == 0 and nnz == 0 included.
 *   - The order.  An edge {a, b} with a < b has a 32-bit key, and the edges are ordered by (key32, a, b)
 *     lexicographically.  With mix32 as bspgemm_graph_coloring defines it (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *     x *= 0x846ca68b; x ^= x >> 16, all in uint32) and h = mix32(mix32((uint32)a ^ seed) ^ (uint32)b):
 *         BSPGEMM_MATCH_NATURAL      key32 = 0                                                  (seed is ignored)
 *         BSPGEMM_MATCH_RANDOM       key32 = h
 *         BSPGEMM_MATCH_LIGHT_FIRST  key32 = (min(deg_S(a) + deg_S(b), 0xffff) << 16) | (h >> 16)
 *     LIGHT_FIRST visits pairs of low degree first, the usual coarsening heuristic.  The formula is part of the contract:
 *     the result is defined by it.
 *   - The result.  The matching that sequential greedy gives when it visits the edges of S in that order and takes an edge
 *     when both of its ends are free.  That is unique, so every run, every lane width and every hub split gives the same
 *     bits.  It is a matching (mate(mate(v)) = v, {v, mate(v)} is an edge of S) and it is maximal: no edge of S has two
 *     unmatched ends.
 *   - *P is the n x n assignment operand, exactly as bspgemm_connected_components returns it: P.row_ptr = 0, 1, ..., n and
 *     P.col_idx[v] = min(v, mate(v)), v itself when v is unmatched.  Every row of P^T then has 0, 1 or 2 entries, and P^T * S * P
 *     by two multiplies is the contracted graph, whose diagonal marks the contracted edges.  It is an owned operand laid out
 *     like an uploaded one (bspgemm_matrix_free), usable in every product, transpose, select and extract, complete on the
 *     context's stream when the call returns.
 *   - mate_host: a host array of n ints, or NULL: mate(v) is v's partner, -1 when v is unmatched.
 *   - info may be NULL; it is zeroed on failure.  rounds, entries_walked and hub_chunks are deterministic as well.
 *   - The scheme is the locally-dominant-edge algorithm: an edge that is the smallest live edge (both ends free) at both of
 *     its ends belongs to the greedy matching.  For a fixed u, comparing (key32, a, b) across its neighbours w equals
 *     comparing (key32, w), so a vertex's candidate is one 64-bit word key32 << 32 | w.  In the context's workspace, grown
 *     once per call: best[n] (64-bit), mate[n], two live lists, the chunk records of the long rows and a counter block,
 *     about 5 n ints.  The first live list holds the vertices of degree > 0.  A round is a POINT launch (4, 16 or 64 lanes per
 *     live vertex u stride over u's row of S; a neighbour w with mate[w] < 0 gives a candidate, and the minimum is stored
 *     in best[u]), for the live rows of more than 4096 entries a HUB launch (one workgroup per chunk of 4096 entries, one
 *     device-scope 64-bit atomicMin per chunk on best[u], so a hub costs what its entries cost), and a PAIR launch (one
 *     thread per live u: without a candidate u retires, unmatched for good; when its candidate w points back, mate[u] = w;
 *     otherwise u is appended to the other list and, if it is a hub, its chunk records are written), then ONE read-back of
 *     8 bytes: the other list's size and its number of chunk records, the grids of the next round.  The lists swap until
 *     one comes back empty.  Decisions rest only on values from earlier launches and on atomic return values; no kernel
 *     waits for another workgroup (csrc/match.hip).
 *   - Cost: one synchronisation per round, and a row is walked AGAIN in every round in which its vertex is still live
 *     (info.entries_walked).  The smallest live edge is matched in every round, so at most n / 2 + 1 rounds run: NATURAL on a
 *     path stored in ascending order takes n / 2, RANDOM took 3 to 7 on the test graphs.  Defensive cap of n
 *     rounds (BSPGEMM_ERR_HIP, "did not converge").
 *   - BSPGEMM_OPT_MATCH_LANES (0 default, 4, 16, 64), read at every call: the lanes per live vertex of the point launches.
 *     It changes no result; info.lanes says what ran.  Environment BSPGEMM_MATCH_TIMING=1 (read in bspgemm_create): the stage
 *     split on stderr -- symmetrize, point launches, hub launches, pair launches, read-backs and the longest round; it then
 *     synchronises behind every launch.
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with *P = NULL, bspgemm_last_error naming the function and the cause: a NULL ctx, A or P and an
 *     unknown order (refused before any operand is dereferenced), a non-square A, A from another context.  Otherwise the
 *     errors of bspgemm_matrix_symmetrize: BSPGEMM_ERR_INVALID for a column outside [0, n) anywhere in A (the context stays
 *     usable), BSPGEMM_ERR_OVERFLOW for more than INT_MAX entries in S, BSPGEMM_ERR_ALLOC.  Nothing is leaked on any path.  */
typedef enum bspgemm_match_order { BSPGEMM_MATCH_NATURAL = 1, BSPGEMM_MATCH_RANDOM = 2,
                                   BSPGEMM_MATCH_LIGHT_FIRST = 3 } bspgemm_match_order;
typedef struct bspgemm_match_info {
    int64_t pairs;            /* matched edges                                                          */
    int64_t entries_walked;   /* sum over rounds of deg_S(u) over the live vertices u of the round       */
    int64_t hub_chunks;       /* chunk records launched over all rounds                                  */
    int     rounds;           /* point launches (below); 0 when S has no entries                         */
    int     lanes;            /* lanes per live vertex that ran: 4, 16 or 64 (0 without a round)         */
} bspgemm_match_info;
bspgemm_status bspgemm_maximal_matching(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_match_order order,
                                        unsigned seed, bspgemm_matrix **P, int *mate_host, bspgemm_match_info *info);

/* Edge weights as a handle: a device-resident array of one uint32 per STORED entry of one operand, what the pattern operands
 * do not carry.  w[k] belongs to stored entry k of A, that is to col_idx[k] as bspgemm_matrix_download shows it; nothing is
 * sorted or deduplicated, so the alignment is never disturbed.  All values 0 .. 2^32 - 1 are legal.
 *   - bspgemm_weights_upload: w_host holds nnz(A) values (it may be NULL when nnz(A) is 0).  The sum is taken on the host.
 *   - bspgemm_weights_hashed generates the weights on the device, in one entry-parallel launch, so that tools and tests need
 *     no weights file.  The formula is part of the contract.  With mix32 as bspgemm_graph_coloring defines it and
 *     (a, b) = (row, col) of the entry, or (min(row, col), max(row, col)) under BSPGEMM_WEIGHTS_SYMMETRIC, so that both
 *     directions of an undirected edge weigh the same:
 *         w = wmin + (uint64) mix32(mix32((uint32)a ^ seed) ^ (uint32)b) % ((uint64)wmax - wmin + 1)
 *     GAP's weights are this with [1, 255].  wmin > wmax and unknown flags are refused.  The sum is an integer reduction
 *     on the device.
 *   - bspgemm_weights_download: the nnz values into w_host.  bspgemm_weights_nnz, bspgemm_weights_sum: the count and the
 *     exact sum of the values (0 for NULL).
 *   - Lifetime.  The handle remembers its context, nnz(A) and A's identity; A is immutable while its handle lives, as
 *     above, and must outlive the calls that take W.  bspgemm_matrix_invalidate(A) knows nothing of weights: after the
 *     wrapped arrays of A were rewritten, W MUST BE REBUILT by the caller.  W does not survive bspgemm_matrix_free(A)
 *     either: the identity is the operand's handle and its col_idx address, which a later operand may be given again, so
 *     free W with A and never pass it on to another operand.  Free W before its context is destroyed.
 *   - The device array goes through the same gate as every device allocation (bspgemm_debug_fail_alloc sees it).
 *     BSPGEMM_ERR_INVALID with *W = NULL: a NULL ctx, A or W, A from another context; BSPGEMM_ERR_OVERFLOW for more than
 *     INT_MAX entries; BSPGEMM_ERR_ALLOC.  Nothing is leaked on any path.  */
typedef struct bspgemm_weights bspgemm_weights;
#define BSPGEMM_WEIGHTS_SYMMETRIC 1u
bspgemm_status bspgemm_weights_upload(bspgemm_context *ctx, const bspgemm_matrix *A, const uint32_t *w_host,
                                      bspgemm_weights **W);
bspgemm_status bspgemm_weights_hashed(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned seed, uint32_t wmin,
                                      uint32_t wmax, unsigned flags, bspgemm_weights **W);
bspgemm_status bspgemm_weights_download(bspgemm_context *ctx, const bspgemm_weights *W, uint32_t *w_host);
int64_t        bspgemm_weights_nnz(const bspgemm_weights *W);
uint64_t       bspgemm_weights_sum(const bspgemm_weights *W);
void           bspgemm_weights_free(bspgemm_weights *W);

/* Single-source shortest paths with unsigned integer lengths, everything device-resident and without a product: the SSSP
 * of LDBC Graphalytics and GAP, by delta-stepping in its near-far form.
 *   - The definition.  A is square, row u lists the out-neighbours of u, and stored entry k = (u, v) has the length w[k]
 *     of W, which was made for A.  dist(v) is the smallest sum of lengths over all walks from `source` to v, in uint64;
 *     dist(source) = 0 and an unreached v has UINT64_MAX.  No sum can wrap: a shortest path has at most n - 1 <= 2^31
 *     edges of at most 2^32 - 1 each.  A repeated entry relaxes more than once and its smallest length wins; a self-loop
 *     never shortens anything; rows need not be sorted.
 *   - parent(source) = source, parent(v) = -1 for an unreached v, and otherwise parent(v) is the SMALLEST u with a stored
 *     entry k = (u, v) for which dist(u) + w[k] == dist(v) (a "tight" entry), found by one pass after the distances are
 *     final.  With all lengths >= 1 the parents form a shortest-path tree.  With zero-length edges parent(v) is still
 *     that well-defined tight predecessor, but zero-length cycles may make the parents CYCLIC (a zero-length self-loop
 *     makes v a tight predecessor of itself): walk them with a bound.
 *   - Both outputs are unique functions of (A, w, source): the same bits on every run and under every delta and lanes.
 *     So are the counts of bspgemm_sssp_info for a given delta, because the rounds are synchronous (below).
 *   - dist_host: a host array of n uint64, or NULL.  parent_host: a host array of n ints, or NULL (the parent pass then
 *     does not run).  params NULL: the defaults.
 *   - params->delta, the bucket width; 0 = the default
 *         delta = max(1, BSPGEMM_SSSP_DELTA_C * (sum / nnz) / max(1, nnz / n)),
 *     integer divisions in exactly this order, sum = bspgemm_weights_sum(W), and 1 when nnz is 0: "lanes x mean length /
 *     mean degree" (Davidson et al., IPDPS 2014).  UINT64_MAX is legal and is Bellman-Ford in one bucket.  info.delta
 *     says what ran.  params->lanes: 0 (default: the smallest of 4, 16, 64 at or above a quarter of the mean stored degree),
 *     4, 16 or 64 lanes per near-list vertex; it changes no result and no count but info.lanes.
 *   - The scheme (csrc/sssp.hip).  T is the exclusive upper end of the open bucket, delta at first.  A vertex is dirty
 *     from the moment it is lowered until its row is walked, and a round's near list holds the dirty vertices below T.
 *     A round is three launches at most: RELAX (W lanes per near vertex u stride over its stored row and send a 64-bit
 *     atomicMin(dist[v], snap[u] + w[k]); snap[u] is u's distance when it was listed, so a round is a pure function of
 *     the state before it; the lane that lowered v lists it as a candidate once per round), HUB (rows of more than 4096
 *     entries: one workgroup per chunk of 4096) and SETTLE (per candidate v: snap[v] = dist[v]; below T it joins the next
 *     near list, otherwise it is pending), then one read-back.  When the near list comes back empty, ADVANCE takes the
 *     exact minimum m of the pending vertices, T = (m / delta + 1) * delta, and a vertex scan moves the pending vertices
 *     below T to the near list; without a pending vertex the search is over.  Every opened bucket is non-empty.  Every
 *     column is tested against [0, n) on the device before it indexes anything.  No kernel waits for another workgroup.
 *   - In-bucket round k finalises the vertices at in-bucket depth k of the shortest-path forest, so a bucket takes at most
 *     (vertices finalised in it) + 1 rounds and the search at most 2 n + 2.  Defensive cap there (BSPGEMM_ERR_HIP, "did not
 *     converge").
 *   - Cost: one synchronisation per round and one per opened bucket.  A small delta walks fewer entries in more rounds; a
 *     high-diameter graph (a grid, a road network) takes about one round per hop and loses to a host Dijkstra
 *     (DESIGN.md 4.25).
 *   - Environment BSPGEMM_SSSP_TIMING=1 (read in bspgemm_create): the stage split on stderr -- relax, hub, settle and advance
 *     launches, read-backs, the parent pass and the longest round; it then synchronises behind every launch.
 *   - The multiply statistics (bspgemm_last_stats) are not touched.
 *   - BSPGEMM_ERR_INVALID with bspgemm_last_error naming the function and the cause, *info zeroed and the host arrays
 *     untouched: a NULL ctx, A or W, a negative source, lanes not in {0, 4, 16, 64} (refused before any operand is
 *     dereferenced); then A or W from another context, a non-square A, a W whose nnz or operand is not A's, a source >= n;
 *     a column outside [0, n) anywhere in A (the context stays usable).  n = 0 returns BSPGEMM_OK with *info zeroed; nnz = 0
 *     reaches the source alone.  BSPGEMM_ERR_ALLOC leaks nothing.  */
#define BSPGEMM_SSSP_DELTA_C 32
typedef struct bspgemm_sssp_params {
    uint64_t delta;           /* bucket width; 0 = the default above                                    */
    int      lanes;           /* 0 default, 4, 16, 64                                                   */
    int      reserved;        /* 0                                                                      */
} bspgemm_sssp_params;
typedef struct bspgemm_sssp_info {
    uint64_t delta;           /* bucket width that ran                                                  */
    uint64_t dist_max;        /* largest finite distance                                                */
    int64_t  reached;         /* vertices with a finite distance, the source included                   */
    int64_t  entries_walked;  /* sum over relax rounds of the stored row lengths of the near list        */
    int64_t  improved;        /* sum over relax rounds of the vertices lowered in the round              */
    int64_t  hub_chunks;      /* chunk records launched over all rounds                                  */
    int      rounds;          /* relax rounds                                                           */
    int      buckets;         /* buckets opened, the first included                                      */
    int      lanes;           /* lanes per near-list vertex that ran: 4, 16 or 64 (0 without a round)    */
    int      reserved;
} bspgemm_sssp_info;
bspgemm_status bspgemm_sssp(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_weights *W, int source,
                            const bspgemm_sssp_params *params, uint64_t *dist_host, int *parent_host,
                            bspgemm_sssp_info *info);

/* Reflexive-transitive closure by repeated boolean squaring, everything device-resident -- the
 * application the reference's report motivates the kernel with (its old/BSpGEMM.c:75-126 keeps
 * an OR-accumulating variant for it): T0 = A or I, T(k+1) = T(k)*T(k) until nnz stops growing
 * (at most max_iter products; ceil(log2 n) suffice).  A must be square.  *iterations = products
 * computed.  The result is T as a product object.                                              */
bspgemm_status bspgemm_closure(bspgemm_context *ctx, const bspgemm_matrix *A, int max_iter,
                               bspgemm_result **T, int *iterations);

/* The closure with flags: 0 is bspgemm_closure itself.  BSPGEMM_CLOSURE_TRANSITIVE computes A+ (paths of length >= 1)
 * instead of A*: T0 = A without the diagonal, T(k+1) = T(k) | T(k)*T(k) by bspgemm_multiply_accumulate (the step of
 * old/BSpGEMM.c:75-126), everything device-resident, until nnz stops growing (the first step never stops it: T0 may
 * hold repeats).  Node i then reaches itself only if it lies on a cycle.  Any other bit is BSPGEMM_ERR_INVALID.     */
#define BSPGEMM_CLOSURE_TRANSITIVE 1u   /* A+ (paths of length >= 1) instead of A* */
bspgemm_status bspgemm_closure_ex(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags, int max_iter,
                                  bspgemm_result **T, int *iterations);

/* Per-row work F_i = sum_{j in A_i} |B_j| ("products", the flag probes of :36-38) as an
 * exclusive prefix over rows [0,A.rows]: prefix[rows] = F.  Used to cut GPU shards at equal
 * work instead of equal row counts (the reference cuts An/numtasks rows, :165). */
bspgemm_status bspgemm_row_work_prefix(bspgemm_context *ctx,
                                       const bspgemm_matrix *A, const bspgemm_matrix *B,
                                       int64_t *prefix_host /* A.rows+1 */);
/* bounds[0..parts] with bounds[0]=0, bounds[parts]=A.rows, equal-F contiguous shards         */
bspgemm_status bspgemm_partition_rows(bspgemm_context *ctx,
                                      const bspgemm_matrix *A, const bspgemm_matrix *B,
                                      int parts, int *bounds);

/* counters of the last bspgemm_multiply* on this context */
#define BSPGEMM_MAX_BINS 20
typedef struct bspgemm_stats {
    int64_t rows;            /* rows multiplied                                              */
    int64_t nnz_a;           /* A nonzeros in those rows                                     */
    int64_t products;        /* F                                                            */
    int64_t nnz_c;           /* output nonzeros                                              */
    int64_t bytes_alg;       /* 4(rows+1)+4nnzA+8nnzA+4F+4nnzC+8(rows+1)     */
    int64_t bytes_read_alg;  /* its HBM-read part: bytes_alg - 4nnzC - 8(rows+1)             */
    int64_t rows_per_bin[BSPGEMM_MAX_BINS]; /* rows per capacity class: [0] empty rows,
                                [1..bins-4] one-wavefront rows with at most bin_cap[b] products,
                                [bins-3] rank rows (2048 < products <= bin_cap: one 512-thread
                                workgroup with a rank bitmap; bin_cap = 2048 where the class is
                                not used), [bins-2], [bins-1] heavy rows (one 512- / 1024-thread
                                workgroup each over dense column windows); rest unused        */
    float   ms_total;        /* hipEvent time of the whole multiply on the stream            */
    float   ms_symbolic;     /* = ms_prepass + ms_count: everything that sizes C.row_ptr     */
    float   ms_prepass;      /*   row work (products per row) + scan + capacity classes      */
    float   ms_count;        /*   exact row sizes (count pass of the one-wave classes, heavy rows) + scan */
    float   ms_numeric;      /* accumulate + emit kernels, rows written at their final place */
    float   ms_stitch;       /* what is left exposed after them (heavy-row move; masked
                                product: count scan + compaction)                            */
    float   ms_bin[BSPGEMM_MAX_BINS];       /* per class: its numeric-phase launch (0 unless bspgemm_set_class_timing) */
    float   ms_bin_count[BSPGEMM_MAX_BINS]; /* per class: its symbolic-phase (count) launch  */
    float   t_bin[BSPGEMM_MAX_BINS];        /* ... and when those launches STARTED, in ms    */
    float   t_bin_count[BSPGEMM_MAX_BINS];  /*     since the multiply began (the class launches
                                               alternate over two streams: with the durations
                                               above this is their timeline)                 */
    int     bins;            /* classes in use, including [0] and the heavy class            */
    int     bin_cap[BSPGEMM_MAX_BINS];      /* products a row of class b may have (masked product:
                                mask-row length); 0 for [0], INT32_MAX for the heavy class   */
    /* which path produced the result (so that a test of a knob can assert that the knob took) */
    int     flow;            /* BSPGEMM_FLOW_UPPER_BOUND or BSPGEMM_FLOW_EXACT: the flow that ran     */
    int     prepass_kernel;  /* 0 k_row_work (B.row_ptr pairs), 1 k_row_work_flat (blocked extents table),
                                2 the single-launch small path's own prepass                          */
    int     class_streams;   /* streams the class launches alternated over                           */
    int     small_path;      /* 1: the single-launch path for small products ran                      */
    int     checked;         /* 1: the device-side capacity guard was armed (BSPGEMM_OPT_CHECK)       */
    int     padded_rows;     /* 1: B's rows were gathered from the padded copy of B.col_idx           */
} bspgemm_stats;
bspgemm_status bspgemm_last_stats(const bspgemm_context *ctx, bspgemm_stats *out);
/* ... and of earlier ones: age 0 = the last multiply, 1 = the one before, ... up to 15.  The
 * HIP events of a multiply are its own, so K timed steps can be read back after the timed region.
 * A small-path attempt that bailed to the general flow is not a multiply of its own: the two share one age. */
bspgemm_status bspgemm_stats_at(const bspgemm_context *ctx, int age, bspgemm_stats *out);

/* ---------------------------------------------------------------- int32 drop-ins ------
 * Same argument lists and ownership as the reference functions they replace: inputs are host
 * arrays and are not modified; `Crow` is caller memory with An+1 ints; `*Ccol` is allocated
 * here with libc malloc so the caller's free() (final/SpGEMM_mpi_omp.c:327) stays valid.
 * The reference functions return void and check nothing; these return a status as well and,
 * on failure, leave *Ccol = NULL and print one line to stderr -- they never fall back to a CPU
 * path.  `tBlock` is accepted and ignored (the GPU grid replaces OpenMP slices).             */

/* replaces SpGEMM_omp, final/SpGEMM_mpi_omp.c:71-74 (all An rows; no divisibility rule) */
int SpGEMM_hip(int *Acol, int *Arow, int An,
               int *Bcol, int *Brow, int Bm,
               int **Ccol, int *Crow, int tBlock);

/* replaces SpGEMM_bigslice, final/SpGEMM_mpi_omp.c:15-18: rows [start_row,end_row), slice-local
 * Crow, *Ccol pre-allocated by the caller with *Csize ints and grown with realloc if needed   */
int SpGEMM_hip_bigslice(int *Acol, int *Arow, int An,
                        int *Bcol, int *Brow, int Bm,
                        int **Ccol, int *Crow, int *Csize,
                        int start_row, int end_row);

/* replaces SpGEMM_mat, Matlab/inc/BSpGEMM.h:2-4 (coder.ceval target, Matlab/SpGEMM.m:9-11):
 * Ccol pre-allocated by the caller with the true nnz                                          */
int SpGEMM_hip_mat(int *Acol, int *Arow, int An,
                   int *Bcol, int *Brow, int Bm,
                   int *Ccol, int *Crow);

/* replaces SpGEMM_masked, final/SpGEMM_mpi_omp.c:232-235 */
int SpGEMM_hip_masked(int *Acol, int *Arow, int An,
                      int *Bcol, int *Brow, int Bm,
                      int *Fcol, int *Frow,
                      int **Ccol, int *Crow, int *Csize);

/* device used by the drop-ins (default 0, or env BSPGEMM_DEVICE) */
int bspgemm_dropin_set_device(int device);

/* ---------------------------------------------------------------- multi-GPU -----------
 * Replaces SpGEMM_mpi, final/SpGEMM_mpi_omp.c:155-225: one process (or thread) per GPU, B
 * replicated, contiguous A-row shards.  The reference gathers nnz, Ccol and Crow on rank 0
 * with MPI_Reduce/Gather/Gatherv (:178-204) and rebases Crow serially (:211-223); here every
 * GPU all-gathers the shard sizes and its local row_ptr over RCCL and rebases on device, so
 * every rank ends with the global C.row_ptr; col_idx stays sharded on the GPUs.
 * The communicator is built from an RCCL unique id that the launcher distributes (MPI,
 * torch.distributed, a file ...): bspgemm_comm_unique_id on rank 0, then bspgemm_comm_create
 * on every rank with the same 128 bytes.                                                      */
typedef struct bspgemm_comm bspgemm_comm;
#define BSPGEMM_UNIQUE_ID_BYTES 128
bspgemm_status bspgemm_comm_unique_id(unsigned char id[BSPGEMM_UNIQUE_ID_BYTES]);
bspgemm_status bspgemm_comm_create(bspgemm_context *ctx, const unsigned char id[BSPGEMM_UNIQUE_ID_BYTES],
                                   int rank, int nranks, bspgemm_comm **comm);
/* The same stitch over a transport the HOST supplies instead of RCCL -- for ranks that share one
 * GPU (RCCL refuses two ranks on a device; `mpirun -n 4` on a one-GPU box is how the reference's
 * `make test` runs, final/Makefile:11-12) and for tests.  Buffers are host memory.  Both
 * callbacks return 0 on success.  allgather: every rank contributes `bytes` bytes, recv gets
 * nranks*bytes, rank-major (MPI_Allgather).  gatherv: rank r contributes send_bytes ==
 * recv_bytes[r]; on `root`, recv gets the concatenation in rank order (MPI_Gatherv, what
 * final/SpGEMM_mpi_omp.c:203 does with Ccol); may be NULL when bspgemm_comm_gather_col_idx /
 * SpGEMM_hip_multi are not used.                                                               */
typedef struct bspgemm_host_transport {
    void *user;
    int (*allgather)(void *user, const void *send, void *recv, size_t bytes);
    int (*gatherv)(void *user, const void *send, size_t send_bytes, void *recv, const size_t *recv_bytes, int root);
} bspgemm_host_transport;
bspgemm_status bspgemm_comm_create_host(bspgemm_context *ctx, const bspgemm_host_transport *transport,
                                        int rank, int nranks, bspgemm_comm **comm);
void           bspgemm_comm_destroy(bspgemm_comm *comm);
/* Collective: every rank passes its own status, every rank gets the worst one.  Run it before a
 * collective that a failed rank would skip -- a rank that leaves the protocol alone leaves the others
 * blocked (the reference's MPI_Gather/Gatherv, final/SpGEMM_mpi_omp.c:178-204, have no such guard).
 * Every RCCL wait of this library is bounded (env BSPGEMM_COMM_TIMEOUT_S, default 120): on a timeout
 * or an asynchronous RCCL error the communicator is aborted and the call returns BSPGEMM_ERR_COMM.  */
bspgemm_status bspgemm_comm_agree(bspgemm_comm *comm, bspgemm_status mine);
/* After such a failure the communicator is DEAD: every later collective call on it (agree, stitch, gather,
 * SpGEMM_hip_multi) returns BSPGEMM_ERR_COMM at once, without touching the transport; destroy it and build a new one.
 * test hook (one-shot): 1 = the next SpGEMM_hip_multi on rank 0 behaves as if its host allocation had failed,
 * 2 = the next bounded RCCL wait behaves as if it had run out (the communicator is aborted), 3 = the next growth of the
 * stitch's staging buffers fails, 4 = the root's device buffer of the next RCCL col_idx gather cannot be allocated */
void           bspgemm_comm_inject_failure(bspgemm_comm *comm, int what);
int            bspgemm_comm_rank(const bspgemm_comm *comm);
int            bspgemm_comm_size(const bspgemm_comm *comm);
/* Second half of a stitch whose collective ran elsewhere (bspgemm/dist.py: torch.distributed):
 * `d_lengths` holds the all-gathered int32 row lengths, rank-major, `width` slots per rank of
 * which bounds[r+1]-bounds[r] are used; writes the global int64 row_ptr (bounds[nranks]+1
 * entries) on the device.  Enqueued on `hip_stream` (a hipStream_t; NULL = HIP's default
 * stream) -- pass the stream the collective was issued on; the context's own stream is not used.
 * Replaces the serial rebase of final/SpGEMM_mpi_omp.c:213-223.                               */
bspgemm_status bspgemm_lengths_to_row_ptr(bspgemm_context *ctx, const int *d_lengths, int nranks, int width,
                                          const int *bounds, int64_t *d_row_ptr, void *hip_stream);
/* The whole stitch: `bounds[nranks+1]` are the shard row bounds every rank used; `local` is this
 * rank's product of rows [bounds[rank],bounds[rank+1]).  Every rank contributes its rows' int32
 * lengths padded to the longest shard, ONE all-gather (RCCL, or the host transport), and
 * bspgemm_lengths_to_row_ptr on the gathered lengths.  On return *d_row_ptr_global points at a
 * device buffer owned by `comm` (bounds[nranks]+1 int64, valid until the next stitch or
 * bspgemm_comm_destroy) holding the global row_ptr on every rank, and shard_nnz[nranks] (host,
 * may be NULL) the per-shard nnz.  Replaces MPI_Reduce + MPI_Gather + MPI_Gather + the serial
 * rebase of final/SpGEMM_mpi_omp.c:178-223 (col_idx stays sharded on the GPUs).               */
bspgemm_status bspgemm_comm_stitch_row_ptr(bspgemm_comm *comm, const bspgemm_result *local,
                                           const int *bounds, const int64_t **d_row_ptr_global,
                                           int64_t *shard_nnz);
/* Root gather of the sharded col_idx, the MPI_Gatherv of final/SpGEMM_mpi_omp.c:203: on `root`,
 * col_idx_host[sum(shard_nnz)] receives the shards in rank order; other ranks pass NULL.
 * shard_nnz as returned by bspgemm_comm_stitch_row_ptr.  Collective: every rank calls it.      */
bspgemm_status bspgemm_comm_gather_col_idx(bspgemm_comm *comm, const bspgemm_result *local,
                                           const int64_t *shard_nnz, int root, int *col_idx_host);
/* replaces SpGEMM_mpi, final/SpGEMM_mpi_omp.c:155-158: the reference's argument list behind the
 * communicator it takes implicitly (MPI_COMM_WORLD).  Every rank passes the whole A and B; the
 * result (*Ccol malloc'ed here, Crow[An+1] caller memory) is valid on rank 0 only (:200-223);
 * other ranks get *Ccol = NULL.  Collective.  Returns a status like the other drop-ins.        */
int SpGEMM_hip_multi(bspgemm_comm *comm, int *Acol, int *Arow, int An,
                     int *Bcol, int *Brow, int Bm,
                     int **Ccol, int *Crow, int tBlock);

/* ---------------------------------------------------------------- test hooks ----------
 * Every device allocation of the library outside the communicator layer (which has bspgemm_comm_inject_failure) passes
 * one gate: the workspaces of a context, the operands and their derived tables, the result buffers and the cache of
 * freed ones.  A result buffer taken from that cache is no allocation and does not pass it.  Pinned and host memory
 * (hipHostMalloc, new, malloc) stay outside.  The gate's state is process-wide and safe to touch from several threads.
 *
 * test hook (one-shot): the `nth` request from now (1 = the next) fails with hipErrorOutOfMemory without calling hipMalloc
 * and leaves its pointer NULL; 0 disarms.  The entry point that made the request returns BSPGEMM_ERR_ALLOC as documented
 * for it -- or succeeds where a fallback is documented: BSPGEMM_FLOW_AUTO runs the exact flow, an optional table is left
 * out, and the retry that follows dropping the result cache is a new request, which may succeed.  The hook leaves no sticky
 * HIP error behind, so what the library does to clear one after a real out-of-memory condition is not exercised by it.    */
void           bspgemm_debug_fail_alloc(int nth);
/* out = {requests so far, live allocations, live bytes, injected failures fired so far}, counted since the process
 * started.  Live: handed out by the gate and not yet freed, buffers held by a context's result cache included; all zero
 * before the first context exists.  Equal live counts before bspgemm_create and after bspgemm_destroy: nothing leaked.  */
void           bspgemm_debug_alloc_state(int64_t out[4]);
/* Three more test hooks of the same gate, for running every entry point on adversarial memory contents.  All are off by
 * default and process-wide like the two above.  With all of them off a request is what it was: one more word read under
 * the lock the gate already takes, hipMalloc and nothing else.
 *
 * fill: while `on` is not 0, every allocation the gate hands out holds copies of `word` before the caller sees it (a
 * trailing 1-3 bytes take the word's low bytes); the fill has completed when the request returns.  A result buffer that
 * comes out of the cache of freed results is no request and is not filled: bspgemm_debug_scribble reaches those.           */
void           bspgemm_debug_fill_alloc(int on, uint32_t word);
/* guard: while `on` is not 0, every request of one byte or more is made 512 bytes larger.  The caller's pointer is 256
 * bytes into it (the 256-byte alignment of hipMalloc is kept), the back zone begins at the first byte past the REQUESTED
 * size -- an overrun of one int is seen even where the request was no multiple of 16 -- and both zones hold a canary byte.
 * Freeing a guarded allocation drains its device and verifies both zones; a changed zone is counted for good.
 * bspgemm_debug_check_guards drains the devices, verifies every live guarded allocation and returns the number damaged so
 * far, the live ones and the ones freed since the hook was last turned on (turning it on from off starts the count again).
 * After a return other than 0, bspgemm_last_error() describes the first damage: "guard damaged: allocation of N bytes,
 * front|back zone, offset K", N as requested, K the first changed byte of that zone.  Call it with no call of the library
 * in flight on another thread.  An allocation keeps its zones until it is freed, whatever the hook says by then.
 * bspgemm_debug_alloc_state goes on counting the requested bytes only.  What the zones see is a store outside a WHOLE
 * allocation: the arrays that one call lays out side by side inside the context's workspace have no gaps between them, and
 * arrays that the caller wraps (bspgemm_matrix_wrap_device) never pass the gate.                                          */
void           bspgemm_debug_guard_alloc(int on);
int64_t        bspgemm_debug_check_guards(void);
/* scribble: waits for the context's streams, fills every scratch array the context keeps between calls with copies of
 * `word`, each to the full size it was allocated with, and waits again.  Scratch is an array whose contents no call is
 * documented to find as an earlier call left them: the per-row block (F, Fmask, Fprefix, partials, hpartials, cnt,
 * bin_tiles, rec, recpre, hub_rec, hub_pre), the grown arrays (ab, tile_row, tmp, tmpv, chunk_row), the scalar blocks
 * (d_prep, d_small, d_small_tiles, bin_count), the scan scratch of bspgemm_lengths_to_row_ptr, and every buffer in the
 * cache of freed results.  A correct call computes the same bits after it as before.  Left out because it is state, not
 * scratch: the device error word of the accumulate kernels (d_err), which bspgemm_create zeroes once (csrc/context.hip:
 * hipMemset(ctx->d_err, 0, 64)) and the kernels only ever OR a bit into; the one reader, a product under
 * BSPGEMM_OPT_CHECK, zeroes its first word again before it looks (csrc/multiply.hip, start_flow).  Operands, their
 * derived tables, weights and live results belong to their handles and are not touched.                                  */
bspgemm_status bspgemm_debug_scribble(bspgemm_context *ctx, uint32_t word);

/* ---------------------------------------------------------------- host utilities (C) --
 * Plain C, no GPU needed.                                                                    */

/* replaces readCOO, final/utils.c:47-81 (with mm_read_banner final/mmio.c:96-179,
 * mm_read_mtx_crd_size :189-217 and coo2csc final/coo2csc.c:22-64): Matrix Market pattern
 * file -> CSR of the TRANSPOSED file matrix (the reference's argument swap at utils.c:77),
 * entries kept in file order inside each row, duplicates kept, square assumed (n = M).
 * The reference exit(1)s on failure (silently for fopen and for the size line, with "Could not
 * process Matrix Market banner." for the banner); this returns BSPGEMM_ERR_IO / _SIZE / _FORMAT
 * so that the CLI can reproduce that behaviour.  Arrays are malloc'd; release with free().     */
bspgemm_status bspgemm_readCOO(const char *path, uint32_t **row, uint32_t **col,
                               uint32_t *M, uint32_t *N, uint32_t *nnz);
/* The same loader with options.  flags = 0 is bspgemm_readCOO.  The
 * reference parses the banner's symmetry token (final/mmio.c:96-179) and then ignores it
 * (final/utils.c:66-71): BSPGEMM_READ_EXPAND_SYMMETRIC mirrors the stored triangle of a
 * symmetric / hermitian / skew-symmetric file so that the CSR holds the full pattern (*nnz is
 * the expanded count).  Off by default: the default result is the reference's, bit for bit.   */
#define BSPGEMM_READ_EXPAND_SYMMETRIC 1u
bspgemm_status bspgemm_readCOO_ex(const char *path, unsigned flags, uint32_t **row, uint32_t **col,
                                  uint32_t *M, uint32_t *N, uint32_t *nnz);
/* writes a CSR as `%%MatrixMarket matrix coordinate pattern general` such that
 * bspgemm_readCOO (and the reference's readCOO) reconstruct exactly this CSR                  */
bspgemm_status bspgemm_write_mtx(const char *path, int rows, int cols,
                                 const int *row_ptr, const int *col_idx);
/* C -> Matrix Market in the FILE's orientation (transposed back), int64 row_ptr              */
bspgemm_status bspgemm_write_result_mtx(const char *path, int rows, int cols,
                                        const int64_t *row_ptr, const int *col_idx);

/* replaces SpGEMM_valid, final/SpGEMM_mpi_omp_validity.c:290-302: exact CSR equality, 1 = same */
int bspgemm_csr_equal(const int *Acol, const int *Arow, const int *Bcol, const int *Brow, int n);
int bspgemm_csr_equal64(const int *Acol, const int64_t *Arow, const int *Bcol, const int64_t *Brow, int n);

/* Seeded synthetic boolean matrices (the reference's inputs came from Matlab
 * sprand via Matlab/write_spm.m:5-8).  Rows sorted, duplicates collapsed.  malloc'd outputs.  */
bspgemm_status bspgemm_gen_uniform(int n, int d, uint64_t seed, int **row_ptr, int **col_idx);
bspgemm_status bspgemm_gen_rmat(int scale, int edge_factor, double a, double b, double c,
                                uint64_t seed, int **row_ptr, int **col_idx);
bspgemm_status bspgemm_gen_powerlaw(int n, int mean_degree, double alpha, int max_degree,
                                    uint64_t seed, int **row_ptr, int **col_idx);

#ifdef __cplusplus
}
#endif
#endif /* BSPGEMM_H */
