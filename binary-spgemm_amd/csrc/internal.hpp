// internal.hpp -- what the translation units behind include/bspgemm.h share: the error macros, the handle
// structs, the builder of derived operands and the operand check that every entry point returning an operand uses, the
// workspace / result-cache helpers (context.hip) that the flows (multiply.hip), the int32 drop-ins (dropin.hip: dropin_run in
// stages -- check and bound, operands, multiply, destination, download, hand-over -- over the early destination that
// early_dest.hpp owns) and the communicator layer (comm.hip) use, the drop-ins' host steps that SpGEMM_hip_multi repeats, the
// flag scratch of select.hip and setop.hip, the host helpers of the round-based graph algorithms (cc.hip to betweenness.hip:
// the operand checks, the canonical checks of A and an optional AT, the read-back of a round, the lanes-per-vertex dispatch,
// the stage clock of their timing modes), and through ws_layout.hpp the cursor that lays their arrays out in ctx->tmp.
// Not installed; nothing here is part of the C ABI.
#pragma once
#include "../../include/bspgemm.h"
#include "kernels.hpp"
#include "ws_layout.hpp"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <new>
#include <type_traits>

// ------------------------------------------------------------------ errors ---------------
// text of the last failure on this thread (bspgemm_last_error); defined in context.hip
extern thread_local char bspgemm_err_text[512];
#define g_err bspgemm_err_text

static inline bspgemm_status fail(bspgemm_status st, const char *what, const char *file, int line)
{
    snprintf(g_err, sizeof g_err, "%s (%s:%d)", what, file, line);
    return st;
}
#define FAIL(st, what) fail((st), (what), __FILE__, __LINE__)
#define HIPCHK(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            snprintf(g_err, sizeof g_err, "%s: %s (%s:%d)", #call, hipGetErrorString(e_),  \
                     __FILE__, __LINE__);                                                  \
            return (e_ == hipErrorOutOfMemory) ? BSPGEMM_ERR_ALLOC : BSPGEMM_ERR_HIP;      \
        }                                                                                  \
    } while (0)
// the same with a clean-up: `bail(status)` must be in scope (frees what the function has built so far)
#define HIPCHK_B(call)                                                                     \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            snprintf(g_err, sizeof g_err, "%s: %s (%s:%d)", #call, hipGetErrorString(e_),  \
                     __FILE__, __LINE__);                                                  \
            return bail((e_ == hipErrorOutOfMemory) ? BSPGEMM_ERR_ALLOC : BSPGEMM_ERR_HIP);\
        }                                                                                  \
    } while (0)

// ------------------------------------------------------------------ device memory (context.hip) ---
// The one gate for device memory: every allocation and release of a device array outside comm.hip (which has hooks of its
// own) goes through this pair -- the workspaces, the operands and their tables, the result buffers and their cache.  It
// counts the live allocations and can fail the n-th request (bspgemm_debug_fail_alloc, include/bspgemm.h), hand every
// allocation out filled with a poison word (bspgemm_debug_fill_alloc) and put a canary zone in front of and behind it
// (bspgemm_debug_guard_alloc: the caller's pointer is then 256 bytes into the hipMalloc'ed block, so only dev_free may
// release it).  A failed request leaves *p NULL.  Pinned (hipHostMalloc) and host memory (new, malloc) stay outside.
hipError_t dev_alloc_bytes(void **p, size_t bytes);
template <class T> static inline hipError_t dev_alloc(T **p, size_t bytes) { return dev_alloc_bytes(reinterpret_cast<void **>(p), bytes); }
hipError_t dev_free(void *p);                           // NULL: nothing

// ------------------------------------------------------------------ objects --------------
using bsp::kNumBins;
using bsp::PrepScalars;
using bsp::RowRec;
struct HostScalars {
    long long totalF;
    long long nnzC;
    int bin_count[kNumBins];
    int a_lo, a_hi;
    long long products;                 // true product count of a masked multiply (totalF is the mask total there)
    long long heavy_total;              // entries the heavy rows may need in the workspace
    PrepScalars prep;                   // upper-bound flow: the prepass results, fetched in one copy
    unsigned err;                       // ctx->d_err, read back when BSPGEMM_OPT_CHECK is on
    bsp::SmallScalars small;            // small path: its one read-back
};

struct bspgemm_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream_b = nullptr;     // second accumulate stream (capacity classes run concurrently)
    hipStream_t stream_c = nullptr;     // compaction stream
    hipEvent_t ev_tile[2][3] = {};                  // per phase (symbolic count, numeric): fork / joins of the side streams
    hipEvent_t ev_join = nullptr;
    // timing events and counters of the last kStatSlots multiplies (bspgemm_stats_at): a caller that
    // times K steps reads K sets of HIP-event brackets afterwards instead of one
    struct StatSlot {
        hipEvent_t ev[5] = {};                      // start / classes known / row sizes known / rows emitted / done
        hipEvent_t ev_cls[2][kNumBins][2] = {};     // per (phase, class): launch brackets
        int R = 0;
        bool cls_timed = false;                     // the class brackets of this multiply were recorded
        int mid_cap = 0, rank_cap = 0;
        HostScalars h = {};
        long long products = 0, nnz_c = 0;
        int cls_n[2][kNumBins] = {};
        bool used = false;
        int flow = 0, prepass_kernel = 0, class_streams = 0;   // which path ran (bspgemm_stats)
        bool small = false, checked = false, padded = false;
    };
    static constexpr int kStatSlots = 16;
    StatSlot slots[kStatSlots];
    int slot_head = 0;                              // the most recent multiply's slot
    long long *stitch_partials = nullptr;           // scan scratch of bspgemm_lengths_to_row_ptr
    size_t stitch_partials_cap = 0;
    // per-row workspace (capacity rows_cap rows)
    size_t rows_cap = 0;
    long long *F = nullptr, *Fprefix = nullptr, *partials = nullptr, *recpre = nullptr, *Fmask = nullptr;
    long long *hpartials = nullptr;     // per scan tile: workspace entries of its heavy rows (scanned)
    RowRec *hub_rec = nullptr;          // the hub rows' records by decreasing products (kHeavySortMax entries)
    long long *hub_pre = nullptr;
    int *cnt = nullptr, *bin_tiles = nullptr, *bin_count = nullptr;
    RowRec *rec = nullptr;
    // per-A-nonzero workspace: (start,length) of the B row behind every A nonzero
    size_t ab_cap = 0;
    int2 *ab = nullptr;
    size_t tile_row_cap = 0;
    int *tile_row = nullptr;            // the flat prepass's first row per tile (ensure_tile_rows)
    // upper-bound placed rows: the heavy rows of a plain product, every row of a masked one
    size_t tmp_cap = 0;
    int *tmp = nullptr;
    size_t tmpv_cap = 0;                // the counting product's values, at the same offsets as tmp
    int *tmpv = nullptr;
    PrepScalars *d_prep = nullptr;      // device side of HostScalars::prep
    bsp::SmallScalars *d_small = nullptr; // device side of HostScalars::small
    bsp::SmallTiles *d_small_tiles = nullptr;   // scan scratch of the small path
    unsigned *d_err = nullptr;          // device error word of the accumulate kernels (kErrCapacity | kErrStaleTable)
    int *chunk_row = nullptr;           // compaction: row of every kCompactGran-th output (left by the count scan)
    size_t chunk_cap = 0;
    HostScalars *h = nullptr;          // pinned
    // freed result buffers, reused by the next multiply (results are allocated per call like the
    // reference's per-call malloc of Ccol, final/SpGEMM_mpi_omp.c:115, without paying hipMalloc)
    struct CachedBuf { void *p; size_t bytes; };
    CachedBuf cache[8] = {};
    size_t cache_budget = 0;            // bytes the cache may pin (a quarter of the device memory)
    int flow = BSPGEMM_FLOW_AUTO;       // bspgemm_set_flow / BSPGEMM_FLOW
    // environment knobs, read ONCE in bspgemm_create (include/bspgemm.h, "Environment")
    bool class_timing = false;          // bspgemm_set_class_timing / BSPGEMM_CLASS_TIMING=1: an event pair around every class launch
    int class_streams = 2;              // BSPGEMM_CLASS_STREAMS: streams the class launches alternate over (measured: 2 -8 %, 3 no better)
    int check = 0;                      // BSPGEMM_CHECK (0/1): the exact flow never emits on unverified sizes
    int rw_blk = -1;                    // BSPGEMM_RW_BLK: 0 never / 1 always use the blocked extents table (default: per operand)
    int pad_rows = 0;                   // BSPGEMM_PAD_ROWS / BSPGEMM_OPT_PADDED_ROWS: 0 never (default), 1 always, -1 per operand: gather from a padded copy of B.col_idx
    int small = -1;                     // BSPGEMM_SMALL / BSPGEMM_OPT_SMALL_PATH: -1 automatic, 0 never, 1 whenever the product fits
    int shared_slots = -1;              // BSPGEMM_SHARED_SLOTS / BSPGEMM_OPT_SHARED_SLOTS: -1 per class (wave_shared_max), 0 off, k: up to k shared slots in every class
    int dot_light = 32;                 // BSPGEMM_OPT_DOT_LIGHT: the longest shorter row that one lane of k_dot_count intersects by itself (dot.hip)
    int bfs_alpha = 15, bfs_beta = 18;  // BSPGEMM_OPT_BFS_ALPHA / _BETA: the direction rule of bspgemm_bfs_tree under AUTO (bfs_tree.hip)
    int bfs_push_lanes = 0;             // BSPGEMM_OPT_BFS_PUSH_LANES: 0 per level from the frontier's mean out-degree, or 4, 16, 64 lanes per frontier vertex
    int lp_min_class = 0;               // BSPGEMM_OPT_LP_MIN_CLASS: 0 .. 3, the smallest degree class of bspgemm_label_propagation (lp.hip)
    int pr_min_class = 0;               // BSPGEMM_OPT_PR_MIN_CLASS: 0 .. 3, the smallest in-degree class of bspgemm_pagerank under PULL (pagerank.hip)
    int bc_lanes = 0;                   // BSPGEMM_OPT_BC_LANES: 0 per level from a quarter of its mean out-degree, or 4, 16, 64 lanes per vertex in both sweeps of bspgemm_betweenness (betweenness.hip)
    int extract_lanes = 0;              // BSPGEMM_OPT_EXTRACT_LANES: 0 from a quarter of the mean length of the rows read, or 4, 16, 64 lanes per out row in the count and the emit of bspgemm_matrix_extract (extract.hip)
    int match_lanes = 0;                // BSPGEMM_OPT_MATCH_LANES: 0 from a quarter of the mean degree of the listed vertices, or 4, 16, 64 lanes per live vertex in the point launches of bspgemm_maximal_matching (match.hip)
    bool debug_alloc = false;           // BSPGEMM_DEBUG_ALLOC: allocation trace on stderr
    bool dropin_timing = false;         // BSPGEMM_DROPIN_TIMING: stage times of the int32 drop-ins on stderr
    bool kcore_timing = false;          // BSPGEMM_KCORE_TIMING: stage times of the k-core peeling on stderr (it then synchronises twice per launch)
    bool scc_timing = false;            // BSPGEMM_SCC_TIMING: trim / forward / backward launch counts and times of the strong components on stderr
    bool bfs_tree_timing = false;       // BSPGEMM_BFS_TREE_TIMING: stage times of the single-source search on stderr (it then synchronises twice per launch)
    bool color_timing = false;          // BSPGEMM_COLOR_TIMING: stage times of the graph colouring on stderr (it then synchronises twice per launch)
    bool lp_timing = false;             // BSPGEMM_LP_TIMING: stage times of the label propagation on stderr (it then synchronises twice per iteration)
    bool pr_timing = false;             // BSPGEMM_PR_TIMING: stage times of the PageRank on stderr (it then synchronises behind every class launch)
    bool bc_timing = false;             // BSPGEMM_BC_TIMING: stage times of the betweenness centrality on stderr (it then synchronises behind every launch group)
    bool extract_timing = false;        // BSPGEMM_EXTRACT_TIMING: stage times of the submatrix extraction on stderr (it then synchronises behind every stage)
    bool match_timing = false;          // BSPGEMM_MATCH_TIMING: stage times of the maximal matching on stderr (it then synchronises behind every launch)
    bool sssp_timing = false;           // BSPGEMM_SSSP_TIMING: stage times of the shortest-path search on stderr (it then synchronises behind every launch)
    int lcc_timing = 0;                // BSPGEMM_LCC_TIMING: 1 stage times of the local clustering on stderr (it then synchronises behind every stage); 2: the same on the half that is not kept (lcc.hip)
};

extern "C" int bspgemm_par_max_plus_one(const int *idx, long long n);              // host/par_copy.c
extern "C" void bspgemm_par_prefault(void *p, size_t bytes);
extern "C" long long bspgemm_par_output_bound(const int *Acol, const int *Arow, int r0, int r1, const int *Brow, int brows, long long cap);

struct bspgemm_matrix {
    bspgemm_context *ctx;
    int rows, cols;
    long long nnz;
    int *d_row_ptr, *d_col_idx;
    bool owned;
    // row lengths clamped to 255, one byte per row: what a product with this matrix as B gathers
    // per A-nonzero to size its rows (csrc/prepass.hip: k_row_products).  Part of the operand's
    // device layout: built when the operand is created (lazily for wrapped device arrays).
    mutable unsigned char *d_deg8 = nullptr;
    // blocked extents table {row_ptr of every 16th row, 16 clamped lengths}: what the prepass gathers per
    // A-nonzero instead of a B.row_ptr pair (csrc/prepass.hip: k_row_work_flat); built on first use as B
    mutable int *d_blk16 = nullptr;
    mutable int blk16_state = 0;          // 0 undecided, 1 in use, 2 not worth it for this operand
    // padded copy of col_idx: every row on a 64-byte boundary (padded to a multiple of 16 entries), so that a gathered B row
    // touches ceil(len / 16) 64-byte sectors instead of one more; built on first use as B (ensure_pad) when it pays
    mutable int *d_col_pad = nullptr;
    mutable int *d_row_ptr_pad = nullptr;  // rows + 1: where row j starts in d_col_pad
    mutable int2 *d_ext = nullptr;         // {start in d_col_pad, length} per row: gathered by k_row_work when there is no blocked table
    mutable int pad_state = 0;             // 0 undecided, 1 in use, 2 not for this operand
    mutable long long nnz_pad = 0;         // entries of d_col_pad (without its 64 of slack): at least 16 when it exists
    // what the accumulate kernels gather from: the padded copy when it exists, and how many entries that array holds
    // (the heavy-row gather picks scalar loads for an array of fewer than four: B->nnz would be wrong for the padded copy)
    const int *gather_col() const { return pad_state == 1 ? d_col_pad : d_col_idx; }
    long long gather_nnz() const { return pad_state == 1 ? nnz_pad : nnz; }
};

bspgemm_status ensure_deg8(const bspgemm_matrix *m);
bspgemm_status ensure_blk16(const bspgemm_matrix *m);
bspgemm_status ensure_pad(const bspgemm_matrix *m);   // before ensure_blk16: the blocked table carries padded bases

// ------------------------------------------------------------------ derived operands (context.hip) ---
// An operand that the library builds on the device (upload, from_result, select, setop, transpose, ...) owns its two
// arrays (owned == true) and is built in three steps, each of which the call site places where its launches and its
// synchronisation want it.  After a failed step *m is NULL or a handle that bspgemm_matrix_free takes, so a caller needs
// one `bail` that frees m, whichever step failed.
bspgemm_status operand_new(bspgemm_context *ctx, int rows, int cols, bspgemm_matrix **m);   // handle (nnz 0) + d_row_ptr
bspgemm_status operand_cols(bspgemm_matrix *m, long long cap);                             // d_col_idx for cap entries
bspgemm_status operand_finish(bspgemm_matrix *m, long long nnz);                           // nnz, and d_deg8 on the stream
// sorted duplicate-free copy of X: transposed twice (transpose.hip)
bspgemm_status operand_canonical(bspgemm_context *ctx, const bspgemm_matrix *X, bspgemm_matrix **out);

// dedup(select(X, op)): the selection with sorted duplicate-free rows, the first step of the triangle count and the
// k-truss under either method (select.hip)
bspgemm_status select_dedup(bspgemm_context *ctx, const bspgemm_matrix *X, bspgemm_select op, bspgemm_matrix **out);

// What an entry point asks of an operand of its context, tested in this order: it belongs to ctx, (NEED_SQUARE) rows ==
// cols, (NEED_ENTRIES_CONSISTENT) an operand with nonzeros has rows and a col_idx.  who: the entry point's name, which the
// message starts with.  BSPGEMM_ERR_INVALID with the text set, or BSPGEMM_OK.
enum : unsigned { NEED_SQUARE = 1u, NEED_ENTRIES_CONSISTENT = 2u };
bspgemm_status check_operand(const bspgemm_context *ctx, const bspgemm_matrix *A, const char *who, unsigned flags);

struct bspgemm_result {
    bspgemm_context *ctx;
    int rows;
    long long nnz;
    long long *d_row_ptr;
    int *d_col_idx;
    long long col_cap;      // entries allocated for d_col_idx (upper bound F >= nnz)
    int *d_values = nullptr;  // bspgemm_multiply_masked_count: the count of every entry, col_cap entries; NULL: pattern only
};

bspgemm_status use_device(bspgemm_context *ctx);

// ------------------------------------------------------------------ workspace (context.hip) ---
bspgemm_status ensure_rows(bspgemm_context *ctx, size_t rows);
bspgemm_status ensure_ab(bspgemm_context *ctx, size_t pairs);
bspgemm_status ensure_tile_rows(bspgemm_context *ctx, size_t items);
bspgemm_status ensure_tmp(bspgemm_context *ctx, size_t ints);
bspgemm_status ensure_tmpv(bspgemm_context *ctx, size_t ints);
bspgemm_status ensure_chunk_rows(bspgemm_context *ctx, size_t entries);
// result buffers: best fit from the context's cache of freed results, else hipMalloc
bool result_cached(const bspgemm_context *ctx, size_t bytes);
hipError_t result_alloc(bspgemm_context *ctx, void **out, size_t bytes);
void result_release(bspgemm_context *ctx, void *p, size_t bytes);
static inline size_t result_bytes_rowptr(int rows) { return ((size_t)rows + 1) * sizeof(long long); }
static inline size_t result_bytes_colidx(long long nnz) { return ((size_t)nnz + 4) * sizeof(int); }
// A counted result of `rows` rows with exactly `entries` entries (nnz == col_cap == entries), nothing written yet: the
// handle, then d_row_ptr, d_col_idx and d_values by result_alloc, in that order.  After a failure *R is NULL or a handle
// that bspgemm_result_free takes, so the caller's `bail` frees it whichever step failed.
bspgemm_status counted_result_new(bspgemm_context *ctx, int rows, long long entries, bspgemm_result **R);

// Scratch of the flag-word passes over E entries (select.hip, setop.hip), carved from ctx->tmp (kept between calls, like
// the transpose's): the flag words (one per 64 entries, whole tiles), the int64 scan of their counts, the scan's partials,
// the counts, and (lbs) an int per entry in whole tiles.
struct FlagScratch {
    unsigned long long *flags;
    long long *pre, *part;
    int *cnt, *lbs;
    int words;
};
// Lays the scratch of E entries out from int offset `at` of tmp, every array on a 16-byte boundary, and returns the end;
// 0: more words than the scan's int count takes.  sc NULL: the end alone (what to ask ensure_tmp for: tmp may move).
size_t flag_scratch_carve(int *tmp, size_t at, long long E, bool lbs, FlagScratch *sc);
// ints of the workspace that a transpose of E entries with `cols` columns takes (transpose.hip; 0: none, or E is refused),
// and the most that bspgemm_matrix_symmetrize of an n x n operand of E entries takes over all its stages (setop.hip)
size_t transpose_workspace_ints(long long E, int cols);
size_t symmetrize_workspace_ints(long long E, int n);

// ------------------------------------------------------------------ round-based algorithms (cc.hip, scc.hip, kcore.hip, color.hip, bfs_tree.hip, lp.hip, lcc.hip, pagerank.hip, betweenness.hip, extract.hip, match.hip, sssp.hip) ---
// What the host side of the algorithms that repeat launches until a read-back says "done" shares: the operand checks, the
// grids (vertex_grid, grid_for), the lanes per vertex (lanes_for_mean, dispatch_lanes), the read-back (round_reset,
// round_fetch, frontier_head_ok), the failures, the stage clock and the symmetrize opening (symmetrized_operand).  The device
// side of the same algorithms is wave.hpp and hub_chunks.hpp.  The loops themselves are each algorithm's own, and so is what
// it does about an untidy operand.  who: the entry point's name, which every message starts with.
// the graph operand: check_operand with `flags`, then an entry count that an int32 entry index cannot hold
static inline bspgemm_status check_graph_operand(const bspgemm_context *ctx, const bspgemm_matrix *A, const char *who, unsigned flags)
{
    if (bspgemm_status st = check_operand(ctx, A, who, flags)) return st;
    if (A->nnz <= INT_MAX) return BSPGEMM_OK;
    char what[128];
    snprintf(what, sizeof what, "%s: more than INT_MAX nonzeros", who);
    return FAIL(BSPGEMM_ERR_OVERFLOW, what);
}
// the optional transposed operand of an entry point that takes A (square: checked already) and AT, tested in this order:
// it belongs to ctx, an int32 entry count, n x n like A, consistent entries.  AT NULL: nothing to check.
static inline bspgemm_status check_transposed_operand(const bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT,
                                                      const char *who)
{
    if (!AT) return BSPGEMM_OK;
    if (bspgemm_status st = check_graph_operand(ctx, AT, who, 0)) return st;
    const int n = A->rows;
    if (AT->rows != n || AT->cols != n) {
        snprintf(g_err, sizeof g_err, "%s: AT is %d x %d, A is %d x %d", who, AT->rows, AT->cols, n, n);
        return BSPGEMM_ERR_INVALID;
    }
    return check_operand(ctx, AT, who, NEED_ENTRIES_CONSISTENT);
}
// The canonical check (kernels.hpp) of every distinct handle into *d_word, two bits per operand (kSetErrRange,
// kSetErrOrder): A at shift 0, an AT that is not A at shift 2.  The workspace and ctx->tile_row are there; no synchronisation.
static inline void launch_graph_canonical_checks(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT,
                                                 unsigned *d_word, hipStream_t s)
{
    const int n = A->rows;
    bsp::launch_canonical_check(A->d_row_ptr, A->d_col_idx, n, n, A->nnz, 0, ctx->tile_row, d_word, s);
    if (AT && AT != A) bsp::launch_canonical_check(AT->d_row_ptr, AT->d_col_idx, n, n, AT->nnz, 2, ctx->tile_row, d_word, s);
}
// the failure where that word holds a range bit: canon_bits & (kSetErrRange | kSetErrRange << 2)
static inline bspgemm_status fail_bad_column_in(const char *who, int n, unsigned canon_bits)
{
    snprintf(g_err, sizeof g_err, "%s: a column index outside [0, %d) in operand %s", who, n,
             (canon_bits & bsp::kSetErrRange) ? "A" : "AT");
    return BSPGEMM_ERR_INVALID;
}
// f(std::integral_constant<int, W>{}) for the lanes per vertex W = 4 or 16; any other W runs the 64-lane instance
template <class F>
static inline void dispatch_lanes(int W, F &&f)
{
    if (W == 4) f(std::integral_constant<int, 4>{});
    else if (W == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 64>{});
}
// the assignment operand of n vertices, laid out like an uploaded one: row v holds one entry, and its col_idx is the label
// array while the rounds run, so nothing is copied at the end (operand_finish(m, n) completes it).  After a failure *m is
// NULL or a handle that bspgemm_matrix_free takes.
static inline bspgemm_status assignment_operand(bspgemm_context *ctx, int n, bspgemm_matrix **m)
{
    if (bspgemm_status st = operand_new(ctx, n, n, m)) return st;
    return operand_cols(*m, n);
}
// the grid of a pass with one thread per vertex and one more (row_ptr has n + 1 words)
static inline dim3 vertex_grid(int n, int threads) { return dim3((unsigned)(((long long)n + 1 + threads - 1) / threads)); }
// the grid of `threads` threads in workgroups of `block`: one workgroup at least, so that thread 0's resets happen
static inline dim3 grid_for(long long threads, int block) { return dim3((unsigned)std::max(1ll, (threads + block - 1) / block)); }
// The lanes per vertex (4, 16 or 64) of a launch whose `rows` rows hold `entries` entries: the smallest W at or above the
// mean row length / per_lane.  per_lane 1 where a long row is a serial tail of its group, 4 where chunk records bound what a
// group walks; the measurement behind each choice stands at its call.
static inline int lanes_for_mean(long long entries, long long rows, int per_lane)
{
    if (entries <= 4ll * per_lane * rows) return 4;
    return entries <= 16ll * per_lane * rows ? 16 : 64;
}
// what a read-back may say of the list that is read next, head = {entries, chunk records}: lo <= entries <= hi, and no
// more records than the chunk array holds.  Anything else: fail_stuck.
static inline bool frontier_head_ok(int2 head, int lo, int hi, size_t chunk_cap)
{
    return head.x >= lo && head.x <= hi && head.y >= 0 && (size_t)head.y <= chunk_cap;
}
// A repetition: zero the leading `bytes` of the device flag block, launch, read the block back -- its one synchronisation.
static inline hipError_t round_reset(void *d_flags, size_t bytes, hipStream_t s) { return hipMemsetAsync(d_flags, 0, bytes, s); }
static inline hipError_t round_fetch(void *h, const void *d_flags, size_t bytes, hipStream_t s)
{
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = hipMemcpyAsync(h, d_flags, bytes, hipMemcpyDeviceToHost, s)) return e;
    return hipStreamSynchronize(s);
}
static inline bspgemm_status fail_bad_column(const char *who, int n)
{
    snprintf(g_err, sizeof g_err, "%s: a column index outside [0, %d) (A.cols)", who, n);
    return BSPGEMM_ERR_INVALID;
}
static inline bspgemm_status fail_stuck(const char *who)
{
    snprintf(g_err, sizeof g_err, "%s: did not converge", who);
    return BSPGEMM_ERR_HIP;
}
// host clocks of the timing modes (BSPGEMM_KCORE_TIMING, BSPGEMM_SCC_TIMING, BSPGEMM_COLOR_TIMING, BSPGEMM_BFS_TREE_TIMING, BSPGEMM_LP_TIMING, BSPGEMM_LCC_TIMING, BSPGEMM_PR_TIMING, BSPGEMM_BC_TIMING, BSPGEMM_EXTRACT_TIMING, BSPGEMM_MATCH_TIMING, BSPGEMM_SSSP_TIMING)
using host_clock = std::chrono::steady_clock;
static inline double ms_since(host_clock::time_point t)
{
    return std::chrono::duration<double, std::milli>(host_clock::now() - t).count();
}
// The stage clock of a timing mode.  A lap runs from start() or the last lap() to this lap(), which adds it to `acc`;
// sync: the timed mode first waits for the stream, so that the lap holds what was launched in it.  Off, start() and lap()
// do nothing: no synchronisation, the call's sequence of HIP calls is the untimed one.  The fprintf stays with the mode.
struct StageClock {
    bool on;
    hipStream_t s;
    host_clock::time_point t0, t;       // the call's start, the current lap's start
    double last = 0, max_ms = 0;        // the lap closed last; the longest that longest() was shown, and its tags
    int max_tag[2] = {0, 0};
    StageClock(bool timed, hipStream_t stream) : on(timed), s(stream), t0(host_clock::now()), t(t0) {}
    void start() { if (on) t = host_clock::now(); }
    hipError_t lap(double &acc, bool sync = false)
    {
        if (!on) return hipSuccess;
        const hipError_t e = sync ? hipStreamSynchronize(s) : hipSuccess;
        const host_clock::time_point now = host_clock::now();
        last = std::chrono::duration<double, std::milli>(now - t).count();
        acc += last;
        t = now;
        return e;
    }
    void longest(double ms, int tag0, int tag1 = 0)
    {
        if (!on || ms <= max_ms) return;
        max_ms = ms;
        max_tag[0] = tag0;
        max_tag[1] = tag1;
    }
    double total() const { return ms_since(t0); }
};
// The opening of an algorithm on the simple undirected graph *S = symmetrize(A, DROP_DIAGONAL) (color.hip, match.hip, lp.hip):
// the workspace grows ONCE, to what the symmetrize takes at most over its stages or, where ask_own, to the call's own
// own_ints if that is more; then the symmetrize, and the lap into ms_sym.  Only for a call whose sequence of HIP calls and
// allocations is exactly this: kcore.hip and lcc.hip order theirs differently.
static inline bspgemm_status symmetrized_operand(bspgemm_context *ctx, const bspgemm_matrix *A, size_t own_ints, bool ask_own,
                                                 StageClock &clk, double &ms_sym, bspgemm_matrix **S)
{
    if (bspgemm_status st = ensure_tmp(ctx, std::max(symmetrize_workspace_ints(A->nnz, A->rows), ask_own ? own_ints : 0))) return st;
    if (bspgemm_status st = bspgemm_matrix_symmetrize(ctx, A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL, S)) return st;
    (void)clk.lap(ms_sym, true);
    return BSPGEMM_OK;
}

// ------------------------------------------------------------------ drop-in host steps (dropin.hip) ---
// one line on stderr for a failed drop-in ("SpGEMM_hip: <status>: <last error>"), returns the status as int
int dropin_fail(const char *fn, bspgemm_status st);
// B's row count is implicit in the reference (never passed): 1 + the largest column that A's rows [r0, r1) use
static inline int dropin_b_rows(const int *Acol, const int *Arow, int r0, int r1)
{
    return bspgemm_par_max_plus_one(Acol + Arow[r0], (long long)Arow[r1] - Arow[r0]);
}
// A's rows [r0, r1) and B (brows x Bm) onto the device; view_ok: B = A through the same host arrays becomes a view of A's
// device copy.  On failure the caller frees whatever *A and *B hold.
bspgemm_status dropin_upload(bspgemm_context *ctx, const int *Acol, const int *Arow, int r0, int r1, const int *Bcol,
                             const int *Brow, int brows, int Bm, bool view_ok, bspgemm_matrix **A, bspgemm_matrix **B);
// the int64 row_ptr of a result that fits the int32 interface (nnz <= INT_MAX was checked) into the caller's Crow
static inline void dropin_crow(const int64_t *rp64, int rows, int *Crow)
{
    for (int i = 0; i <= rows; i++) Crow[i] = (int)rp64[i];
}
