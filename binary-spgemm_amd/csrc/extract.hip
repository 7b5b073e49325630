// extract.hip -- submatrix extraction out = A[I, J] and induced subgraphs, on the device: bspgemm_matrix_extract and
// bspgemm_matrix_extract_rows_of (include/bspgemm.h, which holds the definition).  No product: a filtered
// copy that reads every selected row of A once, keeps the entries whose column is selected and writes the new column number.
//
// An OUT ROW r reads one row of A, src(r): I[r] (or r) when relabelling; r itself under KEEP_SHAPE, where a row that I does
// not name stays empty.  A bitmap cbits[A.cols / 32] says which columns are selected -- what the count and, per entry, the emit
// gather: A.cols / 8 bytes stay in an L2 -- and when relabelling the map cmap[A.cols] holds a selected column's position in J,
// which only a kept entry gathers (under KEEP_SHAPE the column itself is written and there is no map).  J NULL: neither,
// every column is kept as itself.  The state lies in the context's workspace, grown once before anything is launched:
//     ExCounters        the read-backs            cbits, cmap[A.cols], rflag[A.rows] (KEEP_SHAPE with a row list)
//     the lists         (host lists only; the lists of _rows_of are read where their operand stores them)
//     cnt[R], pre[R + 1], part[]   the kept entries per out row, their int64 scan, the scan's partials
//     big[R]            the out rows that a workgroup sorts
// and the chunk records, whose number only read-back one tells, in the values workspace (so the maps do not move):
//     chunk[k] {out row, chunk number}, sub[4 k]: the kept entries of every quarter of a chunk, then their offsets in the row
//
//     k_ex_maps         one lane per list entry: the column's bit, cmap by atomicCAS (the loser raises the duplicate bit), J[c] < J[c - 1]
//                       raises the unsorted bit, an index out of range its list's range bit; per row of I its length goes to
//                       `scanned` and, for a row longer than kExHubChunk, its chunks to `chunks` (under KEEP_SHAPE once per
//                       distinct row: the lane that wins rflag[i]).  The canonical check of A rides in the same read-back.
//     k_ex_hub_records  one lane per out row: a hub takes its records from the cursor (hub_chunks.hpp)
//     k_ex_count<W>     W lanes per out row stride over the row of A and count the kept entries; hubs are skipped
//     k_ex_count_chunk  one workgroup per record, one wave per quarter of the chunk: its count to sub[]
//     k_ex_hub_finish   one lane per hub (the record of chunk 0): sub[] becomes offsets, the sum is the row's count
//     scan              launch_scan_counts, then k_ex_rows: the int32 row_ptr of out, the rows for the workgroup sort, the
//                       largest count above the workgroup cap.  Read-back two: the kept total and those two.
//     k_ex_emit<W>, k_ex_emit_chunk   the same walks; per step a ballot of the keep flags and the rank by the popcount of the
//                       group's lower lanes, so the order inside a row is A's
//     k_ex_sort_wave, k_ex_sort_block   only where J is not ascending: a bitonic network over the out row in LDS, a wave for
//                       rows of up to kExSortWave entries, a workgroup for rows of up to kExSortBlock.  A longer row sends
//                       out through operand_canonical once.
// A is canonical when the walks run (an untidy A is canonicalised first, like setop's operands), so its columns are inside
// [0, A.cols) -- every index into cmap is -- and its rows are duplicate-free; J names no column twice, so the out rows are
// duplicate-free and the sort finishes them.  No kernel waits for another workgroup; every loop is bounded by a row, a
// chunk or a count that the host passed in.  Synchronisations: two with host lists (the error bits, `scanned` and the chunk
// count; the kept total), one more in _rows_of for the lists' lengths.
#include "internal.hpp"
#include "hub_chunks.hpp"
#include "wave.hpp"

#include <algorithm>
#include <vector>

namespace bsp {

constexpr int kExThreads = 256;
constexpr int kExWaves = kExThreads / 64;
constexpr int kExSub = kExHubChunk / kExWaves;       // a wave's quarter of a chunk
constexpr unsigned kExErrRangeI = 1u;                // an entry of the row list outside [0, A.rows)
constexpr unsigned kExErrRangeJ = 2u;                // an entry of the column list outside [0, A.cols)
constexpr unsigned kExErrDup = 4u;                   // a column named twice (relabelling)
constexpr unsigned kExErrUnsorted = 8u;              // J[c] < J[c - 1] somewhere

struct ExCounters {
    u64 scanned;                        // the entries of the rows that are walked
    u64 chunks;                         // the chunk records they need
    unsigned err;                       // kExErr*
    unsigned canon;                     // the canonical check of A (kSetErrRange, kSetErrOrder)
    int cursor;                         // the records taken
    int big;                            // entries of big[]
    int kmax;                           // the largest count of an out row above kExSortBlock, else 0
    int walked;                         // the rows that are read (under KEEP_SHAPE the distinct rows of the list)
    int pad[2];
};

struct ExMaps {
    int rowsA, colsA;
    const int *rpA;
    const int *I, *J;                   // read only where has_i / has_j
    int ni, nj;
    int has_i, has_j, keep;
    int *cmap, *rflag;
    unsigned *cbits;
    ExCounters *cnt;
};

// what the walks get.  R out rows; list: I when relabelling with a row list (else NULL); rflag: KEEP_SHAPE with a row list
// (else NULL); cbits: bit c = column c is selected, NULL: every column is kept as itself; cmap: what is written for a
// selected column, NULL: the column itself
struct ExWalk {
    int R;
    const int *rpA;
    const int *list;
    const int *rflag;
    const unsigned *cbits;
    const int *cmap;
};

// whether column c is kept: a gather from A.cols / 8 bytes, which an L2 holds where the map's 4 bytes per column do not
__device__ __forceinline__ int ex_kept(const ExWalk &a, int c) { return a.cbits ? (int)((a.cbits[c >> 5] >> (c & 31)) & 1u) : 1; }

// the row of A that out row r reads, or -1 for a row that stays empty
__device__ __forceinline__ int ex_src(const ExWalk &a, int r)
{
    if (a.rflag) return a.rflag[r] ? r : -1;
    return a.list ? a.list[r] : r;
}

__global__ __launch_bounds__(kExThreads) void k_ex_maps(ExMaps a)
{
    const int lane = lane_id();
    const long long t = (long long)blockIdx.x * kExThreads + threadIdx.x;
    unsigned err = 0;
    long long sc = 0, ch = 0;
    int wk = 0;
    if (a.has_j && t < a.nj) {
        const int c = a.J[t];
        if ((unsigned)c >= (unsigned)a.colsA) err |= kExErrRangeJ;            // before c indexes anything
        else {
            atomicOr(&a.cbits[c >> 5], 1u << (c & 31));
            if (!a.keep && atomicCAS(&a.cmap[c], -1, (int)t) != -1) err |= kExErrDup;
        }
        if (t > 0 && c < a.J[t - 1]) err |= kExErrUnsorted;
    }
    if (t < (a.has_i ? a.ni : a.rowsA)) {
        const int i = a.has_i ? a.I[t] : (int)t;
        if ((unsigned)i >= (unsigned)a.rowsA) {
            err |= kExErrRangeI;
        } else if (!a.rflag || atomicCAS(&a.rflag[i], 0, 1) == 0) {           // (KEEP_SHAPE: a row counts once)
            const int len = a.rpA[i + 1] - a.rpA[i];
            sc = len;
            wk = 1;
            ch = hub_chunks_over<kExHubChunk>(len);
        }
    }
    sc = wave_sum(sc);
    ch = wave_sum(ch);
    wk = wave_sum(wk);
    unsigned bits = 0;
#pragma unroll
    for (unsigned b = 1; b <= kExErrUnsorted; b <<= 1) bits |= __ballot(err & b) ? b : 0u;
    if (lane == 0) {
        if (sc) atomicAdd(&a.cnt->scanned, (u64)sc);
        if (ch) atomicAdd(&a.cnt->chunks, (u64)ch);
        if (wk) atomicAdd(&a.cnt->walked, wk);
        if (bits) atomicOr(&a.cnt->err, bits);
    }
}

__global__ __launch_bounds__(kExThreads) void k_ex_hub_records(ExWalk a, int2 *__restrict__ chunk, int chunk_cap, ExCounters *cnt)
{
    const long long r = (long long)blockIdx.x * kExThreads + threadIdx.x;
    if (r >= a.R) return;
    const int i = ex_src(a, (int)r);
    if (i < 0) return;
    const int k = hub_chunks_over<kExHubChunk>(a.rpA[i + 1] - a.rpA[i]);
    if (k) hub_chunks_emit((int)r, k, &cnt->cursor, chunk, chunk_cap);
}

// the group's row: entries [pos, e) in steps of W, nothing for a hub (mine false) and for a row that stays empty.  Not
// GroupRow of hub_chunks.hpp: the vertex comes through ex_src, which may name no row at all, and such a group is still `mine`
template <int W>
__device__ __forceinline__ bool ex_group_row(const ExWalk &a, long long f, int sub, long long &pos, long long &e)
{
    pos = e = 0;
    if (f >= a.R) return false;
    const int i = ex_src(a, (int)f);
    if (i < 0) return true;
    const long long b = a.rpA[i];
    e = a.rpA[i + 1];
    if (e - b > kExHubChunk) {                                                // (the chunks' row)
        e = 0;
        return false;
    }
    pos = b + sub;
    return true;
}

template <int W>
__global__ __launch_bounds__(kExThreads) void k_ex_count(ExWalk a, const int *__restrict__ colA, int *__restrict__ cnt)
{
    const long long t = (long long)blockIdx.x * kExThreads + threadIdx.x;
    const long long f = t / W;
    const int sub = (int)(t % W);
    long long pos, e;
    const bool mine = ex_group_row<W>(a, f, sub, pos, e);
    int k = 0;
#pragma unroll 4
    for (; pos < e; pos += W) k += ex_kept(a, colA[pos]);
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) k += __shfl_xor(k, off, 64);
    if (mine && sub == 0) cnt[f] = k;
}

// the quarter of chunk record `rec` that wave w walks
__device__ __forceinline__ void ex_sub_range(const ExWalk &a, int2 rec, int w, long long &b, long long &e)
{
    long long b0, e0;
    hub_chunk_range<kExHubChunk>(a.rpA, make_int2(ex_src(a, rec.x), rec.y), b0, e0);
    b = b0 + (long long)w * kExSub;
    e = min(e0, b + kExSub);
}

__global__ __launch_bounds__(kExThreads) void k_ex_count_chunk(ExWalk a, const int2 *__restrict__ chunk,
                                                              const int *__restrict__ colA, int *__restrict__ sub)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    long long b, e;
    ex_sub_range(a, chunk[blockIdx.x], w, b, e);
    int k = 0;
    for (long long pos = b + lane; pos < e; pos += 64) k += ex_kept(a, colA[pos]);
    k = wave_sum(k);
    if (lane == 0) sub[(size_t)blockIdx.x * kExWaves + w] = k;
}

// a hub's records lie side by side (one atomicAdd took them), the record of chunk 0 first
__global__ __launch_bounds__(kExThreads) void k_ex_hub_finish(ExWalk a, int nchunks, const int2 *__restrict__ chunk,
                                                             int *__restrict__ sub, int *__restrict__ cnt)
{
    const long long t = (long long)blockIdx.x * kExThreads + threadIdx.x;
    if (t >= nchunks) return;
    const int2 rec = chunk[t];
    if (rec.y != 0) return;
    const int i = ex_src(a, rec.x);
    const long long k = hub_chunks_over<kExHubChunk>(a.rpA[i + 1] - a.rpA[i]);
    const long long last = min((t + k) * kExWaves, (long long)nchunks * kExWaves);
    int run = 0;
    for (long long q = t * kExWaves; q < last; q++) {
        const int v = sub[q];
        sub[q] = run;
        run += v;
    }
    cnt[rec.x] = run;
}

// out's row_ptr from the scan; want_sort: the rows that a workgroup sorts behind big[], and the largest count that no
// workgroup takes.  Whole waves.
__global__ __launch_bounds__(kExThreads) void k_ex_rows(int R, const long long *__restrict__ pre, const int *__restrict__ cnt,
                                                       int want_sort, int *__restrict__ row_ptr, int *big, ExCounters *c)
{
    const int lane = lane_id();
    const long long r = (long long)blockIdx.x * kExThreads + threadIdx.x;
    if (r <= R) row_ptr[r] = (int)pre[r];
    if (!want_sort) return;                                                   // (uniform)
    const int k = r < R ? cnt[r] : 0;
    wave_append(k > kExSortWave && k <= kExSortBlock, (int)r, big, &c->big, R, lane);   // (a row is appended once)
    const int m = wave_max(k);
    if (lane == 0 && m > kExSortBlock) atomicMax(&c->kmax, m);
}

// one step of an emit: the wave's lanes with `live` hold entry column c of their group's row; at: where the group's next
// kept entry goes; gm: the lanes of the group.  Whole wave.
__device__ __forceinline__ void ex_emit_step(const ExWalk &a, bool live, int c, u64 gm, long long &at, int *__restrict__ out, int lane)
{
    int v = -1;
    if (live && ex_kept(a, c)) v = a.cmap ? a.cmap[c] : c;                     // (only a kept entry gathers the map)
    const bool keep = live && v >= 0;
    const u64 m = __ballot(keep) & gm;
    if (keep) out[at + __popcll(m & mask_lt(lane))] = v;
    at += __popcll(m);
}

template <int W>
__global__ __launch_bounds__(kExThreads) void k_ex_emit(ExWalk a, const int *__restrict__ colA, const long long *__restrict__ pre,
                                                       int *__restrict__ out)
{
    const int lane = lane_id();
    const long long t = (long long)blockIdx.x * kExThreads + threadIdx.x;
    const long long f = t / W;
    const int sub = (int)(t % W);
    long long pos, e;
    ex_group_row<W>(a, f, sub, pos, e);
    long long at = f < a.R ? pre[f] : 0;
    const u64 gm = W == 64 ? ~0ull : ((1ull << (W & 63)) - 1ull) << (lane - sub);
    // the groups of a wave have different trip counts: the loop runs to the wave's longest, the ballot needs every lane
    while (__ballot(pos < e) != 0) {                                          // (wave-uniform)
        const bool live = pos < e;
        ex_emit_step(a, live, live ? colA[pos] : 0, gm, at, out, lane);
        pos += W;
    }
}

__global__ __launch_bounds__(kExThreads) void k_ex_emit_chunk(ExWalk a, const int2 *__restrict__ chunk, const int *__restrict__ sub,
                                                             const int *__restrict__ colA, const long long *__restrict__ pre,
                                                             int *__restrict__ out)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int2 rec = chunk[blockIdx.x];
    long long b, e;
    ex_sub_range(a, rec, w, b, e);
    long long at = pre[rec.x] + sub[(size_t)blockIdx.x * kExWaves + w];
    for (long long pos = b + lane; __ballot(pos < e) != 0; pos += 64) {       // (wave-uniform)
        const bool live = pos < e;
        ex_emit_step(a, live, live ? colA[pos] : 0, ~0ull, at, out, lane);
    }
}

// ascending bitonic network over s[0 .. n2), n2 a power of two, by `threads` lanes of which this is `tid`.  BLOCK: the lanes
// are a workgroup (a barrier between the stages), else one wave (its LDS operations execute in issue order)
template <bool BLOCK>
__device__ __forceinline__ void ex_bitonic(int *s, int n2, int tid, int threads)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n2 / 2; t += threads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const int x = s[i], y = s[l];
                if ((x > y) == up) {
                    s[i] = y;
                    s[l] = x;
                }
            }
            if (BLOCK) __syncthreads();
            else wave_lds_fence();
        }
}

template <bool BLOCK>
__device__ __forceinline__ void ex_sort_row(int *s, int *__restrict__ row, int k, int tid, int threads)
{
    int n2 = 2;
    while (n2 < k) n2 <<= 1;
    for (int t = tid; t < n2; t += threads) s[t] = t < k ? row[t] : INT_MAX;
    if (BLOCK) __syncthreads();
    else wave_lds_fence();
    ex_bitonic<BLOCK>(s, n2, tid, threads);
    for (int t = tid; t < k; t += threads) row[t] = s[t];
}

// one wave per out row of 2 .. kExSortWave entries
__global__ __launch_bounds__(kExThreads) void k_ex_sort_wave(int R, const int *__restrict__ row_ptr, int *__restrict__ out)
{
    __shared__ int seg[kExWaves][kExSortWave];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * kExWaves + w;
    if (r >= R) return;                                                       // (wave-uniform; no barrier in this kernel)
    const int b = row_ptr[r], k = row_ptr[r + 1] - b;
    if (k < 2 || k > kExSortWave) return;
    ex_sort_row<false>(seg[w], out + b, k, lane, 64);
}

// one workgroup per row of big[]: kExSortWave < entries <= kExSortBlock
__global__ __launch_bounds__(kExThreads) void k_ex_sort_block(const int *__restrict__ big, const int *__restrict__ row_ptr,
                                                             int *__restrict__ out)
{
    __shared__ int s[kExSortBlock];
    const int r = big[blockIdx.x];
    const int b = row_ptr[r], k = row_ptr[r + 1] - b;
    if (k < 2 || k > kExSortBlock) return;                                    // (uniform; defensive)
    ex_sort_row<true>(s, out + b, k, threadIdx.x, kExThreads);
}

}  // namespace bsp

using namespace bsp;

// a row or column list: `all` (every index in order), else n entries on the host or on the device.  name: what the
// messages call it.
struct ExList {
    const int *host, *dev;
    int n;
    bool all;
    const char *name;
};

// The arguments are checked by the callers.  canonical: A is known to have strictly ascending rows (the second round).
static bspgemm_status extract_run(bspgemm_context *ctx, const bspgemm_matrix *A, const ExList &LI, const ExList &LJ, unsigned flags,
                                  bspgemm_matrix **out, bspgemm_extract_info *info, const char *who, bool canonical)
{
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    StageClock clk(ctx->extract_timing, s);
    double ms_maps = 0, ms_back = 0, ms_count = 0, ms_hub = 0, ms_scan = 0, ms_emit = 0, ms_sort = 0;
    const bool keep = (flags & BSPGEMM_EXTRACT_KEEP_SHAPE) != 0;
    const int rowsA = A->rows, colsA = A->cols;
    const long long E = A->nnz;
    const int R = keep || LI.all ? rowsA : LI.n, out_cols = keep || LJ.all ? colsA : LJ.n;
    const int nwalk = LI.all ? rowsA : LI.n, nj = LJ.all ? 0 : LJ.n;
    const int forced_w = ctx->extract_lanes;

    // the workspace, every array on a 16-byte boundary; it grows ONCE, before anything is launched
    ExCounters *d_cnt = nullptr;
    int *cmap = nullptr, *rflag = nullptr, *li = nullptr, *lj = nullptr, *cnt = nullptr, *big = nullptr;
    unsigned *cbits = nullptr;
    long long *pre = nullptr, *part = nullptr;
    auto carve = [&](int *tmp) {
        return WsCursor(tmp).take(d_cnt, 1).take_if(!(LJ.all || keep), cmap, (size_t)colsA).take_if(!LJ.all, cbits, ((size_t)colsA + 31) / 32)
            .take_if(keep && !LI.all, rflag, (size_t)rowsA).take_if(LI.host, li, (size_t)LI.n).take_if(LJ.host, lj, (size_t)LJ.n)
            .take(cnt, (size_t)R).take(pre, (size_t)R + 1).take(part, (size_t)R / 2048 + 4).take(big, ws_pad4((size_t)R)).ints();
    };
    // (to what the canonicalisation of A takes, two transposes, if that is more: an untidy A then grows nothing again)
    const size_t ws_ints = std::max(carve(nullptr), canonical ? (size_t)0 : std::max(transpose_workspace_ints(E, colsA), transpose_workspace_ints(E, rowsA)));
    if (bspgemm_status st = ensure_tmp(ctx, ws_ints)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return st;
    carve(ctx->tmp);
    const int *dI = LI.host ? li : LI.dev, *dJ = LJ.host ? lj : LJ.dev;

    bspgemm_matrix *m = nullptr;
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_matrix_free(m);
        if (info) memset(info, 0, sizeof *info);
        return st;
    };
    auto stage = [&](double &acc) { return clk.lap(acc, true); };             // BSPGEMM_EXTRACT_TIMING: a stage ends
    if (bspgemm_status st = operand_new(ctx, R, out_cols, &m)) return bail(st);

    // ---- the maps, the lists' checks, `scanned` and the chunk count; with them the canonical check of A
    HIPCHK_B(hipMemsetAsync(d_cnt, 0, sizeof(ExCounters), s));
    if (cmap && colsA > 0) HIPCHK_B(hipMemsetAsync(cmap, 0xFF, (size_t)colsA * sizeof(int), s));
    if (cbits && colsA > 0) HIPCHK_B(hipMemsetAsync(cbits, 0, (((size_t)colsA + 31) / 32) * sizeof(unsigned), s));
    if (rflag && rowsA > 0) HIPCHK_B(hipMemsetAsync(rflag, 0, (size_t)rowsA * sizeof(int), s));
    if (LI.host && LI.n > 0) HIPCHK_B(hipMemcpyAsync(li, LI.host, (size_t)LI.n * sizeof(int), hipMemcpyHostToDevice, s));
    if (LJ.host && LJ.n > 0) HIPCHK_B(hipMemcpyAsync(lj, LJ.host, (size_t)LJ.n * sizeof(int), hipMemcpyHostToDevice, s));
    if (std::max(nwalk, nj) > 0) {
        const ExMaps a = {rowsA, colsA, A->d_row_ptr, dI, dJ, LI.all ? 0 : LI.n, nj, !LI.all, !LJ.all, keep, cmap, rflag, cbits, d_cnt};
        hipLaunchKernelGGL(k_ex_maps, grid_for(std::max(nwalk, nj), kExThreads), dim3(kExThreads), 0, s, a);
    }
    if (!canonical) launch_canonical_check(A->d_row_ptr, A->d_col_idx, rowsA, colsA, E, 0, ctx->tile_row, &d_cnt->canon, s);
    ExCounters h = {};
    HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));                            // read-back one
    (void)clk.lap(ms_maps);
    if (h.canon & kSetErrRange) {
        snprintf(g_err, sizeof g_err, "%s: a column index outside [0, %d) in operand A", who, colsA);
        return bail(BSPGEMM_ERR_INVALID);
    }
    if (h.err & kExErrRangeI) {
        snprintf(g_err, sizeof g_err, "%s: an entry of the row list %s outside [0, %d) (A.rows)", who, LI.name, rowsA);
        return bail(BSPGEMM_ERR_INVALID);
    }
    if (h.err & kExErrRangeJ) {
        snprintf(g_err, sizeof g_err, "%s: an entry of the column list %s outside [0, %d) (A.cols)", who, LJ.name, colsA);
        return bail(BSPGEMM_ERR_INVALID);
    }
    if (h.err & kExErrDup) {
        snprintf(g_err, sizeof g_err, "%s: a column named twice in the column list %s (relabelling takes each column once)", who, LJ.name);
        return bail(BSPGEMM_ERR_INVALID);
    }
    if (h.canon & kSetErrOrder) {
        if (canonical) return bail(FAIL(BSPGEMM_ERR_HIP, "extract: a transposed operand is not in ascending order"));
        // what the maps left is discarded: A is transposed twice (in this workspace) and the call starts again
        bspgemm_matrix_free(m);
        m = nullptr;
        bspgemm_matrix *ca = nullptr;
        bspgemm_status st = operand_canonical(ctx, A, &ca);
        if (!st) st = extract_run(ctx, ca, LI, LJ, flags, out, info, who, true);
        bspgemm_matrix_free(ca);
        if (st) return bail(st);
        if (info) info->canonicalised = 1;
        return BSPGEMM_OK;
    }
    const long long scanned = (long long)h.scanned;
    if (scanned < 0 || h.chunks > (u64)(INT_MAX / (2 * kExWaves))) {
        snprintf(g_err, sizeof g_err, "%s: the row list reads %lld entries in %llu hub chunks: too many for one call", who, scanned,
                 (unsigned long long)h.chunks);
        return bail(BSPGEMM_ERR_OVERFLOW);
    }
    const int chunks = (int)h.chunks;
    const bool monotone = keep || LJ.all || !(h.err & kExErrUnsorted);
    // The lanes per out row: a QUARTER of the mean length of the rows that are read, betweenness.hip's rule (no group walks
    // more than kExHubChunk entries, so the mean, not the tail, sets the cost).  The mean is over the rows READ: under
    // KEEP_SHAPE the out rows that the list does not name cost a group that finds nothing, and dividing by all of them chose 4
    // lanes for the 4048 core vertices of a Graph500-skew 18 (0.650 ms, against 0.351 ms under 64).
    const int W = forced_w ? forced_w : lanes_for_mean(scanned, h.walked, 4);
    const ExWalk walk = {R, A->d_row_ptr, keep || LI.all ? nullptr : dI, rflag, cbits, cmap};
    const dim3 block(kExThreads);

    long long kept = 0;
    int sorted_by = 0;
    int2 *chunk = nullptr;
    int *sub = nullptr;
    if (scanned == 0 || R == 0) {
        HIPCHK_B(hipMemsetAsync(m->d_row_ptr, 0, ((size_t)R + 1) * sizeof(int), s));
        if (bspgemm_status st = operand_cols(m, 0)) return bail(st);
    } else {
        if (chunks) {
            if (bspgemm_status st = ensure_tmpv(ctx, (size_t)chunks * (2 + kExWaves))) return bail(st);
            chunk = reinterpret_cast<int2 *>(ctx->tmpv);
            sub = ctx->tmpv + 2 * (size_t)chunks;
            hipLaunchKernelGGL(k_ex_hub_records, grid_for(R, kExThreads), block, 0, s, walk, chunk, chunks, d_cnt);
        }
        // ---- count
        dispatch_lanes(W, [&](auto w) {
            hipLaunchKernelGGL(k_ex_count<decltype(w)::value>, grid_for((long long)R * W, kExThreads), block, 0, s, walk, A->d_col_idx, cnt);
        });
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(stage(ms_count));
        if (chunks) {
            hipLaunchKernelGGL(k_ex_count_chunk, dim3((unsigned)chunks), block, 0, s, walk, chunk, A->d_col_idx, sub);
            hipLaunchKernelGGL(k_ex_hub_finish, grid_for(chunks, kExThreads), block, 0, s, walk, chunks, chunk, sub, cnt);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(stage(ms_hub));
        }
        // ---- scan, out's row_ptr, read-back two
        launch_scan_counts(cnt, R, pre, part, nullptr, s);
        hipLaunchKernelGGL(k_ex_rows, grid_for((long long)R + 1, kExThreads), block, 0, s, R, pre, cnt, monotone ? 0 : 1, m->d_row_ptr, big, d_cnt);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(stage(ms_scan));
        HIPCHK_B(hipMemcpyAsync(&kept, pre + R, sizeof kept, hipMemcpyDeviceToHost, s));
        HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));                        // read-back two
        (void)clk.lap(ms_back);
        if (kept < 0 || kept > scanned || h.big < 0 || h.big > R || h.cursor != chunks)
            return bail(FAIL(BSPGEMM_ERR_HIP, "extract: inconsistent counts"));
        if (kept > INT_MAX) {
            snprintf(g_err, sizeof g_err, "%s: %lld entries in the result: more than INT_MAX, not usable as an int32 operand", who, kept);
            return bail(BSPGEMM_ERR_OVERFLOW);
        }
        if (bspgemm_status st = operand_cols(m, kept)) return bail(st);
        // ---- emit
        if (kept > 0) {
            dispatch_lanes(W, [&](auto w) {
                hipLaunchKernelGGL(k_ex_emit<decltype(w)::value>, grid_for((long long)R * W, kExThreads), block, 0, s, walk, A->d_col_idx, pre,
                                   m->d_col_idx);
            });
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(stage(ms_emit));
            if (chunks) {
                hipLaunchKernelGGL(k_ex_emit_chunk, dim3((unsigned)chunks), block, 0, s, walk, chunk, sub, A->d_col_idx, pre, m->d_col_idx);
                HIPCHK_B(hipGetLastError());
                HIPCHK_B(stage(ms_hub));
            }
        }
        // ---- sort
        if (!monotone && kept > 0) {
            sorted_by = h.kmax > kExSortBlock ? 2 : 1;
            if (sorted_by == 1) {
                hipLaunchKernelGGL(k_ex_sort_wave, dim3((unsigned)(((long long)R + kExWaves - 1) / kExWaves)), block, 0, s, R,
                                   m->d_row_ptr, m->d_col_idx);
                if (h.big > 0)
                    hipLaunchKernelGGL(k_ex_sort_block, dim3((unsigned)h.big), block, 0, s, big, m->d_row_ptr, m->d_col_idx);
                HIPCHK_B(hipGetLastError());
            }
        }
    }
    if (bspgemm_status st = operand_finish(m, kept)) return bail(st);
    if (sorted_by == 2) {                                                     // a row beyond the workgroup sort: two transposes
        bspgemm_matrix *sorted = nullptr;
        if (bspgemm_status st = operand_canonical(ctx, m, &sorted)) return bail(st);
        bspgemm_matrix_free(m);
        m = sorted;
    }
    HIPCHK_B(stage(ms_sort));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: A %d x %d nnz %lld -> %d x %d kept %lld scanned %lld hub chunks %d (%d lanes) monotone %d sorted by %d "
                        "| total %.3f ms = maps and checks %.3f + count %.3f + hub launches %.3f + scan %.3f + read-back two %.3f + "
                        "emit %.3f + sort %.3f + rest\n",
                who, rowsA, colsA, E, R, out_cols, kept, scanned, chunks, W, monotone ? 1 : 0, sorted_by, clk.total(), ms_maps,
                ms_count, ms_hub, ms_scan, ms_back, ms_emit, ms_sort);
    if (info) {
        info->kept = kept;
        info->scanned = scanned;
        info->hub_chunks = chunks;
        info->lanes = W;
        info->cols_monotone = monotone ? 1 : 0;
        info->sorted_by = sorted_by;
        info->canonicalised = 0;
    }
    *out = m;
    return BSPGEMM_OK;
}

// what both entry points ask first; who: the entry point's name
static bspgemm_status extract_arguments(const bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_matrix **out, unsigned flags,
                                        const char *who)
{
    char what[160];
    if (!ctx || !A || !out) {
        snprintf(what, sizeof what, "%s: NULL argument (ctx, A or out)", who);
        return FAIL(BSPGEMM_ERR_INVALID, what);
    }
    if (flags & ~BSPGEMM_EXTRACT_KEEP_SHAPE) {
        snprintf(what, sizeof what, "%s: unknown flag", who);
        return FAIL(BSPGEMM_ERR_INVALID, what);
    }
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_matrix_extract(bspgemm_context *ctx, const bspgemm_matrix *A, int ni, const int *I, int nj,
                                                 const int *J, unsigned flags, bspgemm_matrix **out, bspgemm_extract_info *info)
{
    static const char who[] = "bspgemm_matrix_extract";
    if (out) *out = nullptr;
    if (info) memset(info, 0, sizeof *info);
    // everything below is refused before an operand or a list is dereferenced, and before anything is launched
    if (bspgemm_status st = extract_arguments(ctx, A, out, flags, who)) return st;
    if (I && ni < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_extract: ni < 0");
    if (J && nj < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_extract: nj < 0");
    if (bspgemm_status st = check_graph_operand(ctx, A, who, 0)) return st;
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    // (branch-free first, so that the common case is a vector loop; the offender is looked for only when there is one)
    unsigned bad_i = 0, bad_j = 0, not_ascending = 0;
    for (int r = 0; I && r < ni; r++) bad_i |= (unsigned)((unsigned)I[r] >= (unsigned)A->rows);
    for (int c = 0; J && c < nj; c++) bad_j |= (unsigned)((unsigned)J[c] >= (unsigned)A->cols);
    for (int c = 1; J && c < nj; c++) not_ascending |= (unsigned)(J[c] <= J[c - 1]);
    for (int r = 0; bad_i && r < ni; r++)
        if ((unsigned)I[r] >= (unsigned)A->rows) {
            snprintf(g_err, sizeof g_err, "%s: row %d (I[%d]) of the row list I outside [0, %d) (A.rows)", who, I[r], r, A->rows);
            return BSPGEMM_ERR_INVALID;
        }
    for (int c = 0; bad_j && c < nj; c++)
        if ((unsigned)J[c] >= (unsigned)A->cols) {
            snprintf(g_err, sizeof g_err, "%s: column %d (J[%d]) of the column list J outside [0, %d) (A.cols)", who, J[c], c, A->cols);
            return BSPGEMM_ERR_INVALID;
        }
    if (J && !(flags & BSPGEMM_EXTRACT_KEEP_SHAPE) && not_ascending) {          // (a strictly ascending list has no repeats)
        try {
            std::vector<bool> seen((size_t)A->cols, false);
            for (int c = 0; c < nj; c++) {
                if (seen[(size_t)J[c]]) {
                    snprintf(g_err, sizeof g_err, "%s: column %d (J[%d]) named twice in the column list J (relabelling takes each column once)",
                             who, J[c], c);
                    return BSPGEMM_ERR_INVALID;
                }
                seen[(size_t)J[c]] = true;
            }
        } catch (const std::bad_alloc &) {
            return FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_matrix_extract: host column marks");
        }
    }
    const ExList li = {I, nullptr, I ? ni : 0, I == nullptr, "I"}, lj = {J, nullptr, J ? nj : 0, J == nullptr, "J"};
    return extract_run(ctx, A, li, lj, flags, out, info, who, false);
}

extern "C" bspgemm_status bspgemm_matrix_extract_rows_of(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *MI,
                                                         int ri, const bspgemm_matrix *MJ, int rj, unsigned flags,
                                                         bspgemm_matrix **out, bspgemm_extract_info *info)
{
    static const char who[] = "bspgemm_matrix_extract_rows_of";
    if (out) *out = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (bspgemm_status st = extract_arguments(ctx, A, out, flags, who)) return st;
    if (bspgemm_status st = check_graph_operand(ctx, A, who, 0)) return st;
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    const bspgemm_matrix *M[2] = {MI, MJ};
    const int row[2] = {ri, rj};
    static const char *const names[2] = {"MI", "MJ"};
    for (int q = 0; q < 2; q++) {
        if (!M[q]) continue;
        if (bspgemm_status st = check_graph_operand(ctx, M[q], who, 0)) return st;
        if (bspgemm_status st = check_operand(ctx, M[q], who, NEED_ENTRIES_CONSISTENT)) return st;
        if (row[q] < -1 || row[q] >= M[q]->rows) {
            snprintf(g_err, sizeof g_err, "%s: row %d of %s (r%c) outside [-1, %d)", who, row[q], names[q], q ? 'j' : 'i', M[q]->rows);
            return BSPGEMM_ERR_INVALID;
        }
    }
    // the lists' extents: the one read-back of their lengths (none for a whole col_idx, whose length the handle knows)
    if (bspgemm_status st = use_device(ctx)) return st;
    int ext[2][2] = {{0, 0}, {0, 0}};
    bool fetch = false;
    for (int q = 0; q < 2; q++) {
        if (!M[q]) continue;
        if (row[q] < 0) {
            ext[q][1] = (int)M[q]->nnz;
            continue;
        }
        HIPCHK(hipMemcpyAsync(ext[q], M[q]->d_row_ptr + row[q], 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        fetch = true;
    }
    if (fetch) HIPCHK(hipStreamSynchronize(ctx->stream));
    ExList l[2];
    for (int q = 0; q < 2; q++) {
        l[q] = ExList{nullptr, nullptr, 0, M[q] == nullptr, names[q]};
        if (!M[q]) continue;
        const long long b = ext[q][0], e = ext[q][1];
        if (b < 0 || e < b || e > M[q]->nnz) {
            snprintf(g_err, sizeof g_err, "%s: the row_ptr of %s is not ascending at row %d", who, names[q], row[q]);
            return BSPGEMM_ERR_INVALID;
        }
        l[q].n = (int)(e - b);
        l[q].dev = l[q].n > 0 ? M[q]->d_col_idx + b : nullptr;
    }
    return extract_run(ctx, A, l[0], l[1], flags, out, info, who, false);
}
