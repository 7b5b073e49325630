// lcc.hip -- the local clustering coefficient with a count per vertex, on the device: bspgemm_local_clustering
// (include/bspgemm.h).  The graph is S = bspgemm_matrix_symmetrize(A, DROP_DIAGONAL); num(v) counts the ordered pairs (u, w)
// of distinct neighbours of v with (u, w) in S (undirected: twice the triangles at v) or stored in A (DIRECTED).
//
// Intersecting rows over the whole symmetric S finds every triangle six times (3-5x the cost of the lower
// triangle).  Here every triangle is walked ONCE, on an oriented half T of S (T = select(S, TRIL): row i holds the
// neighbours below i), and all three corners are credited.  Entry p = (i, j) of T and a common element k of T_i and T_j are
// the triangle i > j > k; the intersection yields k's position in both rows, hence the entries (i, k) and (j, k) of T.  With
// w(e) = the number of directions the edge behind entry e is stored in (always 2 when undirected; DIRECTED: 2 when the
// entry is in R = A' and A'^T, else 1), the corner opposite to an edge gets that edge's weight:
//     num[k] += w(i, j)       per hit: summed per workgroup in an LDS cache (lcc_credit below), one device-scope atomicAdd
//                             per cached k and workgroup; a k whose slot is taken, one atomicAdd per hit
//     num[j] += sum w(i, k)   one atomic per entry, only if non-zero
//     num[i] += sum w(j, k)   kept in a register while the lane stays in row i, flushed when it leaves the row (joining the
//                             lanes of a wave that end in one row was measured: no difference, not kept)
// Which half is walked changes no result (TRIU: the same with i < j < k); TRIL is kept, see DESIGN.md 4.20.
//
//   k_lcc_init     the result's pattern (row v holds (v, v)) and num = 0: num IS the result's values array
//   k_lcc_weights  DIRECTED only, entry-parallel over T in select's geometry (sel_rows.hpp): entry (i, j) is searched in
//                  R_i (sel_lower_bound); wgt[p] = 2 if found, else 1, one byte per entry; the found ones are counted
//                  (`reciprocal`, one atomic per wave)
//   k_lcc_count    entry-parallel over T.  j is tested unsigned against n before it indexes row_ptr.  m = min(|T_i|, |T_j|):
//                  0 nothing; LIGHT, m <= BSPGEMM_OPT_DOT_LIGHT: the lane walks the shorter row and searches the longer one
//                  from a lower bound that only advances, crediting as above; HEAVY: the lane remembers the entry and the
//                  wave appends its heavy entries {p, i} to a list (one atomic per wave).  The wave's hits go to the 64-bit
//                  triangle counter by one atomic.
//   k_lcc_heavy    a fixed grid, one wave per list entry; a workgroup takes kLccChunk consecutive entries of the list at a
//                  time and drains its cache behind each chunk; the list's length is read from device memory (the launch
//                  follows k_lcc_count on the stream).  The lanes stride over the shorter row 64 elements per step,
//                  kIsectDeep steps in flight.  A hitting lane credits w(i, j) to k (lcc_credit; the k of a step are
//                  distinct), the wave reduces the two weighted sums and its hits, and lane 0 adds the sums to num[i] and
//                  num[j]; the hits go to the triangle counter once per wave, at its end.
// The two intersections (isect_lane, isect_wave), the heavy list (IsectHeavy, IsectHeavyList) and their constants are
// sel_rows.hpp's, shared with dot.hip; the credits of a hit are written at the two calls.
// One synchronisation reads the counters (heavy entries, triangles, reciprocal) and, where the caller asked for degrees or
// coefficients, S.row_ptr and num; the coefficients are computed on the host in double from those integers.
//
// Visibility.  Every kernel reads only what an EARLIER launch on the same stream wrote (T, R, the weight bytes, the list and
// its length, the zeroed num) or what was there before the call.  num, the triangle and reciprocal counters and the list's
// append counter are written by device-scope atomicAdd alone; only the append's return value is used, to place the entry.
// The LDS cache is a workgroup's own: its slots are claimed and summed by LDS atomics and read after a barrier.
// Nothing in these launches reads num.  Integer addition commutes and every partial sum is bounded by the final value
// (<= nnz(S) <= INT_MAX), so the bits do not depend on scheduling; the ORDER of the list does, and changes nothing.  No
// kernel waits for another workgroup; every loop is bounded by a row's length or the list's.
//
// Cost.  Sum over the entries (i, j) of T of min(|T_i|, |T_j|) searches and two LDS atomics per triangle; the global atomics
// on a hub's counter fall from one per triangle to one per workgroup and chunk (DESIGN.md 4.20 has the numbers before and
// after).  A heavy entry is walked by ONE wave; splitting a hub-hub entry over several waves is not done.
#include "internal.hpp"
#include "sel_rows.hpp"

#include <algorithm>

namespace bsp {

constexpr int kLccChunk = 64;           // consecutive list entries that a workgroup of k_lcc_heavy takes at a time

struct LccCounters {
    u64 triangles;          // hits of the intersections: every triangle of S once
    u64 reciprocal;         // entries of T that are in R
    int heavy;              // entries appended to the heavy list
    int pad;
};
constexpr size_t kLccCounterInts = 8;   // the block that is zeroed: the counters in whole 16-byte units
static_assert(sizeof(LccCounters) <= kLccCounterInts * sizeof(int), "the counters fit their block");

// The per-hit credit num[k] += w goes through a small cache in LDS, one per workgroup: slot k mod kLccSlots belongs to the
// first k that claims it (atomicCAS on the slot's tag), that k's credits are summed in LDS and reach num[k] by ONE global
// atomic when the workgroup is done; a k that finds its slot taken by another goes to num[k] directly.  Without it the
// hits on a hub's counter -- one per triangle at its lowest corner -- arrive one by one at one address (DESIGN.md 4.20:
// k_lcc_count took 13.1 ms on the Graph500-skew graph, 2.2 ms with the cache).  Sums of integers: the bits do not depend
// on who claimed which slot.
constexpr int kLccSlots = 1024;         // 8 KiB of LDS beside the 16 KiB window of row_ptr: six workgroups per CU
static_assert((kLccSlots & (kLccSlots - 1)) == 0 && kLccSlots % kSelThreads == 0, "a power of two, whole rounds of the workgroup");

// called by every thread of the workgroup, before a barrier that precedes the first lcc_credit
__device__ __forceinline__ void lcc_cache_clear(int *tag, int *val)
{
    for (int q = threadIdx.x; q < kLccSlots; q += kSelThreads) {
        tag[q] = -1;
        val[q] = 0;
    }
}

// k in [0, n): tested by the caller
__device__ __forceinline__ void lcc_credit(int *tag, int *val, int *num, int k, int w)
{
    const int slot = k & (kLccSlots - 1);
    const int owner = atomicCAS(&tag[slot], -1, k);
    if (owner == -1 || owner == k) atomicAdd(&val[slot], w);
    else atomicAdd(&num[k], w);
}

// called by every thread of the workgroup when no lcc_credit can follow (it holds the barrier)
__device__ __forceinline__ void lcc_cache_flush(const int *tag, const int *val, int *num)
{
    __syncthreads();
    for (int q = threadIdx.x; q < kLccSlots; q += kSelThreads) {
        const int k = tag[q], v = val[q];
        if (k >= 0 && v) atomicAdd(&num[k], v);
    }
}

// the same, and the cache is empty again for the credits behind the second barrier
__device__ __forceinline__ void lcc_cache_drain(int *tag, int *val, int *num)
{
    __syncthreads();
    for (int q = threadIdx.x; q < kLccSlots; q += kSelThreads) {
        const int k = tag[q], v = val[q];
        if (k >= 0 && v) atomicAdd(&num[k], v);
        tag[q] = -1;
        val[q] = 0;
    }
    __syncthreads();
}

// row v of the result holds (v, v); its value starts at 0
__global__ __launch_bounds__(256) void k_lcc_init(int n, long long *__restrict__ row_ptr, int *__restrict__ col_idx,
                                                  int *__restrict__ num)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v <= n) row_ptr[v] = v;
    if (v < n) {
        col_idx[v] = (int)v;
        num[v] = 0;
    }
}

// The weights as an op of sel_walk_entries.  T's column is only compared with R's, never used as an index.
struct LccWeights {
    const int *__restrict__ rpR, *__restrict__ colR;
    unsigned char *__restrict__ wgt;
    int r0, rlen;                       // the extent of R's row of the row the lane is in
    int found;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int r)
    {
        r0 = rpR[r];
        rlen = rpR[r + 1] - r0;
    }
    __device__ __forceinline__ void entry(int, long long p, int j, int)
    {
        const int at = sel_lower_bound(colR + r0, 0, rlen, j);
        const bool both = at < rlen && colR[r0 + at] == j;
        wgt[p] = both ? 2 : 1;
        found += both ? 1 : 0;
    }
};

__global__ __launch_bounds__(kSelThreads) void k_lcc_weights(const int *__restrict__ rpT, const int *__restrict__ colT, int n,
                                                            long long E, bool vec, const int *__restrict__ tile_row,
                                                            const int *__restrict__ rpR, const int *__restrict__ colR,
                                                            unsigned char *__restrict__ wgt, u64 *reciprocal)
{
    LccWeights op = {rpR, colR, wgt, 0, 0, 0};
    sel_walk_entries<false>(rpT, colT, n, E, vec, tile_row, op);         // (T's columns are read again by k_lcc_count)
    const int found = wave_sum(op.found);
    if (found && lane_id() == 0) atomicAdd(reciprocal, (u64)found);
}

// The count as an op of sel_walk_entries.  num is written by atomics alone and read by nobody here: neither const nor
// __restrict__.
template <bool DIRECTED>
struct LccCount {
    const int *__restrict__ rp, *__restrict__ col;
    const unsigned char *__restrict__ wgt;
    int n, T;
    int *num;
    int *tag, *val;                     // the workgroup's credit cache (LDS)
    int a0, alen;                       // the extent of the row the lane is in
    int cur, acc;                       // that row, and the credit it is owed so far
    int hits;
    IsectHeavy heavy;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void flush()
    {
        if (acc) atomicAdd(&num[cur], acc);                  // (acc != 0 only after row(): cur is a row of T)
        acc = 0;
    }
    __device__ __forceinline__ void row(int r)
    {
        if (r != cur) {
            flush();
            cur = r;
        }
        a0 = rp[r];
        alen = rp[r + 1] - a0;
    }
    __device__ __forceinline__ void entry(int r, long long p, int j, int s)
    {
        if ((unsigned)j >= (unsigned)n) return;              // before j indexes anything
        const int b0 = rp[j], blen = rp[j + 1] - b0;
        const bool a_short = alen <= blen;
        const int m = a_short ? alen : blen;
        if (m == 0) return;
        if (m > T) {                                         // heavy: k_lcc_heavy credits the entry's triangles
            heavy.note(s, r);
            return;
        }
        const int x0 = a_short ? a0 : b0, y0 = a_short ? b0 : a0;   // walked, searched
        const int wij = DIRECTED ? wgt[p] : 2;
        int sx = 0, sy = 0;                                  // the weights of the hits' entries in the walked / searched row
        isect_lane(col + x0, m, col + y0, a_short ? blen : alen, [&](bool hit, int q, int at, int c) {
            if (hit) {
                hits++;
                if ((unsigned)c < (unsigned)n) lcc_credit(tag, val, num, c, wij);
                sx += DIRECTED ? wgt[x0 + q] : 2;
                sy += DIRECTED ? wgt[y0 + at] : 2;
            }
        });
        const int wik = a_short ? sx : sy, wjk = a_short ? sy : sx;
        if (wik) atomicAdd(&num[j], wik);
        acc += wjk;
    }
};

template <bool DIRECTED>
__global__ __launch_bounds__(kSelThreads) void k_lcc_count(const int *__restrict__ rpT, const int *__restrict__ colT, int n,
                                                          long long E, bool vec, const int *__restrict__ tile_row,
                                                          const unsigned char *__restrict__ wgt, int T, int *num,
                                                          int2 *__restrict__ list, LccCounters *cnt)
{
    __shared__ int tag[kLccSlots], val[kLccSlots];
    lcc_cache_clear(tag, val);                                           // (the walk's staging barrier follows)
    LccCount<DIRECTED> op = {rpT, colT, wgt, n, T, num, tag, val, 0, 0, -1, 0, 0, {0u, {}}};
    sel_walk_entries<false>(rpT, colT, n, E, vec, tile_row, op);
    lcc_cache_flush(tag, val, num);
    op.flush();
    const int hits = wave_sum(op.hits);
    if (hits && lane_id() == 0) atomicAdd(&cnt->triangles, (u64)hits);
    op.heavy.append(list, &cnt->heavy, E);
}

// one wave per entry of `list`, k_lcc_count's
template <bool DIRECTED>
__global__ __launch_bounds__(kSelThreads) void k_lcc_heavy(const int *__restrict__ rp, const int *__restrict__ col, int n,
                                                          const unsigned char *__restrict__ wgt, const int2 *__restrict__ list,
                                                          long long cap, int *num, LccCounters *cnt)
{
    __shared__ int tag[kLccSlots], val[kLccSlots];
    lcc_cache_clear(tag, val);
    __syncthreads();
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const IsectHeavyList hl(list, &cnt->heavy, cap, n);
    const long long nh = hl.n;                               // (k_lcc_count's: nothing in this launch appends)
    int triangles = 0;                                       // the wave's hits over all its entries (at most nnz(S) / 6 in all)
    // A workgroup takes `chunk` CONSECUTIVE list entries at a time, its waves striding inside the chunk, and drains its
    // cache behind every chunk: neighbours in the list are neighbours in T (a wave appends up to 64 entries out of 256
    // consecutive ones at once), they share their row and with it the k they credit, so a chunk's credits meet in the
    // cache; entries dealt out one by one over the grid share nothing.  A short list gets shorter chunks, so that it still
    // spreads over the grid.
    long long chunk = (nh + gridDim.x - 1) / gridDim.x;
    chunk = chunk > kLccChunk ? kLccChunk : ((chunk + kIsectWaves - 1) / kIsectWaves) * kIsectWaves;
    for (long long h0 = (long long)blockIdx.x * chunk; h0 < nh; h0 += (long long)gridDim.x * chunk) {   // (workgroup-uniform)
        const long long h1 = h0 + chunk < nh ? h0 + chunk : nh;
        for (long long h = h0 + w; h < h1; h += kIsectWaves) {                                                 // (wave-uniform)
            int p, i;
            if (!hl.entry(h, p, i)) continue;
            const int j = wave_first(col[p]);
            if ((unsigned)j >= (unsigned)n) continue;
            const int a0 = rp[i], alen = rp[i + 1] - a0, b0 = rp[j], blen = rp[j + 1] - b0;
            const bool a_short = alen <= blen;
            const int x0 = a_short ? a0 : b0, y0 = a_short ? b0 : a0;       // strided over, searched
            const int wij = DIRECTED ? wgt[p] : 2;
            int sx = 0, sy = 0, hits = 0;
            isect_wave<kIsectDeep>(col + x0, a_short ? alen : blen, col + y0, a_short ? blen : alen, lane,
                                   [&](bool hit, int q, int at, int c) {
                                       if (hit) {           // (the k of a step are distinct)
                                           hits++;
                                           if ((unsigned)c < (unsigned)n) lcc_credit(tag, val, num, c, wij);
                                           sx += DIRECTED ? wgt[x0 + q] : 2;
                                           sy += DIRECTED ? wgt[y0 + at] : 2;
                                       }
                                   });
            sx = wave_sum(sx);
            sy = wave_sum(sy);
            hits = wave_sum(hits);
            if (lane == 0) {
                const int wik = a_short ? sx : sy, wjk = a_short ? sy : sx;
                if (wik) atomicAdd(&num[j], wik);
                if (wjk) atomicAdd(&num[i], wjk);
            }
            triangles += hits;
        }
        lcc_cache_drain(tag, val, num);
    }
    // one atomic per wave, not per entry: millions of adds to one word run one after the other
    if (triangles && lane == 0) atomicAdd(&cnt->triangles, (u64)(unsigned)triangles);
}

}  // namespace bsp

using namespace bsp;

// ------------------------------------------------------------------ the host side --------
static const char kLccWho[] = "bspgemm_local_clustering";

extern "C" bspgemm_status bspgemm_local_clustering(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags,
                                                   bspgemm_result **counts, int *degree_host, double *lcc_host,
                                                   bspgemm_lcc_info *info)
{
    if (counts) *counts = nullptr;
    if (info) *info = bspgemm_lcc_info{0, 0, 0, 0};
    if (!ctx || !A || !counts) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_local_clustering: NULL argument");
    if (flags & ~BSPGEMM_LCC_DIRECTED) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_local_clustering: unknown flag");
    if (bspgemm_status st = check_operand(ctx, A, kLccWho, NEED_SQUARE)) return st;
    const bool directed = (flags & BSPGEMM_LCC_DIRECTED) != 0;
    // BSPGEMM_LCC_TIMING: host clocks around the stages, each synchronised; 2: the stage split on the half that is NOT kept
    StageClock clk(ctx->lcc_timing != 0, ctx->stream);
    const bspgemm_select side = ctx->lcc_timing == 2 ? BSPGEMM_SELECT_TRIU : BSPGEMM_SELECT_TRIL;
    double ms_sym = 0, ms_weights = 0, ms_count = 0, ms_heavy = 0, ms_finish = 0;

    // the operands: S, its oriented half T and (DIRECTED) R = A' and A'^T, A' = A without its diagonal.  DIRECTED spells
    // bspgemm_matrix_symmetrize out, so that A' and its transpose serve both the union and the intersection
    bspgemm_matrix *S = nullptr, *T = nullptr, *R = nullptr;
    bspgemm_result *res = nullptr;
    int *h_rp = nullptr, *h_num = nullptr;
    auto drop = [&]() {
        free(h_num);
        free(h_rp);
        bspgemm_matrix_free(R);
        bspgemm_matrix_free(T);
        bspgemm_matrix_free(S);
    };
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(ctx->stream);
        bspgemm_result_free(res);
        drop();
        return st;
    };
    // the workspace is grown ONCE, before anything is launched (growing it synchronises), to the most that any stage takes:
    // the symmetrize's stages and the intersection (setop.hip), the select of a half of S (at most 2 nnz(A) entries), and
    // the call's own state for at most nnz(A) entries of T (the counters, the heavy list {p, row} and the weight bytes)
    if (bspgemm_status st0 = use_device(ctx)) return st0;
    // the call's own state for e entries of T: the counter block, the heavy list {p, row} and (DIRECTED) the weight bytes,
    // the two arrays in whole 16-byte units
    LccCounters *d_cnt = nullptr;
    int2 *list = nullptr;
    unsigned char *wgt = nullptr;
    auto carve = [&](int *tmp, long long e) {
        return WsCursor(tmp).take(d_cnt, 1).take(list, ws_pad4(2 * (size_t)e) / 2)
            .take_if(directed, wgt, ((size_t)e + 15) & ~(size_t)15).ints();
    };
    {
        const size_t own = carve(nullptr, A->nnz);
        const size_t sel = A->nnz <= INT_MAX ? flag_scratch_carve(nullptr, 0, 2 * A->nnz, false, nullptr) : 0;
        if (bspgemm_status st0 = ensure_tmp(ctx, std::max(std::max(symmetrize_workspace_ints(A->nnz, A->rows), sel), own))) return st0;
    }
    bspgemm_status st = BSPGEMM_OK;
    if (directed) {
        bspgemm_matrix *off = nullptr, *t = nullptr;
        st = bspgemm_matrix_select(ctx, A, BSPGEMM_SELECT_OFFDIAG, &off);
        if (!st) st = bspgemm_matrix_transpose(ctx, off, &t);
        if (!st) st = bspgemm_matrix_setop(ctx, off, t, BSPGEMM_SETOP_OR, &S);
        if (!st) st = bspgemm_matrix_setop(ctx, off, t, BSPGEMM_SETOP_AND, &R);
        bspgemm_matrix_free(t);
        bspgemm_matrix_free(off);
    } else {
        st = bspgemm_matrix_symmetrize(ctx, A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL, &S);
    }
    if (!st) st = bspgemm_matrix_select(ctx, S, side, &T);
    if (st) return bail(st);
    hipStream_t s = ctx->stream;
    (void)clk.lap(ms_sym, true);
    const int n = S->rows;
    const long long E = T->nnz;

    // the call's own state: the counters, the heavy list {p, row} and the weight bytes
    if (E > 0) {
        if (bspgemm_status st2 = ensure_tmp(ctx, carve(nullptr, E))) return bail(st2);   // (there already, see above: E <= nnz(A))
        if (bspgemm_status st2 = ensure_tile_rows(ctx, (size_t)E)) return bail(st2);
    }
    if (degree_host || lcc_host) {
        h_rp = static_cast<int *>(malloc(((size_t)n + 1) * sizeof(int)));
        if (!h_rp) return bail(FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_local_clustering: host memory for the degrees"));
    }
    if (lcc_host) {
        h_num = static_cast<int *>(malloc(((size_t)n + 1) * sizeof(int)));
        if (!h_num) return bail(FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_local_clustering: host memory for the counts"));
    }
    // the result, allocated as a product's is: its values are num[] while the kernels run
    if (bspgemm_status st2 = counted_result_new(ctx, n, n, &res)) return bail(st2);
    int *num = res->d_values;
    hipLaunchKernelGGL(k_lcc_init, vertex_grid(n, 256), dim3(256), 0, s, n, res->d_row_ptr, res->d_col_idx, num);
    HIPCHK_B(hipGetLastError());

    LccCounters h = {};
    if (E > 0) {                                             // without entries in T: all zeros, no intersection kernel
        carve(ctx->tmp, E);
        const dim3 grid(select_tiles(E)), block(kSelThreads);
        const bool vec = aligned16(T->d_col_idx);
        clk.start();
        auto stage = [&](double &ms) { return clk.lap(ms, true); };   // (timed only: a synchronisation behind the stage)
        HIPCHK_B(hipMemsetAsync(d_cnt, 0, kLccCounterInts * sizeof(int), s));
        launch_select_tile_rows(T->d_row_ptr, n, ctx->tile_row, s);
        if (directed) {
            hipLaunchKernelGGL(k_lcc_weights, grid, block, 0, s, T->d_row_ptr, T->d_col_idx, n, E, vec, ctx->tile_row,
                               R->d_row_ptr, R->d_col_idx, wgt, &d_cnt->reciprocal);
            HIPCHK_B(stage(ms_weights));
            hipLaunchKernelGGL(k_lcc_count<true>, grid, block, 0, s, T->d_row_ptr, T->d_col_idx, n, E, vec, ctx->tile_row, wgt,
                               ctx->dot_light, num, list, d_cnt);
            HIPCHK_B(stage(ms_count));
            hipLaunchKernelGGL(k_lcc_heavy<true>, dim3(kIsectHeavyGrid), block, 0, s, T->d_row_ptr, T->d_col_idx, n, wgt, list, E,
                               num, d_cnt);
        } else {
            hipLaunchKernelGGL(k_lcc_count<false>, grid, block, 0, s, T->d_row_ptr, T->d_col_idx, n, E, vec, ctx->tile_row, wgt,
                               ctx->dot_light, num, list, d_cnt);
            HIPCHK_B(stage(ms_count));
            hipLaunchKernelGGL(k_lcc_heavy<false>, dim3(kIsectHeavyGrid), block, 0, s, T->d_row_ptr, T->d_col_idx, n, wgt, list, E,
                               num, d_cnt);
        }
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(stage(ms_heavy));
        HIPCHK_B(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
    }
    clk.start();
    if (h_rp) HIPCHK_B(hipMemcpyAsync(h_rp, S->d_row_ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    if (h_num && n > 0) HIPCHK_B(hipMemcpyAsync(h_num, num, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));                                        // the call's one synchronisation
    if (h.heavy < 0 || h.heavy > E || h.triangles > (u64)LLONG_MAX || h.reciprocal > (u64)E)
        return bail(FAIL(BSPGEMM_ERR_HIP, "bspgemm_local_clustering: counters out of range"));
    for (int v = 0; v < n && h_rp; v++) {
        const int d = h_rp[v + 1] - h_rp[v];
        if (degree_host) degree_host[v] = d;
        if (lcc_host) lcc_host[v] = d < 2 ? 0.0 : (double)h_num[v] / ((double)d * (double)(d - 1));
    }
    if (clk.on) {
        (void)clk.lap(ms_finish);
        fprintf(stderr, "[bspgemm] %s: n %d nnz(S) %lld %s %s | total %.3f ms = symmetrize and select %.3f + weights %.3f + count %.3f "
                        "+ heavy %.3f (%d of %lld entries) + finish %.3f + rest | triangles %llu\n",
                kLccWho, n, (long long)S->nnz, directed ? "directed" : "undirected", side == BSPGEMM_SELECT_TRIL ? "TRIL" : "TRIU",
                clk.total(), ms_sym, ms_weights, ms_count, ms_heavy, h.heavy, E, ms_finish, h.triangles);
    }
    if (info) {
        info->triangles = (int64_t)h.triangles;
        info->entries = E;
        info->heavy_entries = h.heavy;
        info->reciprocal = directed ? (int64_t)h.reciprocal : 0;
    }
    drop();
    *counts = res;
    return BSPGEMM_OK;
}
