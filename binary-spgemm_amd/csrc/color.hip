// color.hip -- greedy graph colouring with deterministic colours, everything device-resident: bspgemm_graph_coloring
// (include/bspgemm.h).  No product: a Jones-Plassmann sweep with first fit, which is a level-synchronous peeling of the
// priority DAG of the simple undirected graph S = bspgemm_matrix_symmetrize(A, DROP_DIAGONAL) (sorted duplicate-free rows,
// no diagonal, every column in [0, n): the transpose inside symmetrize tests them).  Every vertex has a 64-bit key (the
// header gives the formula); w PRECEDES u when (key[w], w) < (key[u], u).  The arrays:
//     key[n]     64-bit, from the order, the seed and S.row_ptr                               (workspace)
//     cnt[n]     preceding neighbours of v that are not coloured yet                         (workspace)
//     colour[n]  -1 = uncoloured; the col_idx of the assignment operand P that the call returns, so nothing is copied
//     list[2][n] two frontier lists that the launches ping-pong                              (workspace)
// and a block of four counters.
//     k_color_init    per vertex: key, colour = -1, cnt = 0, P.row_ptr
//     k_color_count   per stored entry (u, w) of S, in select's geometry (sel_rows.hpp: a workgroup owns kSelTile consecutive
//                     entries whatever rows they belong to -- a hub row costs what its entries cost): w precedes u adds one to
//                     cnt[u]; a lane sums the entries it walks of one row and adds the sum by one atomicAdd
//     k_color_seed    per vertex: cnt[v] == 0 appends v to list 0 (ballot, one atomicAdd per wave, lane rank by mbcnt)
//     k_color_round   one wave per frontier vertex u, its lanes striding over S's row u.  A neighbour w that precedes u:
//                     colour[w] (plain load) is marked in the wave's LDS bitmap of kColWindow colours, if it lies in
//                     [base, base + kColWindow) -- anything else is ignored, which is what keeps a mark inside the bitmap.  A
//                     neighbour w that follows u: atomicSub(&cnt[w], 1) at device scope, and the one decrement that returns
//                     1 appends w to the OTHER list.  First fit: lane i reads word i, a ballot of the words that are not
//                     all ones finds the first free bit.  A full window (u then has at least base + kColWindow preceding
//                     neighbours) moves base up by kColWindow, clears the bitmap and walks the row again for the colours
//                     alone: the release happens in the first walk only.  The wave's colour goes into the `top` counter by
//                     atomicMax.  One read-back of the other list's size; the lists swap until it is empty.
// Invariants.  cnt[u] starts as the number of u's preceding neighbours and is lowered once by each of them, in the launch
// that colours it: the atomics on cnt[u] return every value from that number down to 1 exactly once, so exactly one
// returns 1 -- u is appended exactly once, by the launch that colours its LAST preceding neighbour (or by the seed, when it
// has none), and its own launch is a LATER one: every preceding neighbour of u was coloured by an earlier launch.  Two
// vertices of one frontier are never adjacent (one of them would precede the other and still be uncoloured).  So colour[u]
// = the smallest colour that no preceding neighbour has = what sequential first fit gives in the order of (key, id): by
// induction along that order the colours are unique, and every run gives the same bits.  The number of launches is the
// number of vertices on the longest chain of ascending (key, id) along edges of S.  The ORDER inside a list depends on
// scheduling and changes nothing: a launch consumes the whole list.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores.  Every decision
// rests on the return value of a device-scope atomic (cnt, the list sizes) or on values from before the launch: key[], S,
// the list and its size, and colour[] of PRECEDING neighbours.  colour[] of any other vertex is never read.  The one plain
// load of a word that the same launch changes is the filter in front of the atomicMax on `top`: a stale value is an older,
// LOWER one, so it only lets an atomic through that was not needed.  No kernel waits for another workgroup: every loop is
// bounded by the thread's own row, by the list size the host passed in, or by the row's length / kColWindow window passes.
//
// Cost.  One synchronisation per launch (4 bytes read back), so a path stored in ascending order takes n launches: the
// call is bound by `rounds` on anything but a dense graph.  Every stored entry of S is walked once by the
// count and once by its row's wave, with one atomic or one LDS mark.  A frontier vertex's row is walked by ONE wave, 64
// entries per step and once per window pass: a hub in the frontier is a serial tail of degree / 64 steps, NOT the "a hub
// costs what its entries cost" geometry of the count.  The host caps the loop at n launches and never spins.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

constexpr int kColThreads = 256;
constexpr int kColWaves = kColThreads / 64;
constexpr int kColWindow = 2048;        // colours of one bitmap window: 64 words, one per lane
constexpr int kColDeep = 4;             // 64-entry steps of a row in flight per trip of the walk (measured: DESIGN.md 4.16)

struct ColFlags {
    int size[2];            // entries appended to list 0 / list 1 by the launch that writes it
    int top;                // the largest colour so far
    int pad;
};

// (key[w], w) < (key[u], u)
__device__ __forceinline__ bool col_precedes(u64 kw, int w, u64 ku, int u) { return kw < ku || (kw == ku && w < u); }

// The frontier lists are appended to by wave_append (wave.hpp).  A vertex is appended once in its life, so a list never
// passes n entries; the store is bounded all the same.

// order: a bspgemm_color_order.  rpS NULL (S has no entries): every degree is 0 and the colours are final (fill = 0).
__global__ __launch_bounds__(kColThreads) void k_color_init(int n, int order, u32 seed, const int *__restrict__ rpS,
                                                           u64 *__restrict__ key, int *__restrict__ cnt,
                                                           int *__restrict__ colour, int *__restrict__ row_ptr, int fill)
{
    const long long v = (long long)blockIdx.x * kColThreads + threadIdx.x;
    if (v <= n) row_ptr[v] = (int)v;
    if (v < n) {
        colour[v] = fill;
        if (rpS) {
            const u32 lo = order == BSPGEMM_COLOR_NATURAL ? (u32)v : mix32((u32)v ^ seed);
            const u32 hi = order == BSPGEMM_COLOR_LARGEST_FIRST ? 0x7fffffffu - (u32)(rpS[v + 1] - rpS[v]) : 0u;
            key[v] = ((u64)hi << 32) | lo;
            cnt[v] = 0;
        }
    }
}

// The count as an op of sel_walk_entries: the lane sums the preceding neighbours among the entries it walks of one row
// and adds the sum when it leaves the row.  The columns need no range check: S is symmetrize's output.
struct ColCount {
    const u64 *__restrict__ key;
    int *cnt;
    int u, acc;
    u64 ku;
    __device__ __forceinline__ void flush()
    {
        if (acc) atomicAdd(&cnt[u], acc);
        acc = 0;
    }
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int r)
    {
        flush();
        u = r;
        ku = key[r];
    }
    __device__ __forceinline__ void entry(int, long long, int w, int) { acc += col_precedes(key[w], w, ku, u) ? 1 : 0; }
};

__global__ __launch_bounds__(kSelThreads) void k_color_count(const int *__restrict__ rpS, const int *__restrict__ colS, int n,
                                                            long long E, bool vec, const int *__restrict__ tile_row,
                                                            const u64 *__restrict__ key, int *cnt)
{
    ColCount op = {key, cnt, 0, 0, 0};
    sel_walk_entries<false>(rpS, colS, n, E, vec, tile_row, op);
    op.flush();
}

__global__ __launch_bounds__(kColThreads) void k_color_seed(int n, const int *__restrict__ cnt, int *__restrict__ list,
                                                           ColFlags *flags)
{
    const long long v = (long long)blockIdx.x * kColThreads + threadIdx.x;
    const bool take = v < n && cnt[v] == 0;
    wave_append(take, (int)v, list, &flags->size[0], n, lane_id());
}

// one wave per vertex of `list` (fsize entries, from the host).  cnt is lowered by atomics only; colour is loaded plainly
// (preceding neighbours: stored by earlier launches) and stored (the wave's own vertex) in the same launch: neither const
// nor __restrict__.  `reset` is the size word of the list being read: the host has it already, and the next launch appends
// to that list.
__global__ __launch_bounds__(kColThreads) void k_color_round(int n, int fsize, const int *__restrict__ list,
                                                            const int *__restrict__ rpS, const int *__restrict__ colS,
                                                            const u64 *__restrict__ key, int *cnt, int *colour,
                                                            int *__restrict__ next, int *next_size, int *reset, int *top)
{
    __shared__ u32 bits[kColWaves][kColWindow / 32];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long f = (long long)blockIdx.x * kColWaves + w;
    if (blockIdx.x == 0 && threadIdx.x == 0) *reset = 0;
    if (f >= fsize) return;                                  // (wave-uniform)
    const int u = list[f];
    const u64 ku = key[u];
    const long long b0 = rpS[u];
    const int e = rpS[u + 1];
    u32 *bm = bits[w];
    bm[lane] = 0u;
    wave_lds_fence();
    bool prev = false;
    // kColDeep steps of 64 entries per trip, stage by stage (columns, keys, then the colour loads and the atomics), so that
    // a long row pays the three dependent memory latencies once per kColDeep * 64 entries
    for (long long b = b0; b < e; b += 64 * kColDeep) {      // (64-bit: e may be INT_MAX)
        int x[kColDeep], old[kColDeep];
        u64 kx[kColDeep];
        bool in[kColDeep];
#pragma unroll
        for (int j = 0; j < kColDeep; j++) {
            in[j] = b + 64 * j + lane < e;
            x[j] = in[j] ? colS[b + 64 * j + lane] : 0;      // in [0, n): S is symmetrize's output
        }
#pragma unroll
        for (int j = 0; j < kColDeep; j++) kx[j] = in[j] ? key[x[j]] : 0;
#pragma unroll
        for (int j = 0; j < kColDeep; j++) {
            old[j] = 0;
            if (!in[j]) continue;
            if (col_precedes(kx[j], x[j], ku, u)) {
                prev = true;
                const unsigned c = (unsigned)colour[x[j]];   // (an uncoloured -1 would be outside every window)
                if (c < (unsigned)kColWindow) atomicOr(&bm[c >> 5], 1u << (c & 31));
            } else {
                old[j] = atomicSub(&cnt[x[j]], 1);
            }
        }
#pragma unroll
        for (int j = 0; j < kColDeep; j++) wave_append(old[j] == 1, x[j], next, next_size, n, lane);
    }
    int c = 0;
    if (__ballot(prev)) {                                    // (wave-uniform)
        int base = 0;
        for (;;) {
            wave_lds_fence();
            const u32 word = bm[lane];
            const u64 open = __ballot(word != ~0u);
            if (open) {
                const int l = __ffsll((long long)open) - 1;
                const u32 first = (u32)wave_bcast((int)word, l);
                c = base + 32 * l + (__ffs((int)~first) - 1);
                break;
            }
            // every colour of the window is taken: at least base + kColWindow preceding neighbours, so base stays an int
            base += kColWindow;
            wave_lds_fence();
            bm[lane] = 0u;
            wave_lds_fence();
            for (long long b = b0; b < e; b += 64 * kColDeep) {   // colours only: the release is not repeated
                int x[kColDeep];
                u64 kx[kColDeep];
                bool in[kColDeep];
#pragma unroll
                for (int j = 0; j < kColDeep; j++) {
                    in[j] = b + 64 * j + lane < e;
                    x[j] = in[j] ? colS[b + 64 * j + lane] : 0;
                }
#pragma unroll
                for (int j = 0; j < kColDeep; j++) kx[j] = in[j] ? key[x[j]] : 0;
#pragma unroll
                for (int j = 0; j < kColDeep; j++) {
                    if (in[j] && col_precedes(kx[j], x[j], ku, u)) {
                        const unsigned d = (unsigned)(colour[x[j]] - base);   // below base: wraps past the window
                        if (d < (unsigned)kColWindow) atomicOr(&bm[d >> 5], 1u << (d & 31));
                    }
                }
            }
        }
    }
    if (lane == 0) {
        colour[u] = c;
        if (c > *top) atomicMax(top, c);                     // (a stale *top is a lower one: see the file head)
    }
}

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_graph_coloring(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_color_order order,
                                                 unsigned seed, bspgemm_matrix **P, int *ncolors, int *rounds)
{
    static const char who[] = "bspgemm_graph_coloring";
    if (P) *P = nullptr;
    if (ncolors) *ncolors = 0;
    if (rounds) *rounds = 0;
    if (!ctx || !A || !P) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_graph_coloring: NULL argument");
    if (order != BSPGEMM_COLOR_NATURAL && order != BSPGEMM_COLOR_RANDOM && order != BSPGEMM_COLOR_LARGEST_FIRST)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_graph_coloring: unknown order");
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_SQUARE)) return st;
    // BSPGEMM_COLOR_TIMING: host clocks around the stages; a launch is then synchronised before its read-back is issued, so
    // that the two are told apart
    StageClock clk(ctx->color_timing, ctx->stream);
    double ms_sym = 0, ms_count = 0, ms_launch = 0, ms_back = 0;
    if (bspgemm_status st = use_device(ctx)) return st;
    // The workspace grows ONCE per call: to what the symmetrize takes at most over its stages or, if that is more, to the
    // call's own state (the counters, key, cnt and the two lists), instead of stage by stage with a synchronisation each.
    const size_t n4 = ws_pad4((size_t)A->rows);
    ColFlags *d_flags = nullptr;
    u64 *key = nullptr;
    int *cnt = nullptr, *list[2] = {nullptr, nullptr};
    auto carve = [&](int *tmp) {
        return WsCursor(tmp).take(d_flags, 1).take(key, n4).take(cnt, n4).take(list[0], n4).take(list[1], n4).ints();
    };
    const size_t own_ints = carve(nullptr);
    bspgemm_matrix *S = nullptr;
    if (bspgemm_status st = symmetrized_operand(ctx, A, own_ints, A->nnz > 0, clk, ms_sym, &S)) return st;
    hipStream_t s = ctx->stream;
    const int n = S->rows;
    const long long E = S->nnz;                             // <= INT_MAX: symmetrize refuses more
    const bool edges = E > 0;
    bspgemm_matrix *m = nullptr;                            // the assignment operand: its col_idx is colour[]
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_matrix_free(m);
        bspgemm_matrix_free(S);
        return st;
    };
    // the counters, key, cnt and the two lists: carved before anything is launched (own_ints: there already, see above)
    if (edges) {
        if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return bail(st);
        if (bspgemm_status st = ensure_tmp(ctx, own_ints)) return bail(st);
        carve(ctx->tmp);
    }
    if (bspgemm_status st = assignment_operand(ctx, n, &m)) return bail(st);
    int *colour = m->d_col_idx;
    const dim3 vgrid = vertex_grid(n, kColThreads), block(kColThreads);
    clk.start();
    // without edges every vertex is isolated: colour 0, nothing to release
    hipLaunchKernelGGL(k_color_init, vgrid, block, 0, s, n, (int)order, (u32)seed, edges ? S->d_row_ptr : nullptr, key, cnt, colour,
                       m->d_row_ptr, edges ? -1 : 0);
    HIPCHK_B(hipGetLastError());
    int launches = 0, top = 0;
    if (edges) {
        HIPCHK_B(round_reset(d_flags, sizeof(ColFlags), s));
        launch_select_tile_rows(S->d_row_ptr, n, ctx->tile_row, s);
        hipLaunchKernelGGL(k_color_count, dim3(select_tiles(E)), dim3(kSelThreads), 0, s, S->d_row_ptr, S->d_col_idx, n, E,
                           aligned16(S->d_col_idx), ctx->tile_row, key, cnt);
        hipLaunchKernelGGL(k_color_seed, vgrid, block, 0, s, n, cnt, list[0], d_flags);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(clk.lap(ms_count, true));
        int fsize = 0, cur = 0;
        HIPCHK_B(hipMemcpyAsync(&fsize, &d_flags->size[0], sizeof fsize, hipMemcpyDeviceToHost, s));
        HIPCHK_B(hipStreamSynchronize(s));
        HIPCHK_B(clk.lap(ms_back));
        if (fsize <= 0 || fsize > n) return bail(fail_stuck(who));   // the first vertex of the order precedes everybody
        long long coloured = 0;
        while (fsize > 0) {
            if (launches >= n) return bail(fail_stuck(who));
            launches++;
            coloured += fsize;
            const dim3 rgrid((unsigned)(((long long)fsize + kColWaves - 1) / kColWaves));
            clk.start();
            hipLaunchKernelGGL(k_color_round, rgrid, block, 0, s, n, fsize, list[cur], S->d_row_ptr, S->d_col_idx, key, cnt, colour,
                               list[cur ^ 1], &d_flags->size[cur ^ 1], &d_flags->size[cur], &d_flags->top);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_launch, true));
            clk.longest(clk.last, fsize);
            HIPCHK_B(hipMemcpyAsync(&fsize, &d_flags->size[cur ^ 1], sizeof fsize, hipMemcpyDeviceToHost, s));
            HIPCHK_B(hipStreamSynchronize(s));              // the launch's one synchronisation
            HIPCHK_B(clk.lap(ms_back));
            if (fsize < 0 || fsize > n) return bail(fail_stuck(who));
            cur ^= 1;
        }
        if (coloured != n) return bail(fail_stuck(who));
        HIPCHK_B(hipMemcpyAsync(&top, &d_flags->top, sizeof top, hipMemcpyDeviceToHost, s));
    }
    if (bspgemm_status st = operand_finish(m, n)) return bail(st);   // one colour per vertex
    HIPCHK_B(hipStreamSynchronize(s));
    if (top < 0 || (n > 0 && top >= n)) return bail(fail_stuck(who));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: n %d nnz(S) %lld order %d colors %d | total %.3f ms = symmetrize %.3f + count %.3f + %d "
                        "launches %.3f + read-backs %.3f + rest | longest launch %.3f ms (%d frontier vertices)\n",
                who, n, E, (int)order, n ? top + 1 : 0, clk.total(), ms_sym, ms_count, launches, ms_launch, ms_back,
                clk.max_ms, clk.max_tag[0]);
    bspgemm_matrix_free(S);
    if (ncolors) *ncolors = n ? top + 1 : 0;
    if (rounds) *rounds = launches;
    *P = m;
    return BSPGEMM_OK;
}
