// cc.hip -- connected components with min-vertex labels, everything device-resident: bspgemm_connected_components
// (include/bspgemm.h).  No product: a label array parent[n] (allocated as the col_idx of the assignment operand P that the
// call returns, so nothing is copied at the end) and rounds of two kernels until a round writes nothing.
//     parent[v] = v
//     round:  k_cc_hook   per stored entry (u, v), v in range and v != u: pu = parent[u], pv = parent[v]; if they differ,
//                         atomicMin(&parent[max(pu, pv)], min(pu, pv)) at device scope.  Entry-parallel in select's geometry
//                         (sel_rows.hpp): a workgroup owns kSelTile consecutive entries of A whatever rows they belong to,
//                         a lane four of them per step (one 16-byte non-temporal load), the tile's window of A.row_ptr is
//                         staged in LDS -- a hub row costs what its entries cost.  A column outside [0, n) is tested BEFORE
//                         it indexes parent[], sets the `bad` word and is skipped.
//             k_cc_jump   per vertex: p = parent[v], kCcJumps times p = parent[p], stored back when it moved; counts the
//                         vertices with parent[v] == v (exact in the round that ends the loop).
//             one read-back of {changed, bad, roots} with the round's one synchronisation
// Invariant: parent[x] <= x at all times (the hook stores min < max, the jump stores an ancestor), so chains strictly
// decrease and cannot cycle, every value that parent[x] ever held lies in x's component, and so does every hook's pair.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores, so a plain load of
// parent[] inside a kernel may return an older value -- with monotone values an earlier ancestor, which costs rounds and
// nothing else.  Nothing waits: every loop's trip count is bounded by the thread's own entries or by kCcJumps.  The decision
// "converged" rests on a round with changed == 0: an atomicMin that lowers nothing and a jump that moves nothing store
// nothing, so every load of that round returned the value of the kernel boundary before it, the true one.  Then
// parent[parent[v]] == parent[v] for every v (every tree is a star) and parent[u] == parent[v] for every entry (a root r
// has parent[r] == r, so two different roots on one entry would have been hooked): one root per component, and by the
// invariant it is the component's smallest vertex.  Every other round lowers some parent value, so the loop ends; the host
// caps it at n + 2 rounds all the same and never spins.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

constexpr int kCcJumps = 2;             // pointer-jumping steps per vertex and round (measured: DESIGN.md 4.13)
constexpr int kCcThreads = 256;

struct CcFlags : SweepFlags {   // changed: a hook lowered a parent, or a jump moved one
    int roots;              // vertices with parent[v] == v after the jump
    unsigned pad;
};

// P.row_ptr = 0 .. n (k_bfs_unit_row_ptr's job) and parent[v] = v in one pass
__global__ __launch_bounds__(kCcThreads) void k_cc_init(int n, int *__restrict__ row_ptr, int *__restrict__ parent)
{
    const long long r = (long long)blockIdx.x * kCcThreads + threadIdx.x;
    if (r <= n) row_ptr[r] = (int)r;
    if (r < n) parent[r] = (int)r;
}

// The hook as an op of sel_sweep_graph (sel_rows.hpp), which walks the entries, tests the columns and skips self-loops.
// parent is read by plain loads and lowered by atomics in the same launch: neither const nor __restrict__
struct CcHook {
    int *parent;
    bool changed;
    int pu;
    __device__ __forceinline__ void row(int u) { pu = parent[u]; }
    __device__ __forceinline__ void edge(int, int v)
    {
        const int pv = parent[v];
        if (pu == pv) return;
        const int hi = max(pu, pv), lo = min(pu, pv);                    // both in [0, n): parent[x] <= x
        if (atomicMin(&parent[hi], lo) > lo) changed = true;
    }
};

__global__ __launch_bounds__(kSelThreads) void k_cc_hook(const int *__restrict__ row_ptr, const int *__restrict__ col, int n,
                                                        long long E, bool vec, const int *__restrict__ tile_row, int *parent,
                                                        CcFlags *__restrict__ flags)
{
    CcHook op = {parent, false, -1};
    sel_sweep_graph(row_ptr, col, n, E, vec, tile_row, flags, op);
}

// Only thread v stores parent[v] here, and what it stores is an ancestor not above the old value: a racing reader sees the
// old or the new one, both ancestors of v.
__global__ __launch_bounds__(kCcThreads) void k_cc_jump(int n, int *parent, CcFlags *__restrict__ flags)
{
    __shared__ int wroots[kCcThreads / 64];
    const long long v = (long long)blockIdx.x * kCcThreads + threadIdx.x;
    bool moved = false, root = false;
    if (v < n) {
        const int p0 = parent[v];
        int p = p0;
#pragma unroll
        for (int k = 0; k < kCcJumps; k++) p = parent[p];
        if (p != p0) {
            parent[v] = p;
            moved = true;
        }
        root = p == (int)v;
    }
    if (__ballot(moved) && lane_id() == 0) flags->changed = 1u;
    block_add<kCcThreads>(root, &flags->roots, nullptr, wroots);
}

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_connected_components(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_matrix **P,
                                                       int *ncomponents, int *rounds)
{
    static const char who[] = "bspgemm_connected_components";
    if (P) *P = nullptr;
    if (ncomponents) *ncomponents = 0;
    if (rounds) *rounds = 0;
    if (!ctx || !A || !P) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_connected_components: NULL argument");
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_SQUARE | NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const int n = A->rows;
    const long long E = A->nnz;
    CcFlags *d_flags = nullptr;
    auto carve = [&](int *tmp) { return WsCursor(tmp).take(d_flags, 1).ints(); };
    if (E > 0) {                                            // (before anything is launched: growing them synchronises)
        if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return st;
        if (bspgemm_status st = ensure_tmp(ctx, carve(nullptr))) return st;
    }
    bspgemm_matrix *m = nullptr;                            // the assignment operand: its col_idx is parent[]
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bspgemm_matrix_free(m); return st; };
    if (bspgemm_status st = assignment_operand(ctx, n, &m)) return bail(st);
    int *parent = m->d_col_idx;
    const dim3 vgrid = vertex_grid(n, kCcThreads), vblock(kCcThreads);
    hipLaunchKernelGGL(k_cc_init, vgrid, vblock, 0, s, n, m->d_row_ptr, parent);
    HIPCHK_B(hipGetLastError());
    CcFlags h = {};
    h.roots = n;                                            // without entries every vertex is a component
    int r = 0;
    if (E > 0) {
        carve(ctx->tmp);
        launch_select_tile_rows(A->d_row_ptr, n, ctx->tile_row, s);
        const dim3 egrid(select_tiles(E)), eblock(kSelThreads);
        const bool vec = aligned16(A->d_col_idx);
        const long long cap = (long long)n + 2;             // defensive: every round but the last lowers a parent value
        for (;;) {
            if (r >= cap) return bail(fail_stuck(who));
            r++;
            HIPCHK_B(round_reset(d_flags, sizeof(CcFlags), s));
            hipLaunchKernelGGL(k_cc_hook, egrid, eblock, 0, s, A->d_row_ptr, A->d_col_idx, n, E, vec, ctx->tile_row, parent,
                               d_flags);
            hipLaunchKernelGGL(k_cc_jump, vgrid, vblock, 0, s, n, parent, d_flags);
            HIPCHK_B(round_fetch(&h, d_flags, sizeof h, s));   // the round's one synchronisation
            if (h.bad) return bail(fail_bad_column(who, n));
            if (!h.changed) break;
        }
    }
    if (bspgemm_status st = operand_finish(m, n)) return bail(st);   // one label per vertex
    HIPCHK_B(hipStreamSynchronize(s));
    if (ncomponents) *ncomponents = h.roots;
    if (rounds) *rounds = r;
    *P = m;
    return BSPGEMM_OK;
}
