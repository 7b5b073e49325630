// scc.hip -- strongly connected components with min-vertex labels, everything device-resident:
// bspgemm_strongly_connected_components (include/bspgemm.h).  No product and no transpose: trimming plus min-colour
// propagation (Orzan's colouring, the "Multistep" family) on A alone, row u = the out-neighbours of u.  State:
//     label[n]    -1 = unassigned ("alive"); the col_idx of the assignment operand P that the call returns, so nothing is
//                 copied at the end
//     color[n], has_out[n], has_in[n] and a block of eight counters                                          (workspace)
// Self-loops (u == v) are skipped everywhere.  Three entry-parallel sweeps in select's geometry (sel_rows.hpp, as k_cc_hook:
// a workgroup owns kSelTile consecutive entries of A whatever rows they belong to, a lane four of them per step by one
// 16-byte non-temporal load, the tile's window of A.row_ptr staged in LDS -- a hub row costs what its entries cost) and three
// vertex-parallel passes:
//     trim     repeat until a pass removes nothing:
//                k_scc_mark   per entry (u, v) with both ends alive: has_out[u] = 1, has_in[v] = 1 (plain stores of the
//                             same value, no atomics).  label[] is only read in this launch, so the marks are those of the
//                             launch boundary and the sequence of trim passes is deterministic.
//                k_scc_trim   per vertex: an alive v that lacks either mark is an SCC by itself, label[v] = v; counts the
//                             removals and the vertices that stay alive, clears the marks and leaves color[v] = v for the
//                             vertices that stay alive and -1 for everybody else -- the start of a colouring round.
//     a colouring round on what is left:
//       forward  repeat until a repetition changes nothing:
//                k_scc_forward  per entry (u, v) with color[u] >= 0 and color[u] < color[v]: atomicMin(&color[v], color[u])
//                               at device scope (-1 marks a vertex that is not alive: it neither gives nor takes a colour)
//                k_scc_jump     per vertex: kSccJumps times color[v] = color[color[v]], stored when it moved
//       k_scc_roots  the alive v with color[v] == v: label[v] = v
//       backward repeat until a sweep stores nothing:
//                k_scc_backward per entry (u, v) with color[u] == color[v] >= 0, label[v] >= 0 and label[u] < 0:
//                               label[u] = color[u] (a plain store, every racer writes the same value)
//     every vertex labelled in the round drops out; trim again, then the next round.
//
// Why the labels are the minima.  color[v] = c always means "c is alive and reaches v" (c == v at the start; an entry
// (u, v) hands v a colour that reaches u; the jump hands v a colour that reaches color[v]), and color[v] <= v.  At the forward
// fixpoint color[u] >= color[v] over every entry between alive vertices, so color[v] is the SMALLEST alive vertex that
// reaches v: the smallest such a has color[a] == a (a colour below a would reach a and so v) and hands a down the path to v.
// A root r (color[r] == r) has no smaller ancestor, so it is the minimum of its SCC, and SCC(r) is exactly the vertices of
// colour r that reach r -- what the backward sweeps collect: they walk entries against their direction from r and never
// leave colour r, and every vertex of SCC(r) has colour r and a path to r inside it.  A labelled v with color[v] >= 0 was
// labelled in this round, with color[v]; the dead vertices of earlier rounds have color -1.  The smallest alive vertex is
// always a root, so a round removes at least one whole SCC; removing whole SCCs leaves the others intact, so starting the
// colours again on the remainder is correct.  A trimmed vertex has no alive in- or no alive out-neighbour apart from itself,
// so it lies on no cycle through alive vertices: an SCC by itself.  Every step's outcome is a unique fixpoint: the labels,
// the number of rounds and the number of trim passes are the same on every run.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores, so a plain load of
// color[] or label[] inside a launch that changes them may return an older value.  color[] only ever falls inside a round
// and label[] only goes from -1 to its final value: a stale colour is an earlier ancestor of the same vertex, a stale label
// is "not yet"; either costs sweeps and nothing else.  Every "converged" decision rests on a repetition that stored nothing:
// an atomicMin that lowers nothing, a jump that moves nothing and a backward sweep without a store leave memory as it was,
// so every load of that repetition returned the values of the kernel boundary before it, the true ones.  The marks are read
// by the next launch only.  No kernel waits for another workgroup: every loop is bounded by the thread's own entries or by
// kSccJumps.
//
// Cost.  Every sweep is one launch that reads all of A, and every repetition ends in one synchronisation with a read-back of
// 32 bytes.  A directed path of n vertices takes about n / 2 trim passes, a cycle of n vertices n backward sweeps (its
// forward sweeps are cut to about log n by the jump), a descending chain of k small SCCs k rounds.  The
// host caps every inner loop at n + 2 repetitions and the rounds at n and never spins.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

constexpr int kSccJumps = 1;            // pointer-jumping steps per vertex and forward repetition; 0: no jump launch
constexpr int kSccThreads = 256;

struct SccFlags : SweepFlags {
    // SweepFlags (changed: a forward sweep lowered a colour, a jump moved one, a backward sweep stored a label) and the next
    // two are zeroed in front of every repetition: the first 16 bytes of the workspace
    int removed;            // vertices that this trim pass labelled
    int alive;              // vertices that this trim pass left unassigned
    // zeroed once
    int components;         // vertices with label[v] == v so far: the trimmed ones and the roots
    int pad[3];
};

// P.row_ptr = 0 .. n, label = fill (-1, or v itself for a graph without entries: every vertex is an SCC), no marks
__global__ __launch_bounds__(kSccThreads) void k_scc_init(int n, int *__restrict__ row_ptr, int *__restrict__ label, bool alive,
                                                         int *__restrict__ has_out, int *__restrict__ has_in,
                                                         SccFlags *__restrict__ flags)
{
    const long long r = (long long)blockIdx.x * kSccThreads + threadIdx.x;
    if (r <= n) row_ptr[r] = (int)r;
    if (r < n) {
        label[r] = alive ? -1 : (int)r;
        if (alive) has_out[r] = has_in[r] = 0;
    }
    if (alive && r == 0) *flags = SccFlags{};
}

// The three sweeps: ops of sel_sweep_graph (sel_rows.hpp), which walks the entries, tests the columns and skips self-loops.
// label[] is only read here: the marks are those of the launch boundary
struct SccMark {
    const int *__restrict__ label;
    int *__restrict__ has_out, *__restrict__ has_in;
    bool changed, alive_u;
    __device__ __forceinline__ void row(int u) { alive_u = label[u] < 0; }
    __device__ __forceinline__ void edge(int u, int v)
    {
        if (alive_u && label[v] < 0) {
            has_out[u] = 1;
            has_in[v] = 1;
        }
    }
};

// color is read by plain loads and lowered by atomics in the same launch: neither const nor __restrict__
struct SccForward {
    int *color;
    bool changed;
    int cu;
    __device__ __forceinline__ void row(int u) { cu = color[u]; }
    __device__ __forceinline__ void edge(int, int v)
    {
        if (cu >= 0 && color[v] > cu && atomicMin(&color[v], cu) > cu) changed = true;   // (-1 > cu never holds)
    }
};

// label is read by plain loads and stored in the same launch: neither const nor __restrict__
struct SccBackward {
    const int *__restrict__ color;
    int *label;
    bool changed, open;
    int cu;
    __device__ __forceinline__ void row(int u)
    {
        open = label[u] < 0;                                             // alive, so color[u] >= 0
        cu = color[u];
    }
    __device__ __forceinline__ void edge(int u, int v)
    {
        if (open && color[v] == cu && label[v] >= 0) {
            label[u] = cu;
            open = false;
            changed = true;
        }
    }
};

__global__ __launch_bounds__(kSelThreads) void k_scc_mark(const int *__restrict__ row_ptr, const int *__restrict__ col, int n,
                                                         long long E, bool vec, const int *__restrict__ tile_row,
                                                         const int *__restrict__ label, int *__restrict__ has_out,
                                                         int *__restrict__ has_in, SccFlags *__restrict__ flags)
{
    SccMark op = {label, has_out, has_in, false, false};
    sel_sweep_graph(row_ptr, col, n, E, vec, tile_row, flags, op);
}

__global__ __launch_bounds__(kSelThreads) void k_scc_forward(const int *__restrict__ row_ptr, const int *__restrict__ col, int n,
                                                            long long E, bool vec, const int *__restrict__ tile_row, int *color,
                                                            SccFlags *__restrict__ flags)
{
    SccForward op = {color, false, -1};
    sel_sweep_graph(row_ptr, col, n, E, vec, tile_row, flags, op);
}

__global__ __launch_bounds__(kSelThreads) void k_scc_backward(const int *__restrict__ row_ptr, const int *__restrict__ col, int n,
                                                             long long E, bool vec, const int *__restrict__ tile_row,
                                                             const int *__restrict__ color, int *label,
                                                             SccFlags *__restrict__ flags)
{
    SccBackward op = {color, label, false, false, -1};
    sel_sweep_graph(row_ptr, col, n, E, vec, tile_row, flags, op);
}

// Only thread v touches label[v], color[v] and the marks of v here.
__global__ __launch_bounds__(kSccThreads) void k_scc_trim(int n, int *__restrict__ label, int *__restrict__ color,
                                                         int *__restrict__ has_out, int *__restrict__ has_in, SccFlags *flags)
{
    __shared__ int wsum[kSccThreads / 64];
    const long long v = (long long)blockIdx.x * kSccThreads + threadIdx.x;
    bool removed = false, stays = false;
    if (v < n) {
        if (label[v] < 0) {
            removed = !(has_out[v] && has_in[v]);
            stays = !removed;
            if (removed) label[v] = (int)v;
        }
        color[v] = stays ? (int)v : -1;
        has_out[v] = has_in[v] = 0;
    }
    block_add<kSccThreads>(removed, &flags->removed, &flags->components, wsum);
    block_add<kSccThreads>(stays, &flags->alive, nullptr, wsum);
}

// Only thread v stores color[v] here, and what it stores is an ancestor of v not above the old value: a racing reader sees
// the old or the new one.  A colour is the id of a vertex that was alive when the round began, so color[c] >= 0.
__global__ __launch_bounds__(kSccThreads) void k_scc_jump(int n, int *color, SccFlags *__restrict__ flags)
{
    const long long v = (long long)blockIdx.x * kSccThreads + threadIdx.x;
    bool moved = false;
    if (v < n) {
        const int c0 = color[v];
        if (c0 >= 0) {
            int c = c0;
#pragma unroll
            for (int k = 0; k < kSccJumps; k++) c = color[c];
            if (c != c0) {
                color[v] = c;
                moved = true;
            }
        }
    }
    if (__ballot(moved) && lane_id() == 0) flags->changed = 1u;
}

__global__ __launch_bounds__(kSccThreads) void k_scc_roots(int n, const int *__restrict__ color, int *__restrict__ label,
                                                          SccFlags *flags)
{
    __shared__ int wsum[kSccThreads / 64];
    const long long v = (long long)blockIdx.x * kSccThreads + threadIdx.x;
    const bool root = v < n && color[v] == (int)v;                       // (color >= 0: alive when the round began)
    if (root) label[v] = (int)v;
    block_add<kSccThreads>(root, &flags->components, nullptr, wsum);
}

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_strongly_connected_components(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_matrix **P,
                                                                int *ncomponents, int *rounds, int *sweeps)
{
    static const char who[] = "bspgemm_strongly_connected_components";
    if (P) *P = nullptr;
    if (ncomponents) *ncomponents = 0;
    if (rounds) *rounds = 0;
    if (sweeps) *sweeps = 0;
    if (!ctx || !A || !P) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_strongly_connected_components: NULL argument");
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_SQUARE | NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const int n = A->rows;
    const long long E = A->nnz;
    const bool edges = E > 0;
    const size_t n4 = ws_pad4((size_t)n);
    SccFlags *d_flags = nullptr;
    int *color = nullptr, *has_out = nullptr, *has_in = nullptr;
    auto carve = [&](int *tmp) { return WsCursor(tmp).take(d_flags, 1).take(color, n4).take(has_out, n4).take(has_in, n4).ints(); };
    if (edges) {                                            // (before anything is launched: growing them synchronises)
        if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return st;
        if (bspgemm_status st = ensure_tmp(ctx, carve(nullptr))) return st;
        carve(ctx->tmp);
    }
    // BSPGEMM_SCC_TIMING: host clocks around the repetitions, each of which ends synchronised anyway
    StageClock clk(ctx->scc_timing, s);
    double ms_trim = 0, ms_fwd = 0, ms_bwd = 0;
    bspgemm_matrix *m = nullptr;                            // the assignment operand: its col_idx is label[]
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bspgemm_matrix_free(m); return st; };
    auto stuck = [&]() { return bail(fail_stuck(who)); };
    if (bspgemm_status st = assignment_operand(ctx, n, &m)) return bail(st);
    int *label = m->d_col_idx;
    const dim3 vgrid = vertex_grid(n, kSccThreads), vblock(kSccThreads);
    hipLaunchKernelGGL(k_scc_init, vgrid, vblock, 0, s, n, m->d_row_ptr, label, edges, has_out, has_in, d_flags);
    HIPCHK_B(hipGetLastError());
    SccFlags h = {};
    h.components = n;                                       // without entries every vertex is an SCC
    int r = 0;
    long long trims = 0, fwd = 0, bwd = 0;
    if (edges) {
        launch_select_tile_rows(A->d_row_ptr, n, ctx->tile_row, s);
        const dim3 egrid(select_tiles(E)), eblock(kSelThreads);
        const bool vec = aligned16(A->d_col_idx);
        const long long cap = (long long)n + 2;             // defensive: every repetition but the last changes a vertex
        // a repetition zeroes the block's first four words and ends in the read-back of all of it: its one synchronisation
        auto reset = [&]() { return round_reset(d_flags, 4 * sizeof(int), s); };
        auto fetch = [&]() { return round_fetch(&h, d_flags, sizeof h, s); };
        for (;;) {
            // trim to the fixpoint; the last pass leaves color[] ready for the round
            clk.start();
            for (long long it = 0;; it++) {
                if (it >= cap) return stuck();
                trims++;
                HIPCHK_B(reset());
                hipLaunchKernelGGL(k_scc_mark, egrid, eblock, 0, s, A->d_row_ptr, A->d_col_idx, n, E, vec, ctx->tile_row, label,
                                   has_out, has_in, d_flags);
                hipLaunchKernelGGL(k_scc_trim, vgrid, vblock, 0, s, n, label, color, has_out, has_in, d_flags);
                HIPCHK_B(fetch());
                if (h.bad) return bail(fail_bad_column(who, n));
                if (h.removed == 0 || h.alive == 0) break;
            }
            (void)clk.lap(ms_trim);
            if (h.alive == 0) break;
            if (r >= n) return stuck();                     // (a round labels at least one vertex)
            r++;
            for (long long it = 0;; it++) {
                if (it >= cap) return stuck();
                fwd++;
                HIPCHK_B(reset());
                hipLaunchKernelGGL(k_scc_forward, egrid, eblock, 0, s, A->d_row_ptr, A->d_col_idx, n, E, vec, ctx->tile_row, color,
                                   d_flags);
                if (kSccJumps > 0) hipLaunchKernelGGL(k_scc_jump, vgrid, vblock, 0, s, n, color, d_flags);
                HIPCHK_B(fetch());
                if (!h.changed) break;
            }
            (void)clk.lap(ms_fwd);
            hipLaunchKernelGGL(k_scc_roots, vgrid, vblock, 0, s, n, color, label, d_flags);
            for (long long it = 0;; it++) {
                if (it >= cap) return stuck();
                bwd++;
                HIPCHK_B(reset());
                hipLaunchKernelGGL(k_scc_backward, egrid, eblock, 0, s, A->d_row_ptr, A->d_col_idx, n, E, vec, ctx->tile_row, color,
                                   label, d_flags);
                HIPCHK_B(fetch());
                if (!h.changed) break;
            }
            (void)clk.lap(ms_bwd);
        }
    }
    if (bspgemm_status st = operand_finish(m, n)) return bail(st);   // one label per vertex
    HIPCHK_B(hipStreamSynchronize(s));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: n %d nnz %lld components %d rounds %d | total %.3f ms = %lld trim passes %.3f + %lld forward "
                        "sweeps %.3f + %lld backward sweeps %.3f + rest\n",
                who, n, E, h.components, r, clk.total(), trims, ms_trim, fwd, ms_fwd, bwd, ms_bwd);
    if (ncomponents) *ncomponents = h.components;
    if (rounds) *rounds = r;
    if (sweeps) *sweeps = (int)(trims + fwd + bwd > INT_MAX ? INT_MAX : trims + fwd + bwd);
    *P = m;
    return BSPGEMM_OK;
}
