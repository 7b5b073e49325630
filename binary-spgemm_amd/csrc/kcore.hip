// kcore.hip -- k-core decomposition with a core number per vertex, everything device-resident: bspgemm_core_numbers and,
// composed on top of it from public calls, bspgemm_kcore (include/bspgemm.h).  No product in the decomposition: level-
// synchronous peeling of the simple undirected graph S = bspgemm_matrix_symmetrize(A, DROP_DIAGONAL) (sorted duplicate-free
// rows, no diagonal, every column in [0, n): the transpose inside symmetrize tests them), on three arrays
//     deg[n]    residual degrees, from S.row_ptr                     (workspace)
//     core[n]   -1 = unassigned; the values array of the result that the call returns, so nothing is copied at the end
//     list[2][n] two frontier lists that the peel launches ping-pong  (workspace)
// and a block of four counters.  Level k = 0, 1, ...:
//     k_kcore_scan(k)   per vertex: an unassigned v with deg[v] <= k gets core[v] = k and is appended to list 0 (ballot,
//                       one atomicAdd per wave, lane rank by mbcnt); the minimum deg over the vertices that stay unassigned
//                       is reduced beside it.  No degree changes in this launch, so that minimum is exact.
//     read-back {frontier size, minimum}: an empty frontier jumps k to the minimum and scans again
//     k_kcore_peel(k)   one wave per frontier vertex u, its lanes striding over S's row u: for a neighbour w with
//                       deg[w] > k (plain load), old = atomicSub(&deg[w], 1) at device scope; old == k + 1 gives
//                       core[w] = k and appends w to the OTHER list.  One read-back of that list's size; the lists swap
//                       until it is empty.  Then k + 1.
// Invariants.  After the scan of level k every unassigned vertex has deg > k.  A degree only ever falls, by one per atomic,
// so the atomics on deg[w] return every value from w's degree at the scan downwards exactly once: exactly one of them
// returns k + 1, w is appended exactly once, by that decrement alone, and never also by a scan (it is assigned by then).
// deg[] of an assigned vertex is read by nobody: it may be decremented further or not, the result does not see it.  A
// vertex enters the frontier of level k exactly when its residual degree among the unassigned vertices reaches k or less,
// which is the peeling definition of the core number (Matula & Beck); the numbers are unique, so every run gives the same
// bits.  The ORDER inside a frontier list depends on scheduling and changes nothing: a launch consumes the whole list.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores.  Every decision
// rests on the return value of a device-scope atomic or on a value from before the launch (the list and its size, core[]
// in the scan, S).  The one plain load of a word that the same launch changes is the deg[w] > k filter in front of the
// atomic: a stale value is an older one, so only ever HIGHER than the true one -- a vertex the load lets pass is merely
// decremented by its atomic, whose return value decides; a vertex it skips has deg <= k in truth, is therefore assigned and
// its degree is dead.  The stores to core[] and to the lists are read by the next launch only.  No kernel waits for another
// workgroup: every loop is bounded by the thread's own row or by the list size the host passed in.
//
// Cost.  One synchronisation per scan and per peel launch -- a path of n vertices takes n / 2 peel launches -- which is
// what dominates on anything but a dense core.  Every stored entry of S is walked once, with at most one
// atomic.  A frontier vertex's row is walked by ONE wave, 64 entries per step: a hub in the frontier is a serial tail of
// degree / 64 steps, NOT the "a hub costs what its entries cost" geometry of the entry-parallel passes (select, setop, cc).
// The host caps the loop at n peel launches and 2 n + 2 scans and never spins.
#include "internal.hpp"
#include "wave.hpp"

namespace bsp {

constexpr int kKcThreads = 256;
constexpr int kKcWaves = kKcThreads / 64;

struct KcFlags {
    int size[2];            // entries appended to list 0 / list 1 by the launch that writes it
    int left;               // INT_MAX - (the smallest deg among the vertices the scan leaves unassigned); 0: none left
    int pad;
};

// The frontier lists are appended to by wave_append (wave.hpp).  A vertex is appended once in its life, so a list never
// passes n entries; the store is bounded all the same and the host refuses a size above n.

// deg from S.row_ptr, core = -1, and the result's pattern: row v holds (v, v)
__global__ __launch_bounds__(kKcThreads) void k_kcore_init(int n, const int *__restrict__ rpS, int *__restrict__ deg,
                                                          int *__restrict__ core, long long *__restrict__ row_ptr,
                                                          int *__restrict__ col_idx, int fill)
{
    const long long v = (long long)blockIdx.x * kKcThreads + threadIdx.x;
    if (v <= n) row_ptr[v] = v;
    if (v < n) {
        if (rpS) deg[v] = rpS[v + 1] - rpS[v];
        core[v] = fill;
        col_idx[v] = (int)v;
    }
}

// core[] and deg[] are only read here apart from the one store of the thread's own core[v]
__global__ __launch_bounds__(kKcThreads) void k_kcore_scan(int n, int k, const int *__restrict__ deg, int *__restrict__ core,
                                                          int *__restrict__ list, KcFlags *flags)
{
    __shared__ int wmin[kKcWaves];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long v = (long long)blockIdx.x * kKcThreads + threadIdx.x;
    bool take = false;
    int left = INT_MAX;
    if (v < n && core[v] < 0) {
        const int d = deg[v];
        take = d <= k;
        if (take) core[v] = k;
        else left = d;
    }
    wave_append(take, (int)v, list, &flags->size[0], n, lane);
    left = wave_min(left);
    if (lane == 0) wmin[w] = left;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < kKcWaves; q++) left = min(left, wmin[q]);
        if (left != INT_MAX) atomicMax(&flags->left, INT_MAX - left);
    }
}

// one wave per vertex of `list` (fsize entries, from the host).  deg is loaded plainly and lowered by atomics in the same
// launch: neither const nor __restrict__.  `reset` is the size word of the list being read: the host has it already, and
// the next launch appends to that list.
__global__ __launch_bounds__(kKcThreads) void k_kcore_peel(int n, int k, int fsize, const int *__restrict__ list,
                                                          const int *__restrict__ rpS, const int *__restrict__ colS, int *deg,
                                                          int *__restrict__ core, int *__restrict__ next, int *next_size,
                                                          int *reset)
{
    const int lane = lane_id();
    const long long f = (long long)blockIdx.x * kKcWaves + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *reset = 0;
    if (f >= fsize) return;                                  // (wave-uniform)
    const int u = list[f];
    const int e = rpS[u + 1];
    for (long long b = rpS[u]; b < e; b += 64) {             // (64-bit: e may be INT_MAX)
        bool hit = false;
        int x = 0;
        if (b + lane < e) {
            x = colS[b + lane];                              // in [0, n): S is symmetrize's output
            if (deg[x] > k && atomicSub(&deg[x], 1) == k + 1) {
                core[x] = k;
                hit = true;
            }
        }
        wave_append(hit, x, next, next_size, n, lane);
    }
}

}  // namespace bsp

using namespace bsp;

// The core numbers of A's graph as a counted result, and (S_out) the graph itself: what both entry points share.
// Every column of S is in range and its rows are sorted and duplicate-free, so the kernels need no check of their own.
static bspgemm_status kcore_numbers(bspgemm_context *ctx, const bspgemm_matrix *A, const char *who, bspgemm_matrix **S_out,
                                    bspgemm_result **cores, int *degeneracy, int *rounds)
{
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_SQUARE)) return st;
    // BSPGEMM_KCORE_TIMING: host clocks around the stages; a launch is then synchronised before its read-back is issued, so
    // that the two are told apart
    StageClock clk(ctx->kcore_timing, ctx->stream);
    double ms_sym = 0, ms_scan = 0, ms_peel = 0, ms_back = 0;
    bspgemm_matrix *S = nullptr;
    if (bspgemm_status st = bspgemm_matrix_symmetrize(ctx, A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL, &S)) return st;
    (void)clk.lap(ms_sym, true);
    if (bspgemm_status st = use_device(ctx)) {
        bspgemm_matrix_free(S);
        return st;
    }
    hipStream_t s = ctx->stream;
    const int n = S->rows;
    const bool edges = S->nnz > 0;
    bspgemm_result *R = nullptr;
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_result_free(R);
        bspgemm_matrix_free(S);
        return st;
    };
    auto stuck = [&]() { return bail(fail_stuck(who)); };
    // the counters, deg and the two lists (before anything is launched: growing the workspace synchronises)
    const size_t n4 = ws_pad4((size_t)n);
    KcFlags *d_flags = nullptr;
    int *deg = nullptr, *list[2] = {nullptr, nullptr};
    auto carve = [&](int *tmp) { return WsCursor(tmp).take(d_flags, 1).take(deg, n4).take(list[0], n4).take(list[1], n4).ints(); };
    if (edges) {
        if (bspgemm_status st = ensure_tmp(ctx, carve(nullptr))) return bail(st);
        carve(ctx->tmp);
    }
    // the result, allocated as a product's is: its values are the core array while the levels run
    if (bspgemm_status st = counted_result_new(ctx, n, n, &R)) return bail(st);
    int *core = R->d_values;
    const dim3 vgrid = vertex_grid(n, kKcThreads), block(kKcThreads);
    // without edges every vertex is isolated: core 0, nothing to peel
    hipLaunchKernelGGL(k_kcore_init, vgrid, block, 0, s, n, edges ? S->d_row_ptr : nullptr, deg, core, R->d_row_ptr,
                       R->d_col_idx, edges ? -1 : 0);
    HIPCHK_B(hipGetLastError());
    int k = 0, top = 0, peels = 0;
    long long scans = 0;
    if (edges) {
        long long assigned = 0;
        const long long scan_cap = 2 * (long long)n + 2;    // defensive: at most two scans per distinct core value
        while (assigned < n) {
            if (++scans > scan_cap) return stuck();
            KcFlags h = {};
            HIPCHK_B(round_reset(d_flags, sizeof(KcFlags), s));
            clk.start();
            hipLaunchKernelGGL(k_kcore_scan, vgrid, block, 0, s, n, k, deg, core, list[0], d_flags);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_scan, true));
            HIPCHK_B(hipMemcpyAsync(&h, d_flags, sizeof h, hipMemcpyDeviceToHost, s));
            HIPCHK_B(hipStreamSynchronize(s));
            HIPCHK_B(clk.lap(ms_back));
            int fsize = h.size[0], cur = 0;
            if (fsize == 0) {                               // nobody at this level: on to the smallest degree that is left
                const int least = INT_MAX - h.left;
                if (h.left == 0 || least <= k) return stuck();
                k = least;
                continue;
            }
            top = k;
            while (fsize > 0) {
                if (peels >= n) return stuck();
                peels++;
                assigned += fsize;
                const dim3 pgrid((unsigned)(((long long)fsize + kKcWaves - 1) / kKcWaves));
                clk.start();
                hipLaunchKernelGGL(k_kcore_peel, pgrid, block, 0, s, n, k, fsize, list[cur], S->d_row_ptr, S->d_col_idx, deg, core,
                                   list[cur ^ 1], &d_flags->size[cur ^ 1], &d_flags->size[cur]);
                HIPCHK_B(hipGetLastError());
                HIPCHK_B(clk.lap(ms_peel, true));
                clk.longest(clk.last, k, fsize);
                HIPCHK_B(hipMemcpyAsync(&fsize, &d_flags->size[cur ^ 1], sizeof fsize, hipMemcpyDeviceToHost, s));
                HIPCHK_B(hipStreamSynchronize(s));          // the launch's one synchronisation
                HIPCHK_B(clk.lap(ms_back));
                if (fsize < 0 || fsize > n) return stuck();
                cur ^= 1;
            }
            k++;
        }
    }
    HIPCHK_B(hipStreamSynchronize(s));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: n %d nnz(S) %lld degeneracy %d | total %.3f ms = symmetrize %.3f + %lld scans %.3f + %d peel "
                        "launches %.3f + read-backs %.3f + rest | longest peel launch %.3f ms (level %d, %d frontier vertices)\n",
                who, n, (long long)S->nnz, top, clk.total(), ms_sym, scans, ms_scan, peels, ms_peel, ms_back, clk.max_ms,
                clk.max_tag[0], clk.max_tag[1]);
    if (degeneracy) *degeneracy = top;
    if (rounds) *rounds = peels;
    *cores = R;
    *S_out = S;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_core_numbers(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_result **cores,
                                               int *degeneracy, int *rounds)
{
    if (cores) *cores = nullptr;
    if (degeneracy) *degeneracy = 0;
    if (rounds) *rounds = 0;
    if (!ctx || !A || !cores) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_core_numbers: NULL argument");
    bspgemm_matrix *S = nullptr;
    bspgemm_status st = kcore_numbers(ctx, A, "bspgemm_core_numbers", &S, cores, degeneracy, rounds);
    bspgemm_matrix_free(S);
    return st;
}

// T = D_k * S * D_k, D_k the diagonal selector of {v : core(v) >= k}
extern "C" bspgemm_status bspgemm_kcore(bspgemm_context *ctx, const bspgemm_matrix *A, int k, bspgemm_matrix **T, int *degeneracy)
{
    if (T) *T = nullptr;
    if (degeneracy) *degeneracy = 0;
    if (!ctx || !A || !T) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_kcore: NULL argument");
    if (k < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_kcore: k < 0");
    bspgemm_matrix *S = nullptr, *D = nullptr, *DSm = nullptr;
    bspgemm_result *cores = nullptr, *DS = nullptr, *DSD = nullptr;
    int top = 0;
    bspgemm_status st = kcore_numbers(ctx, A, "bspgemm_kcore", &S, &cores, &top, nullptr);
    if (st) return st;
    const int n = S->rows;
    if (k == 0) {                                           // every vertex: the graph itself
        *T = S;
        S = nullptr;
    } else if (k > top) {                                   // nobody: D_k is the empty n x n operand, no product
        st = bspgemm_matrix_from_result_where(ctx, cores, n, BSPGEMM_CMP_GE, k, T);
    } else {
        st = bspgemm_matrix_from_result_where(ctx, cores, n, BSPGEMM_CMP_GE, k, &D);
        if (!st) st = bspgemm_multiply(ctx, D, S, 0, n, &DS);
        if (!st) st = bspgemm_matrix_from_result(ctx, DS, n, &DSm);
        if (!st) st = bspgemm_multiply(ctx, DSm, D, 0, n, &DSD);
        if (!st) st = bspgemm_matrix_from_result(ctx, DSD, n, T);
    }
    bspgemm_result_free(DSD);
    bspgemm_matrix_free(DSm);
    bspgemm_result_free(DS);
    bspgemm_matrix_free(D);
    bspgemm_result_free(cores);
    bspgemm_matrix_free(S);
    if (st) return st;
    if (degeneracy) *degeneracy = top;
    return BSPGEMM_OK;
}
