// bfs.hip -- multi-source breadth-first search with a level per reached vertex, everything device-resident: bspgemm_bfs
// (include/bspgemm.h).  The loop is the one the complemented mask was built for,
//     V0 = F0 = one entry (s, sources[s]) per row, level 0
//     level d:  N = !V .* (F * A)      the complement product: what the frontier reaches and V does not hold yet
//               Nm = N as an operand   bspgemm_matrix_from_result: the next frontier
//               V' = V u Nm            the merge below; the entries of Nm get the value d
// and it ends when a frontier comes back empty, when V holds every vertex in every row, or at the depth cap.
//
// The merge is setop.hip's OR for two operands that are canonical (rows strictly ascending) and DISJOINT, with a value per
// entry -- both hold by construction here, V and N are products and N is masked by !V.  Then nothing of the general union
// is needed: no common entries means no flag words, no scan and no read-back (the size is |V| + |N| before anything runs),
// and an entry's place p + lb (DESIGN.md 4.11 with c = 0: p counts the entries of its own operand before it, lb those of the
// other operand in earlier rows and the smaller ones of its row) is used where it is computed instead of being stored.
//   k_merge_disjoint   once per side X against the other side Y, in select's geometry (sel_rows.hpp): a workgroup owns
//                      kSelTile consecutive entries of X whatever rows they belong to, a lane four of them (one 16-byte
//                      load of the columns, one of the values), the tile's window of X.row_ptr is staged in LDS.  Each
//                      column is binary-searched in Y's row, a lane's next entry of the same row from the previous lower
//                      bound on; column and value (V side: the entry's own, N side: the constant d) go to p + lb.
//                      4 + 4 bytes read and 4 + 4 written per entry of V, 4 read and 8 written per entry of N, and the
//                      probes of the searches, which stay in L2: neighbouring entries walk the same Y row.
//   k_merge_row_ptr    row_ptr'[r] = rpV[r] + rpN[r]: O(1) per row, int32 (V' is the next product's mask)
//   k_widen_row_ptr    int32 -> int64, once, for the result object
// BSPGEMM_OPT_CHECK: the kernel also tests whether a search hit its column and ORs a bit into a device word, which the host
// then reads (one synchronisation per level, under the option only).
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

// One side of the merge as an op of sel_walk_entries (sel_rows.hpp).  VALS: the entries' values come from valsX (the V
// side), else every entry gets `level` (the N side).  X's columns and values are read once (non-temporal); Y's columns are
// probed by many lanes and stay temporal.  The destinations p + lb < E + nnz(Y) for consistent row_ptrs: lb <= rpY[rows] =
// nnz(Y).
template <bool VALS, bool CHECK>
struct MergeDisjoint {
    const int *__restrict__ valsX, *__restrict__ rpY, *__restrict__ colY;
    int *__restrict__ out_col, *__restrict__ out_val;
    int level;
    long long E;
    bool vecv, common;
    int from, yend;                                                      // what is left of Y's row: X ascends, so does lb
    v4i x[kSelSteps];
    __device__ __forceinline__ void load(int j, long long e)
    {
        if (VALS) x[j] = load4<true>(valsX, e, E, vecv);
    }
    __device__ __forceinline__ void row(int r)
    {
        from = rpY[r];
        yend = rpY[r + 1];
    }
    __device__ __forceinline__ void entry(int, long long p, int c, int s)
    {
        from = sel_lower_bound(colY, from, yend, c);                     // (an empty row of Y: nothing is read)
        if (CHECK && from < yend && colY[from] == c) common = true;
        const long long dst = p + from;
        out_col[dst] = c;
        out_val[dst] = VALS ? x[s >> 2][s & 3] : level;
    }
};

template <bool VALS, bool CHECK>
__global__ __launch_bounds__(kSelThreads) void k_merge_disjoint(const int *__restrict__ rpX, const int *__restrict__ colX,
                                                               const int *__restrict__ valsX, int level, int rows, long long E,
                                                               bool vec, bool vecv, const int *__restrict__ tile_row,
                                                               const int *__restrict__ rpY, const int *__restrict__ colY,
                                                               int *__restrict__ out_col, int *__restrict__ out_val,
                                                               unsigned *__restrict__ hit)
{
    MergeDisjoint<VALS, CHECK> op = {valsX, rpY, colY, out_col, out_val, level, E, vecv, false, 0, 0, {}};
    sel_walk_entries<true>(rpX, colX, rows, E, vec, tile_row, op);
    if (CHECK && op.common) atomicOr(hit, 1u);
}

__global__ __launch_bounds__(256) void k_merge_row_ptr(const int *__restrict__ rpV, const int *__restrict__ rpN, int rows,
                                                      int *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= rows) out[r] = rpV[r] + rpN[r];
}

__global__ __launch_bounds__(256) void k_widen_row_ptr(const int *__restrict__ src, int n, long long *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// V0: row s holds sources[s] alone -- row_ptr = 0 .. rows
__global__ __launch_bounds__(256) void k_bfs_unit_row_ptr(int rows, int *__restrict__ row_ptr)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= rows) row_ptr[r] = r;
}

// one side of the merge: the nnzX > 0 entries of X (vals: their values, or NULL for the constant `level`) to their places
// in out_col / out_val.  tile_row: nnzX / kSelTile + 1 ints of scratch; hit: NULL, or the device word of the check.
static void launch_merge_side(const int *rpX, const int *colX, const int *vals, int level, int rows, long long nnzX,
                              const int *rpY, const int *colY, int *tile_row, int *out_col, int *out_val, unsigned *hit,
                              hipStream_t s)
{
    if (nnzX <= 0) return;
    launch_select_tile_rows(rpX, rows, tile_row, s);
    const dim3 grid(select_tiles(nnzX)), block(kSelThreads);
    const bool vec = aligned16(colX), vecv = vals && aligned16(vals);
#define BSP_MERGE(VALS, CHECK)                                                                                            \
    hipLaunchKernelGGL((k_merge_disjoint<VALS, CHECK>), grid, block, 0, s, rpX, colX, vals, level, rows, nnzX, vec, vecv, \
                       tile_row, rpY, colY, out_col, out_val, hit)
    if (vals) {
        if (hit) BSP_MERGE(true, true);
        else BSP_MERGE(true, false);
    } else {
        if (hit) BSP_MERGE(false, true);
        else BSP_MERGE(false, false);
    }
#undef BSP_MERGE
}

}  // namespace bsp

using namespace bsp;

// ------------------------------------------------------------------ the host side --------
// The visited set while the loop runs: an int32 operand (the next product's mask) and a level per entry.  Its arrays come
// from the context's result cache, like a product's, because the last V becomes the result object as it stands; the handle
// does not own them.  That is why it is not built by operand_new / operand_cols (internal.hpp): those hipMalloc arrays
// that bspgemm_matrix_free frees, these go back to the cache (bfs_release) or on into the result, with a third array
// (the levels) that an operand does not have.
struct BfsVisited {
    bspgemm_matrix *m = nullptr;
    int *vals = nullptr;
};

static inline size_t bfs_bytes_rowptr32(int rows) { return ((size_t)rows + 1) * sizeof(int); }

static void bfs_release(bspgemm_context *ctx, BfsVisited *V)
{
    if (!V->m) return;
    result_release(ctx, V->m->d_row_ptr, bfs_bytes_rowptr32(V->m->rows));
    result_release(ctx, V->m->d_col_idx, result_bytes_colidx(V->m->nnz));
    result_release(ctx, V->vals, result_bytes_colidx(V->m->nnz));
    bspgemm_matrix_free(V->m);                              // (not owned: the handle and its derived tables)
    V->m = nullptr;
    V->vals = nullptr;
}

// the arrays of a visited set of `nnz` entries, nothing written yet
static bspgemm_status bfs_alloc(bspgemm_context *ctx, int rows, int cols, long long nnz, BfsVisited *V)
{
    V->m = new (std::nothrow) bspgemm_matrix{ctx, rows, cols, nnz, nullptr, nullptr, false};
    if (!V->m) return FAIL(BSPGEMM_ERR_ALLOC, "matrix");
    auto bail = [&](bspgemm_status st) { bfs_release(ctx, V); return st; };
    HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&V->m->d_row_ptr), bfs_bytes_rowptr32(rows)));
    HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&V->m->d_col_idx), result_bytes_colidx(nnz)));
    HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&V->vals), result_bytes_colidx(nnz)));
    return BSPGEMM_OK;
}

// out = V u N with the level `level` on N's entries; V and N canonical and disjoint.  No synchronisation unless the
// context checks (BSPGEMM_OPT_CHECK).
static bspgemm_status bfs_merge(bspgemm_context *ctx, const BfsVisited &V, const bspgemm_matrix *N, int level, BfsVisited *out)
{
    hipStream_t s = ctx->stream;
    const int rows = V.m->rows;
    const long long EV = V.m->nnz, EN = N->nnz;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)(EV > EN ? EV : EN))) return st;
    unsigned *d_hit = nullptr;
    if (ctx->check) {
        if (bspgemm_status st = ensure_tmp(ctx, 4)) return st;
        d_hit = reinterpret_cast<unsigned *>(ctx->tmp);
        HIPCHK(hipMemsetAsync(d_hit, 0, sizeof(unsigned), s));
    }
    if (bspgemm_status st = bfs_alloc(ctx, rows, V.m->cols, EV + EN, out)) return st;
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bfs_release(ctx, out); return st; };
    // the two sides' launches follow each other on the stream, so they share tile_row
    launch_merge_side(V.m->d_row_ptr, V.m->d_col_idx, V.vals, 0, rows, EV, N->d_row_ptr, N->d_col_idx, ctx->tile_row,
                      out->m->d_col_idx, out->vals, d_hit, s);
    launch_merge_side(N->d_row_ptr, N->d_col_idx, nullptr, level, rows, EN, V.m->d_row_ptr, V.m->d_col_idx, ctx->tile_row,
                      out->m->d_col_idx, out->vals, d_hit, s);
    hipLaunchKernelGGL(k_merge_row_ptr, row_pass_grid(rows), dim3(256), 0, s, V.m->d_row_ptr, N->d_row_ptr, rows, out->m->d_row_ptr);
    HIPCHK_B(hipGetLastError());
    if (d_hit) {
        unsigned hit = 0;
        HIPCHK_B(hipMemcpyAsync(&hit, d_hit, sizeof hit, hipMemcpyDeviceToHost, s));
        HIPCHK_B(hipStreamSynchronize(s));
        if (hit) return bail(FAIL(BSPGEMM_ERR_HIP, "bspgemm_bfs: the new frontier holds a vertex of the visited set"));
    }
    if (bspgemm_status st = ensure_deg8(out->m)) return bail(st);
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_bfs(bspgemm_context *ctx, const bspgemm_matrix *A, int nsources, const int *sources,
                                      int max_depth, bspgemm_result **levels, int *depth, int *complete)
{
    if (levels) *levels = nullptr;
    if (depth) *depth = 0;
    if (complete) *complete = 0;
    if (!ctx || !A || !sources || !levels) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_bfs: NULL argument");
    if (nsources < 1) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_bfs: nsources < 1");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_bfs", NEED_SQUARE)) return st;
    const int n = A->rows, S = nsources;
    for (int i = 0; i < S; i++)
        if (sources[i] < 0 || sources[i] >= n) {
            snprintf(g_err, sizeof g_err, "bspgemm_bfs: sources[%d] = %d is outside [0, %d)", i, sources[i], n);
            return BSPGEMM_ERR_INVALID;
        }
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const long long full = (long long)S * n;                // nnz(V) when every source has reached every vertex

    BfsVisited V;
    if (bspgemm_status st = bfs_alloc(ctx, S, n, S, &V)) return st;
    bspgemm_matrix *Fown = nullptr;                         // the frontier of levels >= 1 (level 0: V0 itself)
    bspgemm_result *R = nullptr;                            // the result object, made at the end: shares V's columns and values
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        if (R) result_release(ctx, R->d_row_ptr, result_bytes_rowptr(S));
        delete R;
        bspgemm_matrix_free(Fown);
        bfs_release(ctx, &V);
        return st;
    };
    hipLaunchKernelGGL(k_bfs_unit_row_ptr, row_pass_grid(S), dim3(256), 0, s, S, V.m->d_row_ptr);
    HIPCHK_B(hipGetLastError());
    HIPCHK_B(hipMemcpyAsync(V.m->d_col_idx, sources, (size_t)S * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_B(hipMemsetAsync(V.vals, 0, (size_t)S * sizeof(int), s));
    if (bspgemm_status st = ensure_deg8(V.m)) return bail(st);
    HIPCHK_B(hipStreamSynchronize(s));                      // `sources` is the caller's again

    int d = 0, done = V.m->nnz == full;
    while (!done) {
        const bspgemm_matrix *F = Fown ? Fown : V.m;
        bspgemm_result *N = nullptr;
        bspgemm_matrix *Nm = nullptr;
        if (bspgemm_status st = bspgemm_multiply_masked_ex(ctx, F, A, V.m, BSPGEMM_MASK_COMPLEMENT, 0, S, &N)) return bail(st);
        if (N->nnz == 0) {                                  // nothing new: the search ended by itself
            bspgemm_result_free(N);
            done = 1;
            break;
        }
        if (V.m->nnz + N->nnz > INT_MAX) {
            snprintf(g_err, sizeof g_err, "bspgemm_bfs: %lld reached entries at level %d: more than INT_MAX, not usable as an int32 operand",
                     V.m->nnz + N->nnz, d + 1);
            bspgemm_result_free(N);
            return bail(BSPGEMM_ERR_OVERFLOW);
        }
        bspgemm_status st = bspgemm_matrix_from_result(ctx, N, n, &Nm);
        bspgemm_result_free(N);
        if (st) return bail(st);
        BfsVisited next;
        st = bfs_merge(ctx, V, Nm, d + 1, &next);
        if (st) {
            bspgemm_matrix_free(Nm);
            return bail(st);
        }
        bspgemm_matrix_free(Fown);
        Fown = Nm;
        bfs_release(ctx, &V);
        V = next;
        d++;
        if (V.m->nnz == full) done = 1;                     // every vertex in every row: no further product
        else if (max_depth > 0 && d >= max_depth) break;
    }

    // the last V is the result: its columns and values as they are, its row_ptr widened
    R = new (std::nothrow) bspgemm_result{ctx, S, V.m->nnz, nullptr, V.m->d_col_idx, V.m->nnz};
    if (!R) return bail(FAIL(BSPGEMM_ERR_ALLOC, "result"));
    HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&R->d_row_ptr), result_bytes_rowptr(S)));
    R->d_values = V.vals;
    hipLaunchKernelGGL(k_widen_row_ptr, row_pass_grid(S), dim3(256), 0, s, V.m->d_row_ptr, S + 1, R->d_row_ptr);
    HIPCHK_B(hipGetLastError());
    result_release(ctx, V.m->d_row_ptr, bfs_bytes_rowptr32(S));   // (stream-ordered behind the widening, like any freed result)
    bspgemm_matrix_free(V.m);
    bspgemm_matrix_free(Fown);
    if (depth) *depth = d;
    if (complete) *complete = done;
    *levels = R;
    return BSPGEMM_OK;
}
