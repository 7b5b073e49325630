// dot.hip -- the masked dot product with counts, C = F .* (A * B^T), on the device: bspgemm_multiply_masked_dot, and the two
// loops with a method argument on top of it, bspgemm_triangle_count_ex and bspgemm_ktruss_ex (include/bspgemm.h).
//
// The counting product (bspgemm_multiply_masked_count) is row-wise Gustavson: it expands every product of a row and keeps
// those that land on a mask column, so its cost follows the product count whatever the mask admits.  Here every mask entry
// (i, j) gets ONE intersection of two sorted rows, |A_i n B_j|: the cost follows the mask, sum over (i, j) in F of
// min(|A_i|, |B_j|) searches of log max(|A_i|, |B_j|) steps, and B's rows are read as they are -- no transpose when the
// caller holds the rows to intersect (L with L for triangles, a symmetric S with itself for the k-truss).
//
// For operands whose rows are strictly ascending ("canonical"; k_set_flags<false> of setop.hip checks that form and the
// columns' range of each distinct handle into one error word):
//   k_dot_count   entry-parallel over F in select's geometry (sel_rows.hpp: a workgroup owns kSelTile consecutive mask
//                 entries whatever rows they belong to, a lane four per 16-byte load).  Entry p = (i, j): the two row
//                 extents; j >= B.rows (tested unsigned, before it indexes B.row_ptr) or m = min(|A_i|, |B_j|) == 0 gives
//                 vals[p] = 0.  LIGHT, m <= T: the lane walks the shorter row and searches the longer one from a lower
//                 bound that only advances (isect_lane); vals[p] = the hits.  HEAVY, m > T: the lane writes nothing and
//                 notes the entry; when the walk is over the wave appends its heavy entries {p, i} to a list
//                 (IsectHeavy: ballot, one atomicAdd per wave, rank by popcount).
//   k_dot_heavy   a fixed grid, one wave per list entry, striding over the list; its length is read from device memory (the
//                 launch follows k_dot_count on the stream, nothing in between: IsectHeavyList).  The lanes stride over
//                 the shorter row 64 elements per step, kIsectDeep steps in flight; each lane searches the longer row
//                 from its own advancing lower bound (isect_wave), the wave adds the popcount of the hit ballot, lane 0
//                 stores vals[p].
// The intersections, the list and their constants are sel_rows.hpp's, shared with lcc.hip; what a hit is worth (here: one)
// is written at the call.
//   filter        vals > 0: select's value flags, scan and scatter (F's columns, then vals), and k_dot_row_ptr for the
//                 int64 row_ptr of the result.
// The one synchronisation reads the error word, the heavy count and the kept count.  An operand that the check found not
// canonical is replaced by operand_canonical and the passes run again; a column out of range fails the call.
//
// Visibility.  Every kernel reads only what an EARLIER launch on the same stream wrote (the list and its length, vals, the
// flag words) or what was there before the call.  The one atomic, the list's append counter, is a device-scope atomicAdd
// whose return value places the entry.  The ORDER of the list depends on scheduling; nothing else does: a value is stored
// by its position p.  No kernel waits for another workgroup; every loop is bounded by a row's length or the list's.
//
// Cost.  A light entry is a serial walk of at most T searches by one lane.  A heavy entry is walked by ONE wave: a hub-hub
// mask entry is a serial tail of m / 64 steps of log-deep searches, NOT the "an entry costs what an entry costs" geometry
// of the count pass.  Splitting one entry across waves is not done.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

struct DotCounters {
    unsigned err;           // the canonical checks: two bits per operand (kSetErrRange, kSetErrOrder), A / B / F
    int heavy;              // entries appended to the heavy list
    int pad[2];
};

// The count as an op of sel_walk_entries.  A's and B's columns are only compared, never used as an index; F's column is
// tested unsigned against B.rows before it indexes B.row_ptr.
struct DotCount {
    const int *__restrict__ rpA, *__restrict__ colA, *__restrict__ rpB, *__restrict__ colB;
    int brows, T;
    int *__restrict__ vals;
    int a0, alen;                       // the extent of A's row of the mask row the lane is in
    IsectHeavy heavy;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int r)
    {
        a0 = rpA[r];
        alen = rpA[r + 1] - a0;
    }
    __device__ __forceinline__ void entry(int r, long long p, int j, int s)
    {
        int count = 0;
        if ((unsigned)j < (unsigned)brows) {                 // before j indexes anything
            const int b0 = rpB[j], blen = rpB[j + 1] - b0;
            const bool a_short = alen <= blen;
            const int m = a_short ? alen : blen;
            if (m > T) {                                     // heavy: k_dot_heavy stores vals[p]
                heavy.note(s, r);
                return;
            }
            const int *__restrict__ x = a_short ? colA + a0 : colB + b0;     // walked
            const int *__restrict__ y = a_short ? colB + b0 : colA + a0;     // searched
            isect_lane(x, m, y, a_short ? blen : alen, [&](bool hit, int, int, int) { count += hit ? 1 : 0; });
        }
        vals[p] = count;
    }
};

__global__ __launch_bounds__(kSelThreads) void k_dot_count(const int *__restrict__ rpF, const int *__restrict__ colF, int rows,
                                                          long long E, bool vec, const int *__restrict__ tile_row,
                                                          const int *__restrict__ rpA, const int *__restrict__ colA,
                                                          const int *__restrict__ rpB, const int *__restrict__ colB, int brows,
                                                          int T, int *__restrict__ vals, int2 *__restrict__ list, int *nheavy)
{
    DotCount op = {rpA, colA, rpB, colB, brows, T, vals, 0, 0, {0u, {}}};
    sel_walk_entries<false>(rpF, colF, rows, E, vec, tile_row, op);      // (F's columns are read again by the scatter)
    op.heavy.append(list, nheavy, E);
}

// one wave per entry of `list`, striding over it
__global__ __launch_bounds__(kSelThreads) void k_dot_heavy(const int *__restrict__ colF, const int *__restrict__ rpA,
                                                          const int *__restrict__ colA, const int *__restrict__ rpB,
                                                          const int *__restrict__ colB, int rows, int brows,
                                                          const int2 *__restrict__ list, const int *__restrict__ nheavy,
                                                          long long cap, int *__restrict__ vals)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const IsectHeavyList hl(list, nheavy, cap, rows);
    for (long long h = (long long)blockIdx.x * kIsectWaves + w; h < hl.n; h += (long long)gridDim.x * kIsectWaves) {   // (wave-uniform)
        int p, i;
        if (!hl.entry(h, p, i)) continue;
        const int j = wave_first(colF[p]);
        int total = 0;
        if ((unsigned)j < (unsigned)brows) {
            const int a0 = rpA[i], alen = rpA[i + 1] - a0, b0 = rpB[j], blen = rpB[j + 1] - b0;
            const bool a_short = alen <= blen;
            const int *__restrict__ x = a_short ? colA + a0 : colB + b0;     // strided over
            const int *__restrict__ y = a_short ? colB + b0 : colA + a0;     // searched
            isect_wave<kIsectDeep>(x, a_short ? alen : blen, y, a_short ? blen : alen, lane,
                                   [&](bool hit, int, int, int) { total += __popcll(__ballot(hit)); });
        }
        if (lane == 0) vals[p] = total;
    }
}

// the result's int64 row_ptr from F's int32 one and the kept flags (k_sel_row_ptr of select.hip writes an operand's int32)
__global__ __launch_bounds__(256) void k_dot_row_ptr(const int *__restrict__ rp, int rows, long long E, long long words,
                                                    const u64 *__restrict__ flags, const long long *__restrict__ pre,
                                                    long long *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    const long long p = rp[r];
    out[r] = p >= E ? pre[words] : pre[p >> 6] + __popcll(flags[p >> 6] & mask_lt((int)(p & 63)));
}

}  // namespace bsp

using namespace bsp;

// ------------------------------------------------------------------ the host side --------
static const char kDotWho[] = "bspgemm_multiply_masked_dot";

// The arguments are checked by the caller.  canonical: the operands are known to have strictly ascending rows (the second
// round); bits: the `canonicalised` word so far.
static bspgemm_status dot_run(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, const bspgemm_matrix *F,
                              bspgemm_result **out, bspgemm_dot_info *info, int bits, bool canonical)
{
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const long long E = F->nnz;
    const int rows = A->rows;
    const int T = ctx->dot_light;
    // the workspace: the counters, vals (whole tiles), the heavy list {p, row} and the flag scratch of the filter
    DotCounters *d_cnt = nullptr;
    int *vals = nullptr;
    int2 *list = nullptr;
    FlagScratch sc;
    auto carve = [&](int *tmp) {
        WsCursor c(tmp);
        c.take(d_cnt, 1).take(vals, 64 * select_words(E)).take(list, (size_t)E);
        return flag_scratch_carve(tmp, c.aligned(), E, false, tmp ? &sc : nullptr);
    };
    const size_t total = carve(nullptr);
    if (!total) return FAIL(BSPGEMM_ERR_OVERFLOW, "bspgemm_multiply_masked_dot: too many mask entries for the word scan");
    if (bspgemm_status st = ensure_tmp(ctx, total)) return st;
    const long long Emax = std::max(E, std::max(A->nnz, B->nnz));
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)Emax)) return st;
    carve(ctx->tmp);

    // every distinct handle is checked once, under the bits of the first role it plays; the kernels follow each other on
    // the stream, so they share tile_row, and F's comes last: k_dot_count walks F
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(DotCounters), s));
    launch_canonical_check(A->d_row_ptr, A->d_col_idx, A->rows, A->cols, A->nnz, 0, ctx->tile_row, &d_cnt->err, s);
    if (B != A) launch_canonical_check(B->d_row_ptr, B->d_col_idx, B->rows, B->cols, B->nnz, 2, ctx->tile_row, &d_cnt->err, s);
    if (F != A && F != B) launch_canonical_check(F->d_row_ptr, F->d_col_idx, F->rows, F->cols, E, 4, ctx->tile_row, &d_cnt->err, s);
    if (E > 0) {
        launch_select_tile_rows(F->d_row_ptr, F->rows, ctx->tile_row, s);
        hipLaunchKernelGGL(k_dot_count, dim3(select_tiles(E)), dim3(kSelThreads), 0, s, F->d_row_ptr, F->d_col_idx, F->rows, E,
                           aligned16(F->d_col_idx), ctx->tile_row, A->d_row_ptr, A->d_col_idx, B->d_row_ptr, B->d_col_idx, B->rows,
                           T, vals, list, &d_cnt->heavy);
        hipLaunchKernelGGL(k_dot_heavy, dim3(kIsectHeavyGrid), dim3(kSelThreads), 0, s, F->d_col_idx, A->d_row_ptr, A->d_col_idx,
                           B->d_row_ptr, B->d_col_idx, rows, B->rows, list, &d_cnt->heavy, E, vals);
        launch_select_flags_value(vals, E, BSPGEMM_CMP_GT, 0, sc.flags, sc.cnt, s);
        launch_scan_counts(sc.cnt, sc.words, sc.pre, sc.part, nullptr, s);
    }
    HIPCHK(hipGetLastError());
    DotCounters h = {};
    long long kept = 0;
    if (E > 0) HIPCHK(hipMemcpyAsync(&kept, sc.pre + sc.words, sizeof kept, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                                          // the call's one synchronisation

    const unsigned range = kSetErrRange | (kSetErrRange << 2) | (kSetErrRange << 4);
    const unsigned order = kSetErrOrder | (kSetErrOrder << 2) | (kSetErrOrder << 4);
    if (h.err & range) {
        const bspgemm_matrix *X = (h.err & kSetErrRange) ? A : (h.err & (kSetErrRange << 2)) ? B : F;
        snprintf(g_err, sizeof g_err, "%s: a column index outside [0, %d) in operand %s", kDotWho, X->cols,
                 X == A ? "A" : X == B ? "B" : "F");
        return BSPGEMM_ERR_INVALID;
    }
    if (h.err & order) {
        if (canonical) return FAIL(BSPGEMM_ERR_HIP, "bspgemm_multiply_masked_dot: a transposed operand is not in ascending order");
        // what the passes left is discarded: the operands whose rows are unsorted or hold repeats are transposed twice
        const bool bad_a = h.err & kSetErrOrder, bad_b = B == A ? bad_a : (h.err & (kSetErrOrder << 2)) != 0;
        const bool bad_f = F == A ? bad_a : F == B ? bad_b : (h.err & (kSetErrOrder << 4)) != 0;
        bspgemm_matrix *ca = nullptr, *cb = nullptr, *cf = nullptr;
        bspgemm_status st = BSPGEMM_OK;
        if (bad_a) st = operand_canonical(ctx, A, &ca);
        if (!st && bad_b && B != A) st = operand_canonical(ctx, B, &cb);
        if (!st && bad_f && F != A && F != B) st = operand_canonical(ctx, F, &cf);
        const bspgemm_matrix *a2 = ca ? ca : A, *b2 = B == A ? a2 : (cb ? cb : B);
        const bspgemm_matrix *f2 = F == A ? a2 : F == B ? b2 : (cf ? cf : F);
        if (!st) st = dot_run(ctx, a2, b2, f2, out, info, bits | (bad_a ? 1 : 0) | (bad_b ? 2 : 0) | (bad_f ? 4 : 0), true);
        bspgemm_matrix_free(cf);
        bspgemm_matrix_free(cb);
        bspgemm_matrix_free(ca);
        return st;
    }
    if (h.heavy < 0 || h.heavy > E || kept < 0 || kept > E) return FAIL(BSPGEMM_ERR_HIP, "bspgemm_multiply_masked_dot: counters out of range");

    // the result object: an ordinary counted result, allocated the way a product's is
    bspgemm_result *R = nullptr;
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bspgemm_result_free(R); return st; };
    if (bspgemm_status st = counted_result_new(ctx, rows, kept, &R)) return bail(st);
    if (E > 0) {
        launch_select_scatter(F->d_col_idx, E, sc.flags, sc.pre, R->d_col_idx, s);
        launch_select_scatter(vals, E, sc.flags, sc.pre, R->d_values, s);
        hipLaunchKernelGGL(k_dot_row_ptr, row_pass_grid(rows), dim3(256), 0, s, F->d_row_ptr, rows, E, (long long)sc.words,
                           sc.flags, sc.pre, R->d_row_ptr);
    } else {
        HIPCHK_B(hipMemsetAsync(R->d_row_ptr, 0, result_bytes_rowptr(rows), s));
    }
    HIPCHK_B(hipGetLastError());
    if (info) {
        info->entries = E;
        info->heavy_entries = h.heavy;
        info->kept = kept;
        info->canonicalised = bits;
    }
    *out = R;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_multiply_masked_dot(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                                      const bspgemm_matrix *F, unsigned flags, bspgemm_result **C,
                                                      bspgemm_dot_info *info)
{
    if (C) *C = nullptr;
    if (info) *info = bspgemm_dot_info{0, 0, 0, 0};
    if (!ctx || !A || !B || !F || !C) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_multiply_masked_dot: NULL argument");
    if (flags != 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_multiply_masked_dot: flags must be 0 (reserved)");
    if (bspgemm_status st = check_operand(ctx, A, kDotWho, 0)) return st;
    if (bspgemm_status st = check_operand(ctx, B, kDotWho, 0)) return st;
    if (bspgemm_status st = check_operand(ctx, F, kDotWho, 0)) return st;
    if (A->cols != B->cols) {
        snprintf(g_err, sizeof g_err, "%s: A.cols (%d) != B.cols (%d): rows of different widths are not intersected", kDotWho,
                 A->cols, B->cols);
        return BSPGEMM_ERR_INVALID;
    }
    if (F->rows != A->rows) {
        snprintf(g_err, sizeof g_err, "%s: F.rows (%d) != A.rows (%d)", kDotWho, F->rows, A->rows);
        return BSPGEMM_ERR_INVALID;
    }
    if (bspgemm_status st = check_operand(ctx, A, kDotWho, NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = check_operand(ctx, B, kDotWho, NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = check_operand(ctx, F, kDotWho, NEED_ENTRIES_CONSISTENT)) return st;
    return dot_run(ctx, A, B, F, C, info, 0, false);
}

// ------------------------------------------------------------------ triangles, k-truss ---
extern "C" bspgemm_status bspgemm_triangle_count_ex(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_support_method method,
                                                    int64_t *triangles)
{
    if (method == BSPGEMM_SUPPORT_PRODUCT) return bspgemm_triangle_count(ctx, A, triangles);
    if (method != BSPGEMM_SUPPORT_DOT) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_triangle_count_ex: unknown method");
    if (!ctx || !A || !triangles) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_triangle_count_ex: NULL argument");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_triangle_count_ex", NEED_SQUARE)) return st;
    // a triangle i > j > k is the entry (i, j) of L together with k in L_i n L_j: rows of L against rows of L, no transpose
    bspgemm_matrix *L = nullptr;
    bspgemm_result *C = nullptr;
    int64_t sum = 0;
    bspgemm_status st = select_dedup(ctx, A, BSPGEMM_SELECT_TRIL, &L);
    if (!st) st = bspgemm_multiply_masked_dot(ctx, L, L, L, 0, &C, nullptr);
    if (!st) st = bspgemm_result_values_sum(ctx, C, &sum);
    bspgemm_result_free(C);
    bspgemm_matrix_free(L);
    if (st) return st;
    *triangles = sum;
    return BSPGEMM_OK;
}

// bspgemm_ktruss with the step's support counted by rows: C_ij = |S_i n (S^T)_j| is the entry (i, j) of S .* (S * S).  A
// symmetric S0 is its own transpose and stays symmetric (the support of (i, j) is that of (j, i)), so the symmetry is
// decided once; otherwise every step transposes its S.
extern "C" bspgemm_status bspgemm_ktruss_ex(bspgemm_context *ctx, const bspgemm_matrix *A, int k, int max_iter,
                                            bspgemm_support_method method, bspgemm_matrix **T, int *iterations, int *converged)
{
    if (method == BSPGEMM_SUPPORT_PRODUCT) return bspgemm_ktruss(ctx, A, k, max_iter, T, iterations, converged);
    if (T) *T = nullptr;
    if (iterations) *iterations = 0;
    if (converged) *converged = 0;
    if (method != BSPGEMM_SUPPORT_DOT) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_ktruss_ex: unknown method");
    if (!ctx || !A || !T) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_ktruss_ex: NULL argument");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_ktruss_ex", NEED_SQUARE)) return st;
    if (k < 2) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_ktruss_ex: k < 2");
    const int n = A->rows;
    bspgemm_matrix *S = nullptr, *St = nullptr;             // St: the transpose of the current S, when one is held
    bspgemm_status st = select_dedup(ctx, A, BSPGEMM_SELECT_OFFDIAG, &S);
    if (st) return st;
    int done = k == 2, sym = 0;                             // the 2-truss is the graph itself: no support is counted
    if (!done) {
        st = bspgemm_matrix_transpose(ctx, S, &St);
        if (!st) st = bspgemm_matrix_equal(ctx, S, St, &sym);
        if (sym) {
            bspgemm_matrix_free(St);
            St = nullptr;
        }
    }
    for (int it = 0; !st && !done; it++) {
        bspgemm_result *C = nullptr;
        bspgemm_matrix *next = nullptr;
        if (!sym && !St) st = bspgemm_matrix_transpose(ctx, S, &St);
        if (st) break;
        st = bspgemm_multiply_masked_dot(ctx, S, sym ? S : St, S, 0, &C, nullptr);
        bspgemm_matrix_free(St);
        St = nullptr;
        if (st) break;
        if (iterations) *iterations = it + 1;
        st = bspgemm_matrix_from_result_where(ctx, C, n, BSPGEMM_CMP_GE, k - 2, &next);
        bspgemm_result_free(C);
        if (st) break;
        const bool fixpoint = next->nnz == S->nnz || next->nnz == 0;   // nothing removed, or nothing left
        bspgemm_matrix_free(S);
        S = next;
        if (fixpoint) done = 1;
        else if (max_iter > 0 && it + 1 >= max_iter) break;
    }
    bspgemm_matrix_free(St);
    if (st) {
        bspgemm_matrix_free(S);
        return st;
    }
    if (converged) *converged = done;
    *T = S;
    return BSPGEMM_OK;
}
