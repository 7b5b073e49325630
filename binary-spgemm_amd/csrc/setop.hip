// setop.hip -- entry-wise set operations on the patterns of two CSR operands, on the device: bspgemm_matrix_setop
// (A | B, A & B, A \ B, A ^ B), bspgemm_matrix_equal and bspgemm_matrix_symmetrize (include/bspgemm.h).
//
// The passes are select.hip's (sel_rows.hpp holds the device code they share, internal.hpp the flag scratch): work is
// spread over ENTRIES, a workgroup owns kSelTile consecutive entries of one operand X whatever rows they belong to, and
// what is kept is described by 64-bit flag words, their popcounts and one scan.  For operands whose rows are strictly
// ascending ("canonical"):
//   pass 1  k_set_flags     every lane takes four consecutive entries of X (one 16-byte load) and finds their row like the
//                           structural select.  It CHECKS them -- 0 <= col < cols, and col[p] > col[p - 1] unless p starts a
//                           row -- into an error word, and binary-searches each column in the same row of the other operand
//                           Y: lb = the position in Y.col_idx of the first entry of that row that is not below the column,
//                           common = Y holds the column.  The common bits become the flag word and its popcount (12 bytes per
//                           64 entries); OR and XOR also keep lb, 4 bytes per entry, because with it pass 2 needs no row.
//   scan    launch_scan_counts over the per-word counts: cX(p) = common entries of X before p
//   pass 2  AND / ANDNOT    select's scatter and row pass over A's flags (ANDNOT: pass 1 wrote them inverted)
//           OR / XOR        k_set_place, once per operand: entry p of X goes to p + lb[p] - k cX(p), k = 1 (OR: all of A, the
//                           non-common entries of B) or 2 (XOR: the non-common entries of both).  That is base[r] + i + ...
//                           of the row-wise formula with the row's terms cancelled: p counts the X-entries before it, lb
//                           the Y-entries of earlier rows and the smaller ones of this row, and cX(p) those counted twice.
//   rows    k_set_row_ptr   row_ptr'[r] = rpA[r] + rpB[r] - k cA(rpA[r]): O(1) per row
// The one synchronisation reads the error word and the common count (the result's size follows from it).  An operand that
// the check found not canonical is brought to that form by transposing it twice and the passes run again; a column out of
// range fails the call.  Positions are 64-bit inside the kernels.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

constexpr int kSetErrShiftB = 2;         // operand B's two bits (kSetErrRange, kSetErrOrder: kernels.hpp)

// pass 1 over operand X.  SEARCH false: the check alone (nothing but *err is written).  The columns are read again by pass
// 2, so the loads stay temporal.  invert: the flags are the NON-common entries (ANDNOT).  lbs (may be NULL): lb per entry.
template <bool SEARCH>
__global__ __launch_bounds__(kSelThreads) void k_set_flags(const int *__restrict__ rpX, const int *__restrict__ colX, int rows,
                                                          int cols, long long E, bool vec, const int *__restrict__ tile_row,
                                                          const int *__restrict__ rpY, const int *__restrict__ colY,
                                                          bool invert, int err_shift, u64 *__restrict__ flags,
                                                          int *__restrict__ cnt, int *__restrict__ lbs,
                                                          unsigned *__restrict__ err)
{
    __shared__ int srp[kSelStage + 1];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const SelTileRows tr = sel_stage_tile_rows(rpX, rows, E, tile_row, srp);
    const long long w0 = (long long)blockIdx.x * kSelTile + w * kSelWaveSpan;
    v4i v[kSelSteps];
    int before[kSelSteps];                                               // the column in front of the lane's four
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        v[j] = load4<false>(colX, e, E, vec);
        before[j] = e > 0 && e < E ? colX[e - 1] : -1;
    }
    unsigned bad = 0;
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e0 = w0 + j * kSelGroup + 4 * lane;
        unsigned nib = 0;
        if (e0 < E) {
            const int c[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            int lb[4] = {0, 0, 0, 0};
            int r = tr.find(tr.rb, (int)e0);                             // one search per lane and step, then a walk
            int beg = tr.row_begin(r), end = tr.row_end(r);
            int from = 0, yend = 0;                                      // what is left of Y's row: X ascends, so does lb
            if (SEARCH) {
                from = rpY[r];
                yend = rpY[r + 1];
            }
            int pc = before[j];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const long long p = e0 + k;
                if (p >= E) break;
                if (p >= end) {
                    r = tr.find(r + 1, (int)p);
                    beg = tr.row_begin(r);
                    end = tr.row_end(r);
                    if (SEARCH) {
                        from = rpY[r];
                        yend = rpY[r + 1];
                    }
                }
                if ((unsigned)c[k] >= (unsigned)cols) bad |= kSetErrRange;
                if (p > beg && c[k] <= pc) bad |= kSetErrOrder;
                pc = c[k];
                if (SEARCH) {
                    from = sel_lower_bound(colY, from, yend, c[k]);
                    const bool common = from < yend && colY[from] == c[k];
                    if (common != invert) nib |= 1u << k;
                    lb[k] = from;
                }
            }
            if (SEARCH && lbs) *reinterpret_cast<v4i *>(lbs + e0) = v4i{lb[0], lb[1], lb[2], lb[3]};   // (whole tiles)
        }
        if (SEARCH) store_flag_word(row_flag_word(nib, lane), w0 + j * kSelGroup, lane, flags, cnt);
    }
    if (bad) atomicOr(err, bad << err_shift);
}

// pass 2 of OR and XOR over operand X: entry p goes to p + lb[p] - k * (common entries before p); all: the common entries
// are placed too (the A side of OR), else only the others.  flags: the COMMON entries.
__global__ __launch_bounds__(kSelThreads) void k_set_place(const int *__restrict__ colX, long long E, bool vec,
                                                          const u64 *__restrict__ flags, const long long *__restrict__ pre,
                                                          const int *__restrict__ lbs, int k, bool all, int *__restrict__ out)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long w0 = (long long)blockIdx.x * kSelTile + w * kSelWaveSpan;
    u64 word[kSelSteps];
    long long base[kSelSteps];
    v4i v[kSelSteps], g[kSelSteps];
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        word[j] = flags[e >> 6];
        base[j] = pre[e >> 6];
        v[j] = load4<true>(colX, e, E, vec);
        g[j] = *reinterpret_cast<const v4i *>(lbs + e);                  // (whole tiles)
    }
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        const int bit = (4 * lane) & 63;
        const unsigned nib = (unsigned)(word[j] >> bit) & 0xfu;
        long long common = base[j] + __popcll(word[j] & mask_lt(bit));
        const int c[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        const int lb[4] = {g[j].x, g[j].y, g[j].z, g[j].w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (e + q >= E) break;
            const bool is_common = (nib >> q) & 1u;
            if (all || !is_common) out[e + q + lb[q] - k * common] = c[q];
            common += is_common;
        }
    }
}

// row_ptr of A | B (k = 1) or A ^ B (k = 2) from A's flags of common entries; EA == 0: nothing is common
__global__ __launch_bounds__(256) void k_set_row_ptr(const int *__restrict__ rpA, const int *__restrict__ rpB, int rows,
                                                    long long EA, long long wordsA, const u64 *__restrict__ flags,
                                                    const long long *__restrict__ pre, int k, int *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    const long long p = rpA[r];
    long long common = 0;
    if (EA > 0) common = p >= EA ? pre[wordsA] : pre[p >> 6] + __popcll(flags[p >> 6] & mask_lt((int)(p & 63)));
    out[r] = (int)(p + rpB[r] - k * common);
}

// pass 1 over operand X against Y (same shape): *err |= (kSetErrRange: a column outside [0, cols), kSetErrOrder: a row not
// strictly ascending), shifted left by kSetErrShiftB when `second`.  search: bit b of flags[w] = entry 64 w + b of X is also
// in Y's row (invert: is not), cnt[w] its popcount, and (lbs != NULL, whole tiles of ints) lbs[e] = the position in colY of
// the first entry of the row that is not below X's column.  Without search only the check runs.  tile_row: nnzX / kSelTile
// + 1 ints of scratch.
static void launch_setop_flags(const int *rpX, const int *colX, int rows, int cols, long long nnzX, const int *rpY,
                               const int *colY, bool search, bool invert, bool second, int *tile_row,
                               unsigned long long *flags, int *cnt, int *lbs, unsigned *err, hipStream_t s)
{
    if (nnzX <= 0) return;
    launch_select_tile_rows(rpX, rows, tile_row, s);
    const dim3 grid(select_tiles(nnzX)), block(kSelThreads);
    const int shift = second ? kSetErrShiftB : 0;
    if (search)
        hipLaunchKernelGGL(k_set_flags<true>, grid, block, 0, s, rpX, colX, rows, cols, nnzX, aligned16(colX), tile_row, rpY,
                           colY, invert, shift, flags, cnt, lbs, err);
    else
        hipLaunchKernelGGL(k_set_flags<false>, grid, block, 0, s, rpX, colX, rows, cols, nnzX, aligned16(colX), tile_row, rpY,
                           colY, invert, shift, flags, cnt, lbs, err);
}

// the check alone over one operand (kernels.hpp): k_set_flags<false>, the instance that setop's second side launches
void launch_canonical_check(const int *row_ptr, const int *col_idx, int rows, int cols, long long nnz, int err_shift,
                            int *tile_row, unsigned *err, hipStream_t s)
{
    if (nnz <= 0) return;
    launch_select_tile_rows(row_ptr, rows, tile_row, s);
    hipLaunchKernelGGL(k_set_flags<false>, dim3(select_tiles(nnz)), dim3(kSelThreads), 0, s, row_ptr, col_idx, rows, cols, nnz,
                       aligned16(col_idx), tile_row, (const int *)nullptr, (const int *)nullptr, false, err_shift,
                       (u64 *)nullptr, (int *)nullptr, (int *)nullptr, err);
}

// pass 2 of OR (k = 1) and XOR (k = 2) over X: out[e + lbs[e] - k * (common entries before e)] = colX[e] for every entry
// (all) or every non-common one; flags: the common entries, prefix: the scan of their counts
static void launch_setop_place(const int *colX, long long nnzX, const unsigned long long *flags, const long long *prefix,
                               const int *lbs, int k, bool all, int *out, hipStream_t s)
{
    if (nnzX <= 0) return;
    hipLaunchKernelGGL(k_set_place, dim3(select_tiles(nnzX)), dim3(kSelThreads), 0, s, colX, nnzX, aligned16(colX), flags,
                       prefix, lbs, k, all, out);
}

// out[r] = rpA[r] + rpB[r] - k * (common entries of A before rpA[r]), r in [0, rows]
static void launch_setop_row_ptr(const int *rpA, const int *rpB, int rows, long long nnzA, const unsigned long long *flags,
                                 const long long *prefix, int k, int *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_set_row_ptr, row_pass_grid(rows), dim3(256), 0, s, rpA, rpB, rows, nnzA,
                       (long long)select_words(nnzA), flags, prefix, k, out);
}

}  // namespace bsp

using namespace bsp;

// ------------------------------------------------------------------ the host side --------
// op: a bspgemm_setop, or 0 for the comparison (*equal).  The arguments are checked by the callers.  canonical: both
// operands are known to have strictly ascending rows (the second round).
static bspgemm_status setop_run(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, int op,
                                bspgemm_matrix **out, int *equal, const char *who, bool canonical)
{
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const long long EA = A->nnz, EB = B->nnz;
    const int rows = A->rows, cols = A->cols;
    const bool both = op == BSPGEMM_SETOP_OR || op == BSPGEMM_SETOP_XOR;      // B contributes entries: both sides are searched
    const int k = op == BSPGEMM_SETOP_XOR ? 2 : 1;
    // the workspace: the error word (four ints), then the flag scratch of each side (B's is empty unless B is searched)
    const long long EBs = both ? EB : 0;
    const size_t o_b = flag_scratch_carve(nullptr, 4, EA, both, nullptr);
    const size_t total = o_b ? flag_scratch_carve(nullptr, o_b, EBs, both, nullptr) : 0;
    if (!total) return FAIL(BSPGEMM_ERR_OVERFLOW, "setop: too many entries for the word scan");
    if (bspgemm_status st = ensure_tmp(ctx, total)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)(EA > EB ? EA : EB))) return st;
    unsigned *d_err = reinterpret_cast<unsigned *>(ctx->tmp);
    FlagScratch sa, sb;
    flag_scratch_carve(ctx->tmp, 4, EA, both, &sa);
    flag_scratch_carve(ctx->tmp, o_b, EBs, both, &sb);

    // A's flags: its common entries (ANDNOT: the others).  The kernels of the two sides follow each other on the stream,
    // so they share tile_row.
    HIPCHK(hipMemsetAsync(d_err, 0, 4 * sizeof(int), s));
    launch_setop_flags(A->d_row_ptr, A->d_col_idx, rows, cols, EA, B->d_row_ptr, B->d_col_idx, true, op == BSPGEMM_SETOP_ANDNOT,
                       false, ctx->tile_row, sa.flags, sa.cnt, sa.lbs, d_err, s);
    if (EA > 0) launch_scan_counts(sa.cnt, sa.words, sa.pre, sa.part, nullptr, s);
    launch_setop_flags(B->d_row_ptr, B->d_col_idx, rows, cols, EB, A->d_row_ptr, A->d_col_idx, both, false, true, ctx->tile_row,
                       sb.flags, sb.cnt, sb.lbs, d_err, s);
    if (both && EB > 0) launch_scan_counts(sb.cnt, sb.words, sb.pre, sb.part, nullptr, s);
    HIPCHK(hipGetLastError());
    long long flagged = 0;                                                    // entries of A that pass 1 flagged
    unsigned err = 0;
    if (EA > 0) HIPCHK(hipMemcpyAsync(&flagged, sa.pre + sa.words, sizeof flagged, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                                          // the call's one synchronisation

    const unsigned range = kSetErrRange | (kSetErrRange << kSetErrShiftB), order = kSetErrOrder | (kSetErrOrder << kSetErrShiftB);
    if (err & range) {
        snprintf(g_err, sizeof g_err, "%s: a column index outside [0, %d) in operand %s", who, cols, (err & kSetErrRange) ? "A" : "B");
        return BSPGEMM_ERR_INVALID;
    }
    if (err & order) {
        if (canonical) return FAIL(BSPGEMM_ERR_HIP, "setop: a transposed operand is not in ascending order");
        // what pass 1 left is discarded: the operands whose rows are unsorted or hold repeats are transposed twice
        bspgemm_matrix *ca = nullptr, *cb = nullptr;
        bspgemm_status st = BSPGEMM_OK;
        const bool same = A == B;
        if (same || (err & kSetErrOrder)) st = operand_canonical(ctx, A, &ca);
        if (same) cb = ca;
        else if (!st && (err & (kSetErrOrder << kSetErrShiftB))) st = operand_canonical(ctx, B, &cb);
        if (!st) st = setop_run(ctx, ca ? ca : A, cb ? cb : B, op, out, equal, who, true);
        if (cb != ca) bspgemm_matrix_free(cb);
        bspgemm_matrix_free(ca);
        return st;
    }
    if (op == 0) {
        *equal = EA == EB && flagged == EA;
        return BSPGEMM_OK;
    }
    const long long kept = both ? EA + EB - k * flagged : flagged;
    if (kept > INT_MAX) {
        snprintf(g_err, sizeof g_err, "%s: %lld entries in the result: more than INT_MAX, not usable as an int32 operand", who, kept);
        return BSPGEMM_ERR_OVERFLOW;
    }
    bspgemm_matrix *m = nullptr;
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bspgemm_matrix_free(m); return st; };
    if (bspgemm_status st = operand_new(ctx, rows, cols, &m)) return bail(st);
    if (bspgemm_status st = operand_cols(m, kept)) return bail(st);
    if (both ? EA + EB == 0 : EA == 0) {
        HIPCHK_B(hipMemsetAsync(m->d_row_ptr, 0, ((size_t)rows + 1) * sizeof(int), s));
    } else if (both) {
        launch_setop_place(A->d_col_idx, EA, sa.flags, sa.pre, sa.lbs, k, op == BSPGEMM_SETOP_OR, m->d_col_idx, s);
        launch_setop_place(B->d_col_idx, EB, sb.flags, sb.pre, sb.lbs, k, false, m->d_col_idx, s);
        launch_setop_row_ptr(A->d_row_ptr, B->d_row_ptr, rows, EA, sa.flags, sa.pre, k, m->d_row_ptr, s);
    } else {
        launch_select_scatter(A->d_col_idx, EA, sa.flags, sa.pre, m->d_col_idx, s);
        launch_select_row_ptr(A->d_row_ptr, nullptr, rows, EA, sa.flags, sa.pre, m->d_row_ptr, s);
    }
    HIPCHK_B(hipGetLastError());
    if (bspgemm_status st = operand_finish(m, kept)) return bail(st);
    *out = m;
    return BSPGEMM_OK;
}

// what setop and equal ask of their operands; who: the function's name
static bspgemm_status setop_operands(const bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, const char *who)
{
    if (bspgemm_status st = check_operand(ctx, A, who, 0)) return st;
    if (bspgemm_status st = check_operand(ctx, B, who, 0)) return st;
    if (A->rows != B->rows || A->cols != B->cols) {
        snprintf(g_err, sizeof g_err, "%s: the operands differ in shape", who);
        return BSPGEMM_ERR_INVALID;
    }
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    return check_operand(ctx, B, who, NEED_ENTRIES_CONSISTENT);
}

extern "C" bspgemm_status bspgemm_matrix_setop(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                               bspgemm_setop op, bspgemm_matrix **out)
{
    if (out) *out = nullptr;
    if (!ctx || !A || !B || !out) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_setop: NULL argument");
    if (op != BSPGEMM_SETOP_OR && op != BSPGEMM_SETOP_AND && op != BSPGEMM_SETOP_ANDNOT && op != BSPGEMM_SETOP_XOR)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_setop: unknown set operation");
    if (bspgemm_status st = setop_operands(ctx, A, B, "bspgemm_matrix_setop")) return st;
    return setop_run(ctx, A, B, (int)op, out, nullptr, "bspgemm_matrix_setop", false);
}

extern "C" bspgemm_status bspgemm_matrix_equal(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, int *equal)
{
    if (!ctx || !A || !B || !equal) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_equal: NULL argument");
    if (bspgemm_status st = setop_operands(ctx, A, B, "bspgemm_matrix_equal")) return st;
    int eq = 0;
    if (bspgemm_status st = setop_run(ctx, A, B, 0, nullptr, &eq, "bspgemm_matrix_equal", false)) return st;
    *equal = eq;
    return BSPGEMM_OK;
}

// What bspgemm_matrix_symmetrize below asks of the context's upper-bound workspace at most, for an n x n operand of E
// entries: the select's flag scratch, the transposes (of the operand, and of both sides when rows turn out unsorted) and
// the union's two flag scratches, each of at most E entries and each monotone in its entry count.  A caller that carves
// state of its own from the workspace afterwards grows it once, to the larger of the two, instead of stage by stage.
size_t symmetrize_workspace_ints(long long E, int n)
{
    size_t ints = flag_scratch_carve(nullptr, 0, E, false, nullptr);
    ints = std::max(ints, transpose_workspace_ints(E, n));
    const size_t o_b = flag_scratch_carve(nullptr, 4, E, true, nullptr);
    return std::max(ints, o_b ? flag_scratch_carve(nullptr, o_b, E, true, nullptr) : 0);
}

extern "C" bspgemm_status bspgemm_matrix_symmetrize(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags,
                                                    bspgemm_matrix **out)
{
    if (out) *out = nullptr;
    if (!ctx || !A || !out) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_symmetrize: NULL argument");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_matrix_symmetrize", 0)) return st;
    if (flags & ~BSPGEMM_SYMMETRIZE_DROP_DIAGONAL) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_symmetrize: unknown flag");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_matrix_symmetrize", NEED_SQUARE)) return st;
    bspgemm_matrix *off = nullptr, *t = nullptr;
    bspgemm_status st = BSPGEMM_OK;
    if (flags & BSPGEMM_SYMMETRIZE_DROP_DIAGONAL) st = bspgemm_matrix_select(ctx, A, BSPGEMM_SELECT_OFFDIAG, &off);
    const bspgemm_matrix *src = off ? off : A;
    if (!st) st = bspgemm_matrix_transpose(ctx, src, &t);
    if (!st) st = bspgemm_matrix_setop(ctx, src, t, BSPGEMM_SETOP_OR, out);
    bspgemm_matrix_free(t);
    bspgemm_matrix_free(off);
    return st;
}
