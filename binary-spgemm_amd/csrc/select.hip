// select.hip -- stable filters of CSR entries on the device, the reduction of a counted result's values, and the two loops
// built on them: bspgemm_matrix_select, bspgemm_matrix_from_result_where, bspgemm_result_values_sum, bspgemm_triangle_count,
// bspgemm_ktruss (include/bspgemm.h).  The loads, the flag-word join and the row search are in sel_rows.hpp (also setop.hip's),
// the flag scratch and the operand builder in internal.hpp.
//
// One design serves the structural select (col against row) and the value select (count against a threshold).  Work is
// spread over ENTRIES: a workgroup owns kSelTile consecutive entries whatever rows they belong to, so a hub row of 10^5
// entries and a run of empty rows cost what any other 4096 entries cost.
//   pass 1  k_sel_flags_*   every lane takes four consecutive entries (one 16-byte load), evaluates the predicate and the
//                           16 lanes of a DPP row join their nibbles into the 64-bit flag word of their 64 entries: the
//                           word and its popcount are written, 12 bytes per 64 entries.  The value select reads only the
//                           values; the structural select reads col_idx and finds each entry's row: the tile's first row
//                           comes from a scatter over the rows (k_sel_tile_rows, as the flat prepass does it), the tile's
//                           window of row_ptr is staged in LDS, a lane searches that window once for its first entry and
//                           walks on from there for the other three.
//   scan    launch_scan_counts over the per-word counts
//   pass 2  k_sel_scatter   flag word, word prefix and col_idx again: kept entries go to prefix[word] + popcount(flags below)
//   rows    k_sel_row_ptr   new row_ptr[r] = prefix[p >> 6] + popcount(flags[p >> 6] & low_mask(p & 63)) for p = row_ptr[r]:
//                           O(1) per row, empty rows need nothing special
// Positions are 64-bit throughout: a counted result may hold more than 2^31 entries as long as the kept ones fit an operand.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

__device__ __forceinline__ bool keep_value(int v, int cmp, int thr)
{
    switch (cmp) {
    case BSPGEMM_CMP_GE: return v >= thr;
    case BSPGEMM_CMP_GT: return v > thr;
    case BSPGEMM_CMP_LE: return v <= thr;
    case BSPGEMM_CMP_LT: return v < thr;
    case BSPGEMM_CMP_EQ: return v == thr;
    default: return v != thr;
    }
}

__device__ __forceinline__ bool keep_struct(int col, int row, int op)
{
    return op == BSPGEMM_SELECT_TRIL ? col < row : (op == BSPGEMM_SELECT_TRIU ? col > row : col != row);
}

// pass 1 of the value select: 4 bytes read per entry, the values are not needed again (non-temporal)
__global__ __launch_bounds__(kSelThreads) void k_sel_flags_value(const int *__restrict__ vals, long long E, int cmp, int thr,
                                                                bool vec, u64 *__restrict__ flags, int *__restrict__ cnt)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long w0 = (long long)blockIdx.x * kSelTile + w * kSelWaveSpan;
    v4i v[kSelSteps];
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) v[j] = load4<true>(vals, w0 + j * kSelGroup + 4 * lane, E, vec);
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        unsigned nib = 0;
        if (e < E && keep_value(v[j].x, cmp, thr)) nib |= 1u;
        if (e + 1 < E && keep_value(v[j].y, cmp, thr)) nib |= 2u;
        if (e + 2 < E && keep_value(v[j].z, cmp, thr)) nib |= 4u;
        if (e + 3 < E && keep_value(v[j].w, cmp, thr)) nib |= 8u;
        store_flag_word(row_flag_word(nib, lane), w0 + j * kSelGroup, lane, flags, cnt);
    }
}

// tile_row[t] = the row that holds entry t * kSelTile, for every such entry below nnz: a scatter over the rows (a row of
// L entries writes at most L / kSelTile + 1 of them)
__global__ __launch_bounds__(256) void k_sel_tile_rows(const int *__restrict__ row_ptr, int rows, int *__restrict__ tile_row)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const long long a0 = row_ptr[r], a1 = row_ptr[r + 1];
    for (long long t = (a0 + kSelTile - 1) / kSelTile; t * kSelTile < a1; t++) tile_row[t] = r;
}

// pass 1 of the structural select.  col_idx is read again by pass 2, so these loads stay temporal.
__global__ __launch_bounds__(kSelThreads) void k_sel_flags_struct(const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                                 int rows, long long E, int op, bool vec,
                                                                 const int *__restrict__ tile_row, u64 *__restrict__ flags,
                                                                 int *__restrict__ cnt)
{
    __shared__ int srp[kSelStage + 1];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long b0 = (long long)blockIdx.x * kSelTile;               // < E: the grid is ceil(E / kSelTile)
    const bool last = b0 + kSelTile >= E;
    const int rb = tile_row[blockIdx.x];
    const int rl = last ? rows - 1 : tile_row[blockIdx.x + 1];           // every entry of the tile lies in rows rb .. rl
    const int span = rl - rb + 1;
    const bool staged = span <= kSelStage;                               // (else: mostly empty rows; searched in row_ptr itself)
    if (staged)
        for (int q = threadIdx.x; q <= span; q += kSelThreads) srp[q] = row_ptr[rb + q];
    __syncthreads();
    auto find = [&](int lo, int e) { return staged ? rb + sel_row_of(srp, lo - rb, span - 1, e) : sel_row_of(row_ptr, lo, rl, e); };
    auto row_end = [&](int r) { return staged ? srp[r - rb + 1] : row_ptr[r + 1]; };

    const long long w0 = b0 + w * kSelWaveSpan;
    v4i v[kSelSteps];
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) v[j] = load4<false>(col, w0 + j * kSelGroup + 4 * lane, E, vec);
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e0 = w0 + j * kSelGroup + 4 * lane;
        unsigned nib = 0;
        if (e0 < E) {
            const int c[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            int r = find(rb, (int)e0);                                   // one search per lane and step, then a walk
            int end = row_end(r);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (e0 + k >= E) break;
                if (e0 + k >= end) {
                    r = find(r + 1, (int)(e0 + k));
                    end = row_end(r);
                }
                if (keep_struct(c[k], r, op)) nib |= 1u << k;
            }
        }
        store_flag_word(row_flag_word(nib, lane), w0 + j * kSelGroup, lane, flags, cnt);
    }
}

// pass 2: the kept entries of src, in order, to out[pre[word] + flags below].  8 + 8 bytes per 64 entries, 4 bytes read per
// entry of a 16-byte group that keeps any, 4 bytes written per kept entry.
__global__ __launch_bounds__(kSelThreads) void k_sel_scatter(const int *__restrict__ src, long long E, bool vec,
                                                            const u64 *__restrict__ flags, const long long *__restrict__ pre,
                                                            int *__restrict__ out)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long w0 = (long long)blockIdx.x * kSelTile + w * kSelWaveSpan;
    u64 word[kSelSteps];
    long long base[kSelSteps];
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        word[j] = flags[e >> 6];
        base[j] = pre[e >> 6];
    }
    v4i v[kSelSteps];
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const long long e = w0 + j * kSelGroup + 4 * lane;
        v[j] = v4i{0, 0, 0, 0};
        if ((word[j] >> (e & 63)) & 0xfull) v[j] = load4<true>(src, e, E, vec);
    }
#pragma unroll
    for (int j = 0; j < kSelSteps; j++) {
        const int bit = (4 * lane) & 63;
        const unsigned nib = (unsigned)(word[j] >> bit) & 0xfu;
        long long pos = base[j] + __popcll(word[j] & mask_lt(bit));
        if (nib & 1u) out[pos++] = v[j].x;
        if (nib & 2u) out[pos++] = v[j].y;
        if (nib & 4u) out[pos++] = v[j].z;
        if (nib & 8u) out[pos++] = v[j].w;
    }
}

// the filtered row_ptr from the unfiltered one (int32 of an operand, int64 of a result)
template <typename P>
__global__ __launch_bounds__(256) void k_sel_row_ptr(const P *__restrict__ rp, int rows, long long E, long long words,
                                                    const u64 *__restrict__ flags, const long long *__restrict__ pre,
                                                    int *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    const long long p = rp[r];
    out[r] = p >= E ? (int)pre[words] : (int)(pre[p >> 6] + __popcll(flags[p >> 6] & mask_lt((int)(p & 63))));
}

// *sum += the values: int64 per lane, one shuffle reduction per wave, one atomic per workgroup
__global__ __launch_bounds__(256) void k_values_sum(const int *__restrict__ vals, long long E, bool vec,
                                                   unsigned long long *__restrict__ sum)
{
    __shared__ long long wsum[4];
    long long acc = 0;
    for (long long e = 4 * ((long long)blockIdx.x * 256 + threadIdx.x); e < E; e += 1024ll * gridDim.x) {
        const v4i v = load4<true>(vals, e, E, vec);
        acc += (long long)v.x + v.y + v.z + v.w;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);          // (open code: wave_sum compiles to other code here)
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum, (unsigned long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]));
}

void launch_select_tile_rows(const int *row_ptr, int rows, int *tile_row, hipStream_t s)
{
    hipLaunchKernelGGL(k_sel_tile_rows, dim3((rows + 255) / 256), dim3(256), 0, s, row_ptr, rows, tile_row);
}

void launch_select_flags_struct(const int *row_ptr, const int *col_idx, int rows, long long nnz, int op, int *tile_row,
                                unsigned long long *flags, int *cnt, hipStream_t s)
{
    if (nnz <= 0) return;
    launch_select_tile_rows(row_ptr, rows, tile_row, s);
    hipLaunchKernelGGL(k_sel_flags_struct, dim3(select_tiles(nnz)), dim3(kSelThreads), 0, s, row_ptr, col_idx, rows, nnz, op,
                       aligned16(col_idx), tile_row, flags, cnt);
}

void launch_select_flags_value(const int *vals, long long nnz, int cmp, int threshold, unsigned long long *flags, int *cnt,
                               hipStream_t s)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(k_sel_flags_value, dim3(select_tiles(nnz)), dim3(kSelThreads), 0, s, vals, nnz, cmp, threshold,
                       aligned16(vals), flags, cnt);
}

void launch_select_scatter(const int *src, long long nnz, const unsigned long long *flags, const long long *prefix, int *out,
                           hipStream_t s)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(k_sel_scatter, dim3(select_tiles(nnz)), dim3(kSelThreads), 0, s, src, nnz, aligned16(src), flags, prefix, out);
}

void launch_select_row_ptr(const int *row_ptr32, const long long *row_ptr64, int rows, long long nnz,
                           const unsigned long long *flags, const long long *prefix, int *out, hipStream_t s)
{
    const long long words = (long long)select_words(nnz);
    const dim3 grid = row_pass_grid(rows);
    if (row_ptr32)
        hipLaunchKernelGGL(k_sel_row_ptr<int>, grid, dim3(256), 0, s, row_ptr32, rows, nnz, words, flags, prefix, out);
    else
        hipLaunchKernelGGL(k_sel_row_ptr<long long>, grid, dim3(256), 0, s, row_ptr64, rows, nnz, words, flags, prefix, out);
}

void launch_values_sum(const int *vals, long long nnz, unsigned long long *sum, hipStream_t s)
{
    if (nnz <= 0) return;
    long long grid = (nnz + 4095) / 4096;                 // 16 entries per thread, up to 8 workgroups per CU
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(k_values_sum, dim3((unsigned)grid), dim3(256), 0, s, vals, nnz, aligned16(vals), sum);
}

}  // namespace bsp

using namespace bsp;

// ------------------------------------------------------------------ the two selects ------
// the flag scratch (internal.hpp) of a select over E entries, at the start of the context's upper-bound workspace
static bspgemm_status select_scratch(bspgemm_context *ctx, long long E, FlagScratch *sc)
{
    const size_t ints = flag_scratch_carve(nullptr, 0, E, false, nullptr);
    if (!ints) return FAIL(BSPGEMM_ERR_OVERFLOW, "select: too many entries for the word scan");
    if (bspgemm_status st = ensure_tmp(ctx, ints)) return st;
    flag_scratch_carve(ctx->tmp, 0, E, false, sc);
    return BSPGEMM_OK;
}

// What both selects do once pass 1 has left the flag words and counts of the E entries of `src`: the operand's handle and
// row_ptr, the scan, the call's one synchronisation (the kept count), col_idx, pass 2 and the row pass.  The operand is
// complete on the context's stream when the call returns; a failed call has freed what it made.
static bspgemm_status select_finish(bspgemm_context *ctx, int rows, int cols, const int *src, long long E, const int *rp32,
                                    const long long *rp64, const FlagScratch &sc, const char *who, bspgemm_matrix **out)
{
    hipStream_t s = ctx->stream;
    long long kept = 0;
    bspgemm_matrix *m = nullptr;
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bspgemm_matrix_free(m); return st; };
    if (bspgemm_status st = operand_new(ctx, rows, cols, &m)) return bail(st);
    if (E > 0) {
        launch_scan_counts(sc.cnt, sc.words, sc.pre, sc.part, nullptr, s);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(hipMemcpyAsync(&kept, sc.pre + sc.words, sizeof kept, hipMemcpyDeviceToHost, s));
        HIPCHK_B(hipStreamSynchronize(s));
        if (kept > INT_MAX) {
            snprintf(g_err, sizeof g_err, "%s: %lld entries kept: more than INT_MAX, not usable as an int32 operand", who, kept);
            return bail(BSPGEMM_ERR_OVERFLOW);
        }
    }
    if (bspgemm_status st = operand_cols(m, kept)) return bail(st);
    if (E > 0) {
        launch_select_scatter(src, E, sc.flags, sc.pre, m->d_col_idx, s);
        launch_select_row_ptr(rp32, rp64, rows, E, sc.flags, sc.pre, m->d_row_ptr, s);
    } else {
        HIPCHK_B(hipMemsetAsync(m->d_row_ptr, 0, ((size_t)rows + 1) * sizeof(int), s));
    }
    HIPCHK_B(hipGetLastError());
    if (bspgemm_status st = operand_finish(m, kept)) return bail(st);
    *out = m;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_matrix_select(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_select op,
                                                bspgemm_matrix **out)
{
    const char *who = "bspgemm_matrix_select";
    if (out) *out = nullptr;
    if (!ctx || !A || !out) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_select: NULL argument");
    if (bspgemm_status st = check_operand(ctx, A, who, 0)) return st;
    if (op != BSPGEMM_SELECT_TRIL && op != BSPGEMM_SELECT_TRIU && op != BSPGEMM_SELECT_OFFDIAG)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_select: unknown select op");
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    const long long E = A->nnz;
    FlagScratch sc = {};
    if (bspgemm_status st = select_scratch(ctx, E, &sc)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return st;
    launch_select_flags_struct(A->d_row_ptr, A->d_col_idx, A->rows, E, (int)op, ctx->tile_row, sc.flags, sc.cnt, ctx->stream);
    return select_finish(ctx, A->rows, A->cols, A->d_col_idx, E, A->d_row_ptr, nullptr, sc, who, out);
}

extern "C" bspgemm_status bspgemm_matrix_from_result_where(bspgemm_context *ctx, const bspgemm_result *C, int cols,
                                                           bspgemm_compare cmp, int threshold, bspgemm_matrix **out)
{
    if (out) *out = nullptr;
    if (!ctx || !C || !out) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_from_result_where: NULL argument");
    if (C->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_from_result_where: result belongs to another context");
    if (cols < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_from_result_where: negative column count");
    if (cmp < BSPGEMM_CMP_GE || cmp > BSPGEMM_CMP_NE) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_from_result_where: unknown comparison");
    if (!C->d_values) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_matrix_from_result_where: pattern-only result (no values)");
    if (bspgemm_status st = use_device(ctx)) return st;
    const long long E = C->nnz;
    FlagScratch sc = {};
    if (bspgemm_status st = select_scratch(ctx, E, &sc)) return st;
    launch_select_flags_value(C->d_values, E, (int)cmp, threshold, sc.flags, sc.cnt, ctx->stream);
    return select_finish(ctx, C->rows, cols, C->d_col_idx, E, nullptr, C->d_row_ptr, sc, "bspgemm_matrix_from_result_where", out);
}

extern "C" bspgemm_status bspgemm_result_values_sum(bspgemm_context *ctx, const bspgemm_result *C, int64_t *sum)
{
    if (!ctx || !C || !sum) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_result_values_sum: NULL argument");
    if (C->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_result_values_sum: result belongs to another context");
    if (!C->d_values) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_result_values_sum: pattern-only result (no values)");
    if (bspgemm_status st = use_device(ctx)) return st;
    if (bspgemm_status st = ensure_tmp(ctx, 4)) return st;
    unsigned long long *d_sum = reinterpret_cast<unsigned long long *>(ctx->tmp);
    long long h = 0;
    HIPCHK(hipMemsetAsync(d_sum, 0, sizeof *d_sum, ctx->stream));
    launch_values_sum(C->d_values, C->nnz, d_sum, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, d_sum, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *sum = h;
    return BSPGEMM_OK;
}

// ------------------------------------------------------------------ triangles, k-truss ---
// dedup(select(A, op)): the selection with sorted duplicate-free rows (internal.hpp: also dot.hip's loops)
bspgemm_status select_dedup(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_select op, bspgemm_matrix **out)
{
    bspgemm_matrix *sel = nullptr;
    bspgemm_status st = bspgemm_matrix_select(ctx, A, op, &sel);
    if (!st) st = operand_canonical(ctx, sel, out);
    bspgemm_matrix_free(sel);
    return st;
}

extern "C" bspgemm_status bspgemm_triangle_count(bspgemm_context *ctx, const bspgemm_matrix *A, int64_t *triangles)
{
    if (!ctx || !A || !triangles) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_triangle_count: NULL argument");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_triangle_count", NEED_SQUARE)) return st;
    bspgemm_matrix *L = nullptr;
    bspgemm_result *C = nullptr;
    int64_t sum = 0;
    bspgemm_status st = select_dedup(ctx, A, BSPGEMM_SELECT_TRIL, &L);
    if (!st) st = bspgemm_multiply_masked_count(ctx, L, L, L, 0, A->rows, &C);
    if (!st) st = bspgemm_result_values_sum(ctx, C, &sum);
    bspgemm_result_free(C);
    bspgemm_matrix_free(L);
    if (st) return st;
    *triangles = sum;
    return BSPGEMM_OK;
}

// S(0) = dedup(select(A, OFFDIAG)); S(j+1) = the entries of S(j) .* (S(j) * S(j)) with a count of k - 2 or more.  S(j+1) is a
// subset of S(j), so equal nnz is equal sets.
extern "C" bspgemm_status bspgemm_ktruss(bspgemm_context *ctx, const bspgemm_matrix *A, int k, int max_iter,
                                         bspgemm_matrix **T, int *iterations, int *converged)
{
    if (T) *T = nullptr;
    if (iterations) *iterations = 0;
    if (converged) *converged = 0;
    if (!ctx || !A || !T) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_ktruss: NULL argument");
    if (bspgemm_status st = check_operand(ctx, A, "bspgemm_ktruss", NEED_SQUARE)) return st;
    if (k < 2) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_ktruss: k < 2");
    const int n = A->rows;
    bspgemm_matrix *S = nullptr;
    bspgemm_status st = select_dedup(ctx, A, BSPGEMM_SELECT_OFFDIAG, &S);
    if (st) return st;
    int done = k == 2;                                      // the 2-truss is the graph itself: no product
    for (int it = 0; !st && !done; it++) {
        bspgemm_result *C = nullptr;
        bspgemm_matrix *next = nullptr;
        st = bspgemm_multiply_masked_count(ctx, S, S, S, 0, n, &C);
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
    if (st) {
        bspgemm_matrix_free(S);
        return st;
    }
    if (converged) *converged = done;
    *T = S;
    return BSPGEMM_OK;
}
