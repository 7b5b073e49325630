// multiply.hip -- bspgemm_multiply and what is built on it: the two ways from row sizes to C.col_idx
// (upper-bound placement + compaction, exact symbolic sizes + emit in place), the masked product, products
// as operands, the closure, the sharding helpers.  Replaces SpGEMM_omp / SpGEMM_bigslice
// (final/SpGEMM_mpi_omp.c:71-143, :15-58) behind the native handle API.
#include "internal.hpp"

using namespace bsp;

// ------------------------------------------------------------------ multiply -------------
static bspgemm_status check_operands(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                     int row_begin, int row_end)
{
    if (!ctx || !A || !B) return FAIL(BSPGEMM_ERR_INVALID, "NULL operand");
    if (A->ctx != ctx || B->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "operand belongs to another context");
    if (row_begin < 0 || row_end < row_begin || row_end > A->rows) return FAIL(BSPGEMM_ERR_INVALID, "row range");
    if (B->rows < A->cols) return FAIL(BSPGEMM_ERR_INVALID, "B has fewer rows than A has columns");
    return BSPGEMM_OK;
}


// Launch order of the classes of one phase: order[1..kNumBins-1], alternating over the class streams.  The heavy
// rows first (few long-running workgroups: started early they finish under the other classes instead of being
// the phase's tail), then the one-wave classes LARGEST WORK FIRST (rows x capacity): a phase then ends with its
// small launches, whose ramp-down is short, instead of with the 24-32-chunk classes (measured on the bench
// matrix against ascending capacity: numeric phase 3.74 -> 3.60 ms, step -1.7 %; descending capacity -0.5 %;
// `profiles/r03_ab_class_order.log`).  Where the heavy classes are a large part of the product the one-wave
// classes queue behind them and ascending capacity measured better (power-law: +0.8 % otherwise): kept there.
static void class_order(const int *bin_count, long long total_products, int *order, int *lane)
{
    int light[kWaveBins];                                         // the one-wave classes in launch order
    for (int k = 0; k < kWaveBins; k++) light[k] = k + 1;
    const long long heavy_lower_bound = ((long long)bin_count[kRankBin] + bin_count[kMidBin] + bin_count[kDenseBin]) * kMaxWaveCap;
    if (heavy_lower_bound * 8 < total_products) {
        long long key[kNumBins] = {};
        for (int b = 1; b <= kWaveBins; b++) key[b] = (long long)bin_count[b] * kWaveChunks[b];
        for (int a = 1; a < kWaveBins; a++)                       // insertion sort of 16 entries, stable
            for (int c = a; c > 0 && key[light[c]] > key[light[c - 1]]; c--) {
                const int t = light[c];
                light[c] = light[c - 1];
                light[c - 1] = t;
            }
    }
    // streams (taken modulo the number in use): the hub rows on 1, the small dense shape on 0 and the rank class behind IT --
    // the hub rows' stream ends last where heavy rows matter (power-law stress input: the rank class used to wait 2.5 ms for
    // them) -- and the one-wave classes alternating from 1, as they always did
    order[0] = 0;
    lane[0] = 0;
    order[1] = kDenseBin;
    lane[1] = 1;
    order[2] = kMidBin;
    lane[2] = 0;
    order[3] = kRankBin;
    lane[3] = 0;
    for (int k = 0; k < kWaveBins; k++) {
        order[4 + k] = light[k];
        lane[4 + k] = 3 + k;
    }
    static_assert(kNumBins == kWaveBins + 4, "every class has a position");
}

// the hub rows (class kDenseBin) of a multiply, largest first when there are few enough to rank
static void hub_order(bspgemm_context *ctx, int b, int n, const RowRec *&rec, const long long *&recpre, hipStream_t sx)
{
    if (b != kDenseBin || n < 2 || n > kHeavySortMax) return;
    launch_order_heavy(rec, recpre, n, ctx->hub_rec, ctx->hub_pre, sx);
    rec = ctx->hub_rec;
    recpre = ctx->hub_pre;
}

// opens the next stat slot of the context; small: the single-round-trip path (one stream, never checked)
static bspgemm_context::StatSlot &open_slot(bspgemm_context *ctx, int flow, bool small)
{
    ctx->slot_head = (ctx->slot_head + 1) % bspgemm_context::kStatSlots;
    bspgemm_context::StatSlot &slot = ctx->slots[ctx->slot_head];
    slot.used = false;
    slot.flow = flow;
    slot.class_streams = small ? 1 : ctx->class_streams;
    slot.small = small;
    slot.checked = !small && ctx->check;
    return slot;
}

// closes the multiply's stat slot (its events have all completed: the caller has synchronised)
static void close_slot(bspgemm_context *ctx, int R, const HostScalars *h, long long products, long long nnz_c,
                       const int (*cls_n)[kNumBins], int mid_cap, int rank_cap = 0)
{
    bspgemm_context::StatSlot &sl = ctx->slots[ctx->slot_head];
    sl.R = R;
    sl.cls_timed = ctx->class_timing;
    sl.mid_cap = mid_cap;
    sl.rank_cap = rank_cap;
    sl.h = *h;
    sl.products = products;
    sl.nnz_c = nnz_c;
    memcpy(sl.cls_n, cls_n, sizeof sl.cls_n);
    sl.used = true;
}

// releases a result of the general flows that failed: nothing of C may still be written when it is released
static bspgemm_status drop_result(bspgemm_result *C, bspgemm_status st)
{
    const bspgemm_context *ctx = C->ctx;
    hipStreamSynchronize(ctx->stream); hipStreamSynchronize(ctx->stream_b); hipStreamSynchronize(ctx->stream_c);
    bspgemm_result_free(C);
    return st;
}

// C.col_idx with room for `cap` entries
static hipError_t alloc_col_idx(bspgemm_context *ctx, bspgemm_result *C, long long cap)
{
    if (hipError_t e = result_alloc(ctx, reinterpret_cast<void **>(&C->d_col_idx), result_bytes_colidx(cap))) return e;
    C->col_cap = cap;
    return hipSuccess;
}
// entries of C.col_idx once nnz(C) is known: exactly that, or the flow's bound when it is within 2 % of nnz(C) (the next
// product of this shape then finds it cached)
static long long col_cap_for(long long bound, long long nnz_c) { return (bound - nnz_c <= nnz_c / 50 + 4096) ? bound : nnz_c; }

// What both general flows start with: the operands checked (Fm: the mask, or NULL), the per-row workspace sized, the result
// *C with its row_ptr, the stat slot opened (ev[0]), B's derived tables built on its first use as B (the padded copy, then the
// blocked table over it; wrapped device arrays: first use) and the prepass launched: F_i and the extents ab[] of the rows.
static bspgemm_status start_flow(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                 const bspgemm_matrix *Fm, int row_begin, int row_end, int flow, bspgemm_result **out,
                                 bspgemm_result **Cp)
{
    if (!out) return FAIL(BSPGEMM_ERR_INVALID, "result pointer is NULL");
    *out = nullptr;
    if (bspgemm_status st = check_operands(ctx, A, B, row_begin, row_end)) return st;
    if (Fm && (Fm->ctx != ctx || Fm->rows < row_end)) return FAIL(BSPGEMM_ERR_INVALID, "mask has fewer rows than A / wrong context");
    if (bspgemm_status st = use_device(ctx)) return st;
    const int R = row_end - row_begin;
    hipStream_t s = ctx->stream;
    if (bspgemm_status st = ensure_rows(ctx, (size_t)R + 1)) return st;
    if (bspgemm_status st = ensure_ab(ctx, (size_t)A->nnz + 1)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)A->nnz + (size_t)R)) return st;

    bspgemm_result *C = new (std::nothrow) bspgemm_result{ctx, R, 0, nullptr, nullptr, 0};
    if (!C) return FAIL(BSPGEMM_ERR_ALLOC, "result");
    auto bail = [&](bspgemm_status st) { return drop_result(C, st); };
    bspgemm_context::StatSlot &slot = open_slot(ctx, flow, false);
    HIPCHK_B(hipEventRecord(slot.ev[0], s));
    HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&C->d_row_ptr), result_bytes_rowptr(R)));
    if (bspgemm_status st = ensure_pad(B)) return bail(st);
    if (bspgemm_status st = ensure_blk16(B)) return bail(st);
    if (ctx->check) {              // BSPGEMM_OPT_CHECK: B's derived tables verified against its row_ptr before the prepass uses them
        HIPCHK_B(hipMemsetAsync(ctx->d_err, 0, sizeof(unsigned), s));
        launch_check_tables(B->d_row_ptr, B->rows, B->d_deg8, B->blk16_state == 1 ? B->d_blk16 : nullptr,
                            B->pad_state == 1 ? B->d_row_ptr_pad : nullptr, ctx->d_err, s);
    }
    slot.prepass_kernel = B->blk16_state == 1 ? 1 : 0;
    slot.padded = B->pad_state == 1;
    launch_row_work(A->d_row_ptr, A->d_col_idx, B->d_row_ptr, B->blk16_state == 1 ? B->d_blk16 : nullptr,
                    B->pad_state == 1 ? B->d_row_ptr_pad : nullptr, B->pad_state == 1 ? B->d_ext : nullptr, row_begin, row_end,
                    A->nnz, ctx->tile_row, ctx->F, ctx->ab, s);
    *Cp = C;
    return BSPGEMM_OK;
}

// One phase's class launches (0: the exact flow's count pass, 1: the numeric pass), the classes of h->bin_count in
// class_order.  The launches are independent (disjoint rows): they alternate over the class streams so that one launch's
// draining tail overlaps the next one's ramp-up.  The side streams start behind the phase's inputs (fork) and the main
// stream waits for them at its end (join).  heavy_on_third: the heavy classes run on the third stream, which the phase
// forks and the caller joins.  launch(b, n, rec, recpre, stream) launches the n rows of class b; cls_n[b] = n.
template <class Launch>
static bspgemm_status class_phase(bspgemm_context *ctx, int phase, long long products, int *cls_n, bool heavy_on_third,
                                  Launch launch)
{
    const int *bin_count = ctx->h->bin_count;
    hipStream_t lanes[3] = {ctx->stream, ctx->stream_b, ctx->stream_c};
    const int nlanes = ctx->class_streams;
    hipEvent_t *tile = ctx->ev_tile[phase];
    hipEvent_t (*ev_cls)[2] = ctx->slots[ctx->slot_head].ev_cls[phase];
    size_t bin_start[kNumBins + 1] = {0, 0};               // class b's segment of rec[] (class 0 has none)
    for (int b = 1; b < kNumBins; b++) bin_start[b + 1] = bin_start[b] + (size_t)bin_count[b];
    int order[kNumBins], lane_of[kNumBins];
    class_order(bin_count, products, order, lane_of);

    HIPCHK(hipEventRecord(tile[0], lanes[0]));
    for (int l = 1; l < 3; l++)
        if (l < nlanes || (l == 2 && heavy_on_third)) HIPCHK(hipStreamWaitEvent(lanes[l], tile[0], 0));
    for (int pos = 1; pos < kNumBins; pos++) {
        const int b = order[pos];
        const int n = bin_count[b];
        cls_n[b] = n;
        if (n <= 0) continue;
        hipStream_t sx = heavy_on_third && b > kWaveBins ? lanes[2] : lanes[lane_of[pos] % nlanes];
        if (ctx->class_timing) HIPCHK(hipEventRecord(ev_cls[b][0], sx));
        HIPCHK(launch(b, n, ctx->rec + bin_start[b], ctx->recpre + bin_start[b], sx));
        if (ctx->class_timing) HIPCHK(hipEventRecord(ev_cls[b][1], sx));
    }
    HIPCHK(hipGetLastError());
    for (int l = 1; l < nlanes; l++) {
        HIPCHK(hipEventRecord(tile[l], lanes[l]));
        HIPCHK(hipStreamWaitEvent(lanes[0], tile[l], 0));
    }
    return BSPGEMM_OK;
}

// What both general flows end with once C.col_idx is complete on the main stream: ev[4], the error word read back, the last
// synchronisation, the verdict, the stat slot closed and C handed out
static bspgemm_status finish_flow(bspgemm_context *ctx, bspgemm_result *C, const bspgemm_matrix *B, long long products,
                                  int rank_cap, const int (*cls_n)[kNumBins], bspgemm_result **out)
{
    auto bail = [&](bspgemm_status st) { return drop_result(C, st); };
    hipStream_t s = ctx->stream;
    HostScalars *h = ctx->h;
    HIPCHK_B(hipEventRecord(ctx->slots[ctx->slot_head].ev[4], s));
    if (ctx->check) HIPCHK_B(hipMemcpyAsync(&h->err, ctx->d_err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));
    if (ctx->check && h->err)      // (start_flow cleared the error word)
        return bail(FAIL(BSPGEMM_ERR_INVALID, (h->err & kErrStaleTable)
            ? "operand B was rewritten in place: its derived tables do not match its row_ptr (call bspgemm_matrix_invalidate)"
            : "a row gathered more products than its capacity class holds (operand changed during the multiply?)"));
    C->nnz = h->nnzC;
    close_slot(ctx, C->rows, h, products, C->nnz, cls_n, mid_cap_for_cols(B->cols), rank_cap);
    *out = C;
    return BSPGEMM_OK;
}


// C rows [row_begin,row_end) of A*B:  symbolic (row work -> classes -> EXACT row sizes -> scan =
// C.row_ptr) then numeric (every one-wave row emitted at its final place in a C.col_idx of exactly
// nnz(C) entries) -- the two passes BASELINE.json's north star names.  Heavy rows (F_i > 2048) are
// accumulated and read out once, during the symbolic phase, into a workspace bounded by
// sum(min(F_i, cols)), and moved to their place during the numeric phase.
static bspgemm_status multiply_exact(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                     int row_begin, int row_end, bspgemm_result **out)
{
    bspgemm_result *C = nullptr;
    if (bspgemm_status st = start_flow(ctx, A, B, nullptr, row_begin, row_end, BSPGEMM_FLOW_EXACT, out, &C)) return st;
    auto bail = [&](bspgemm_status st) { return drop_result(C, st); };
    bspgemm_context::StatSlot &slot = ctx->slots[ctx->slot_head];
    const int R = C->rows;
    hipStream_t s = ctx->stream;
    const int *Bcol = B->gather_col();                     // B.col_idx, or its padded copy (the extents in ab[] point into it)

    // ---- symbolic 1: per-row products, their prefix, capacity classes ---------------------
    const int scan_tiles = (R + 2047) / 2048;
    const int heavy_cols = B->cols > 0 ? B->cols : 1;
    launch_scan_and_bin(ctx->F, R, row_begin, A->d_row_ptr, ctx->Fprefix, ctx->partials, ctx->bin_tiles,
                        ctx->bin_count, ctx->rec, ctx->recpre, ctx->cnt, heavy_cols, ctx->hpartials, mid_cap_for_cols(B->cols), rank_cap_for_cols(B->cols), 0, s);
    HostScalars *h = ctx->h;
    HIPCHK_B(hipMemcpyAsync(&h->totalF, ctx->Fprefix + R, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipMemcpyAsync(&h->heavy_total, ctx->hpartials + scan_tiles, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipMemcpyAsync(h->bin_count, ctx->bin_count, kNumBins * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipMemcpyAsync(&h->a_lo, A->d_row_ptr + row_begin, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipMemcpyAsync(&h->a_hi, A->d_row_ptr + row_end, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipEventRecord(slot.ev[1], s));
    HIPCHK_B(hipStreamSynchronize(s));
    const long long totalF = R > 0 ? h->totalF : 0;
    if (R == 0) { memset(h->bin_count, 0, sizeof h->bin_count); h->heavy_total = 0; }
    if (bspgemm_status st = ensure_tmp(ctx, (size_t)h->heavy_total + 1)) return bail(st);
    int cls_n[2][kNumBins] = {};

    // ---- symbolic 2: exact |C_i| of every row, scanned into C.row_ptr -----------------------
    if (R > 0) {
        // the numeric kernel without its emit half: |C_i| = F_i as soon as every product is seen to sit alone in its
        // 32-column slot, the level-0 masks are only built and counted for the other rows.  The heavy rows are
        // accumulated and read out into their workspace (offsets in recpre)
        auto count = [&](int b, int n, const RowRec *rec, const long long *recpre, hipStream_t sx) {
            hub_order(ctx, b, n, rec, recpre, sx);
            return launch_class(b, ctx->ab, Bcol, B->gather_nnz(), B->cols, rec, recpre, n, row_begin, ctx->tmp, ctx->cnt,
                                ctx->d_err, MaskMode::None, nullptr, nullptr, sx, true);
        };
        if (bspgemm_status st = class_phase(ctx, 0, totalF, cls_n[0], false, count)) return bail(st);
        launch_scan_counts(ctx->cnt, R, C->d_row_ptr, ctx->partials, nullptr, s);
    } else {
        HIPCHK_B(hipMemsetAsync(C->d_row_ptr, 0, sizeof(long long), s));
    }
    HIPCHK_B(hipMemcpyAsync(&h->nnzC, C->d_row_ptr + R, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipEventRecord(slot.ev[2], s));

    // C.col_idx: nnz(C) <= F entries are needed.  A cached buffer that holds F entries is taken
    // without waiting for nnz(C); otherwise the size is read back and exactly that is allocated
    // (or F itself, col_cap_for).  Development (BSPGEMM_OPT_CHECK): never emit on unverified sizes.
    if (!ctx->check && result_cached(ctx, result_bytes_colidx(totalF))) {
        HIPCHK_B(alloc_col_idx(ctx, C, totalF));
    } else {
        HIPCHK_B(hipStreamSynchronize(s));
        if (h->nnzC < 0 || h->nnzC > totalF) return bail(FAIL(BSPGEMM_ERR_HIP, "symbolic pass counted more outputs than products"));
        HIPCHK_B(alloc_col_idx(ctx, C, col_cap_for(totalF, h->nnzC)));
    }

    // ---- numeric: every row emitted at its final place; the heavy rows' move runs beside the class launches on the third stream
    if (R > 0) {
        const int levels = wave_levels_for_cols(B->cols);
        auto emit = [&](int b, int n, const RowRec *rec, const long long *recpre, hipStream_t sx) {
            if (b <= kWaveBins)
                return launch_wave_rows(b, levels, ctx->ab, Bcol, B->cols, rec, recpre, C->d_row_ptr, n, row_begin,
                                        C->d_col_idx, nullptr, ctx->d_err, MaskMode::None, nullptr, nullptr, sx, false,
                                        ctx->shared_slots);
            launch_place_heavy(ctx->tmp, rec, recpre, n, C->d_row_ptr, row_begin, C->d_col_idx, sx);
            return hipSuccess;
        };
        if (bspgemm_status st = class_phase(ctx, 1, totalF, cls_n[1], true, emit)) return bail(st);
    }
    HIPCHK_B(hipEventRecord(slot.ev[3], s));
    if (R > 0) {                                           // the heavy rows' move (third stream)
        HIPCHK_B(hipEventRecord(ctx->ev_join, ctx->stream_c));
        HIPCHK_B(hipStreamWaitEvent(s, ctx->ev_join, 0));
    }
    return finish_flow(ctx, C, B, totalF, rank_cap_for_cols(B->cols), cls_n, out);
}


// C = A*B (mode None, Fm NULL), C = F .* (A*B) (Keep), C = !F .* (A*B) (Drop) or C = D | (A*B) (Insert, Fm = D), rows placed
// in an upper-bound workspace and squeezed together by the compaction kernel once the counts are scanned.  Keep: the mask
// bounds a row (|C_i| <= |F_i|), usually far below its product count, so rows are binned and placed by MASK length.  Drop:
// the mask bounds nothing (|C_i| <= min(F_i, cols) still), so rows are binned, placed and ordered exactly as unmasked, and
// each class runs the drop twin of its kernel.  Insert: D's row is gathered like one more B row, so rows are binned and
// placed by F_i + |D_i| (|C_i| <= min(F_i + |D_i|, cols)) -- a row without products but with a row of D is a record too --
// and each class runs the accumulate twin of its kernel.  Count: Keep's sizes, bins and placement, the counting twin of
// every kernel, and a second workspace (tmpv) that holds each row's counts at the offsets of its columns in tmp and goes
// through the same compaction into the result's values.
static bspgemm_status multiply_upper_bound(bspgemm_context *ctx, const bspgemm_matrix *A,
                                           const bspgemm_matrix *B, const bspgemm_matrix *Fm, MaskMode mode,
                                           int row_begin, int row_end, bspgemm_result **out)
{
    const bool count = mode == MaskMode::Count;
    const bool keep = mode == MaskMode::Keep || count, insert = mode == MaskMode::Insert;
    bspgemm_result *C = nullptr;
    if (bspgemm_status st = start_flow(ctx, A, B, Fm, row_begin, row_end, BSPGEMM_FLOW_UPPER_BOUND, out, &C)) return st;
    auto bail = [&](bspgemm_status st) { return drop_result(C, st); };
    bspgemm_context::StatSlot &slot = ctx->slots[ctx->slot_head];
    const int R = C->rows;
    hipStream_t s = ctx->stream;
    const int *Bcol = B->gather_col();                     // B.col_idx, or its padded copy (the extents in ab[] point into it)
    HostScalars *h = ctx->h;
    h->products = 0;
    // rows are classified by their products and placed by min(products, B.cols) -- or, masked (Keep), both by
    // the mask row's length (|C_i| <= |F_i|), or, accumulating (Insert), by products + |D_i|; the true product count is
    // summed separately
    const long long *size_by = ctx->F;
    if (count) {
        HIPCHK_B(hipMemsetAsync(&ctx->d_prep->max_f, 0, sizeof ctx->d_prep->max_f, s));
        launch_mask_lengths_count(ctx->F, Fm->d_row_ptr, row_begin, R, ctx->Fmask, &ctx->d_prep->max_f, s);
        size_by = ctx->Fmask;
    } else if (keep) {
        launch_mask_lengths(ctx->F, Fm->d_row_ptr, row_begin, R, ctx->Fmask, s);
        size_by = ctx->Fmask;
    } else if (insert) {
        launch_insert_lengths(ctx->F, Fm->d_row_ptr, row_begin, R, ctx->Fmask, s);
        size_by = ctx->Fmask;
    }
    launch_scan_and_bin(size_by, R, row_begin, A->d_row_ptr, ctx->Fprefix, ctx->partials, ctx->bin_tiles,
                        ctx->bin_count, ctx->rec, ctx->recpre, ctx->cnt, 0, ctx->hpartials, mid_cap_for_cols(B->cols),
                        keep ? 0 : rank_cap_for_cols(B->cols), B->cols > 0 ? B->cols : 1, s, ctx->d_prep,
                        keep || insert ? ctx->F : nullptr);
    HIPCHK_B(hipMemcpyAsync(&h->prep, ctx->d_prep, sizeof(PrepScalars), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipEventRecord(slot.ev[1], s));
    HIPCHK_B(hipStreamSynchronize(s));
    h->totalF = h->prep.totalF;
    h->products = h->prep.products;
    h->a_lo = h->prep.a_lo;
    h->a_hi = h->prep.a_hi;
    memcpy(h->bin_count, h->prep.bin_count, sizeof h->bin_count);
    const long long total = R > 0 ? h->totalF : 0;         // sum of min(products, cols) (Keep: of mask-row lengths, Insert: of
                                                           // products + |D_i|): bounds nnz(C)
    if (R == 0) memset(h->bin_count, 0, sizeof h->bin_count);
    // a count is at most its row's product count: refused before any kernel of the numeric phase when that can exceed int32
    if (count && R > 0 && h->prep.max_f > (unsigned long long)INT_MAX)
        return bail(FAIL(BSPGEMM_ERR_OVERFLOW, "a row has more than INT_MAX products: its counts may not fit int32"));
    if (bspgemm_status st = ensure_tmp(ctx, (size_t)total + 1)) return bail(st);
    if (count)
        if (bspgemm_status st = ensure_tmpv(ctx, (size_t)total + 1)) return bail(st);
    if (bspgemm_status st = ensure_chunk_rows(ctx, compact_chunk_rows(total))) return bail(st);
    // C.col_idx: a cached buffer of the upper-bound size is taken now (nothing to wait for); else it
    // is allocated with exactly nnz(C) entries once the counts are scanned
    if (result_cached(ctx, result_bytes_colidx(total))) HIPCHK_B(alloc_col_idx(ctx, C, total));
    HIPCHK_B(hipEventRecord(slot.ev[2], s));               // no count phase here: ev[1]..ev[2] is the host's turn-around

    int cls_n[2][kNumBins] = {};
    if (R > 0) {
        const int *Frow = Fm ? Fm->d_row_ptr : nullptr, *Fcol = Fm ? Fm->d_col_idx : nullptr;
        auto place = [&](int b, int n, const RowRec *rec, const long long *recpre, hipStream_t sx) {
            if (!keep) hub_order(ctx, b, n, rec, recpre, sx);
            return launch_class(b, ctx->ab, Bcol, B->gather_nnz(), B->cols, rec, recpre, n, row_begin, ctx->tmp, ctx->cnt,
                                ctx->d_err, mode, Frow, Fcol, sx, false, count ? ctx->tmpv : nullptr, ctx->shared_slots);
        };
        if (bspgemm_status st = class_phase(ctx, 1, h->products, cls_n[1], false, place)) return bail(st);
        HIPCHK_B(hipEventRecord(slot.ev[3], s));
        launch_scan_counts(ctx->cnt, R, C->d_row_ptr, ctx->partials, nullptr, s, ctx->chunk_row);
    } else {
        HIPCHK_B(hipMemsetAsync(C->d_row_ptr, 0, sizeof(long long), s));
        HIPCHK_B(hipEventRecord(slot.ev[3], s));
    }
    HIPCHK_B(hipMemcpyAsync(&h->nnzC, C->d_row_ptr + R, sizeof(long long), hipMemcpyDeviceToHost, s));
    if (!C->d_col_idx) {
        HIPCHK_B(hipStreamSynchronize(s));
        HIPCHK_B(alloc_col_idx(ctx, C, col_cap_for(total, h->nnzC)));
    }
    if (count)                                             // as many entries as C.col_idx
        HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&C->d_values), result_bytes_colidx(C->col_cap)));
    if (R > 0) {
        launch_compact(ctx->tmp, ctx->Fprefix, C->d_row_ptr, 0, R, total, C->d_col_idx, s, ctx->chunk_row);
        if (count)                                         // the counts take the same row shifts as the columns
            launch_compact(ctx->tmpv, ctx->Fprefix, C->d_row_ptr, 0, R, total, C->d_values, s, ctx->chunk_row);
        HIPCHK_B(hipGetLastError());
    }
    return finish_flow(ctx, C, B, R > 0 ? h->products : 0, keep ? 0 : rank_cap_for_cols(B->cols), cls_n, out);
}

// Small products (csrc/small.hip): five launches, no size goes to the host before the end, ONE read-back.  *bailed = true
// (status OK, no result) when the device found that the product does not fit the path: the caller runs the general flow.
static bool small_eligible(const bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, int R)
{
    if (ctx->small == 0 || R <= 0 || R > kSmallMaxRows || A->nnz > kSmallMaxNnzA) return false;
    if (ctx->small == 1) return true;
    // automatic: expected products = A's nonzeros x B's mean row length must leave room below the path's capacity
    const double mean_b = B->rows > 0 ? (double)B->nnz / (double)B->rows : 0.0;
    return (double)A->nnz * mean_b <= 0.5 * kSmallMaxProducts;
}

static bspgemm_status multiply_small(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                     int row_begin, int row_end, bspgemm_result **out, bool *bailed)
{
    *bailed = false;
    if (!out) return FAIL(BSPGEMM_ERR_INVALID, "result pointer is NULL");
    *out = nullptr;
    if (bspgemm_status st = check_operands(ctx, A, B, row_begin, row_end)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    const int R = row_end - row_begin;
    hipStream_t s = ctx->stream;
    if (bspgemm_status st = ensure_rows(ctx, (size_t)R + 1)) return st;
    if (bspgemm_status st = ensure_tmp(ctx, (size_t)kSmallMaxProducts + 1)) return st;
    bspgemm_result *C = new (std::nothrow) bspgemm_result{ctx, R, 0, nullptr, nullptr, 0};
    if (!C) return FAIL(BSPGEMM_ERR_ALLOC, "result");
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_result_free(C);
        return st;
    };
    // (the upper-bound flow's kind: rows are placed by their product count and squeezed together)
    bspgemm_context::StatSlot &slot = open_slot(ctx, BSPGEMM_FLOW_UPPER_BOUND, true);
    slot.prepass_kernel = 2;
    slot.padded = false;                                   // (B.col_idx itself: the path never builds the padded copy)
    HIPCHK_B(hipEventRecord(slot.ev[0], s));
    HIPCHK_B(result_alloc(ctx, reinterpret_cast<void **>(&C->d_row_ptr), result_bytes_rowptr(R)));
    HIPCHK_B(alloc_col_idx(ctx, C, kSmallMaxProducts));
    launch_small(A->d_row_ptr, A->d_col_idx, B->d_row_ptr, B->d_col_idx, row_begin, R, ctx->F, ctx->Fprefix,
                 reinterpret_cast<int *>(ctx->rec), ctx->cnt, ctx->tmp, C->d_row_ptr, C->d_col_idx, ctx->d_small_tiles, ctx->d_small, s);
    HIPCHK_B(hipGetLastError());
    HostScalars *h = ctx->h;
    HIPCHK_B(hipMemcpyAsync(&h->small, ctx->d_small, sizeof(SmallScalars), hipMemcpyDeviceToHost, s));
    for (int e = 1; e <= 4; e++) HIPCHK_B(hipEventRecord(slot.ev[e], s));   // one phase: everything is "total"
    HIPCHK_B(hipStreamSynchronize(s));
    if (h->small.bail) {
        // the attempt is no multiply of its own: its stat slot goes back, the general flow opens the same one again
        ctx->slot_head = (ctx->slot_head + bspgemm_context::kStatSlots - 1) % bspgemm_context::kStatSlots;
        bspgemm_result_free(C);
        *bailed = true;
        return BSPGEMM_OK;
    }
    C->nnz = h->small.nnzC;
    h->totalF = h->small.totalF;
    h->nnzC = h->small.nnzC;
    h->a_lo = h->small.a_lo;
    h->a_hi = h->small.a_hi;
    memset(h->bin_count, 0, sizeof h->bin_count);
    h->bin_count[0] = R - h->small.nonempty;               // (one "class": every non-empty row is sorted by one wave)
    h->bin_count[kWaveBins] = h->small.nonempty;
    int cls_n[2][kNumBins] = {};
    close_slot(ctx, R, h, h->small.totalF, C->nnz, cls_n, mid_cap_for_cols(B->cols));
    *out = C;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_multiply(bspgemm_context *ctx, const bspgemm_matrix *A,
                                           const bspgemm_matrix *B, int row_begin, int row_end,
                                           bspgemm_result **out)
{
    // Two ways to the same CSR (tuning): "exact" sizes every row first (symbolic
    // count pass) and emits at the final place: C.col_idx is nnz(C) entries and there is no workspace
    // of F entries; "upper-bound" places rows by their product count and squeezes them together
    // afterwards: faster where duplicates are rare (the compaction streams at HBM rate, the count
    // pass costs most of a numeric pass), but it holds 2F entries.  Default: upper-bound, and exact
    // when that does not fit.
    if (!ctx) return FAIL(BSPGEMM_ERR_INVALID, "ctx is NULL");
    if (A && B && ctx->flow != BSPGEMM_FLOW_EXACT && small_eligible(ctx, A, B, row_end - row_begin)) {
        bool bailed = false;
        const bspgemm_status st = multiply_small(ctx, A, B, row_begin, row_end, out, &bailed);
        if (st != BSPGEMM_OK || !bailed) return st;        // done (or failed); a product that did not fit falls through
    }
    if (ctx->flow == BSPGEMM_FLOW_EXACT) return multiply_exact(ctx, A, B, row_begin, row_end, out);
    bspgemm_status st = multiply_upper_bound(ctx, A, B, nullptr, MaskMode::None, row_begin, row_end, out);
    if (st == BSPGEMM_ERR_ALLOC && ctx->flow == BSPGEMM_FLOW_AUTO) {
        (void)hipGetLastError();
        st = multiply_exact(ctx, A, B, row_begin, row_end, out);
    }
    return st;
}


extern "C" bspgemm_status bspgemm_multiply_masked(bspgemm_context *ctx, const bspgemm_matrix *A,
                                                  const bspgemm_matrix *B, const bspgemm_matrix *F,
                                                  int row_begin, int row_end, bspgemm_result **out)
{
    if (!F) {
        if (out) *out = nullptr;
        return FAIL(BSPGEMM_ERR_INVALID, "mask is NULL");
    }
    return multiply_upper_bound(ctx, A, B, F, MaskMode::Keep, row_begin, row_end, out);
}

extern "C" bspgemm_status bspgemm_multiply_masked_ex(bspgemm_context *ctx, const bspgemm_matrix *A,
                                                     const bspgemm_matrix *B, const bspgemm_matrix *F, unsigned flags,
                                                     int row_begin, int row_end, bspgemm_result **out)
{
    if (flags & ~BSPGEMM_MASK_COMPLEMENT) {
        if (out) *out = nullptr;
        return FAIL(BSPGEMM_ERR_INVALID, "unknown mask flags");
    }
    if (!(flags & BSPGEMM_MASK_COMPLEMENT)) return bspgemm_multiply_masked(ctx, A, B, F, row_begin, row_end, out);
    if (!F) {
        if (out) *out = nullptr;
        return FAIL(BSPGEMM_ERR_INVALID, "mask is NULL");
    }
    return multiply_upper_bound(ctx, A, B, F, MaskMode::Drop, row_begin, row_end, out);
}

extern "C" bspgemm_status bspgemm_multiply_masked_count(bspgemm_context *ctx, const bspgemm_matrix *A,
                                                        const bspgemm_matrix *B, const bspgemm_matrix *F,
                                                        int row_begin, int row_end, bspgemm_result **out)
{
    if (!F) {
        if (out) *out = nullptr;
        return FAIL(BSPGEMM_ERR_INVALID, "mask is NULL");
    }
    return multiply_upper_bound(ctx, A, B, F, MaskMode::Count, row_begin, row_end, out);
}

extern "C" bspgemm_status bspgemm_multiply_accumulate(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B,
                                                      const bspgemm_matrix *D, int row_begin, int row_end, bspgemm_result **out)
{
    if (out) *out = nullptr;
    if (!ctx || !A || !B || !D || !out) return FAIL(BSPGEMM_ERR_INVALID, "NULL argument");
    if (D->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "D belongs to another context");
    if (D->rows < row_end) return FAIL(BSPGEMM_ERR_INVALID, "D has fewer rows than the row range needs");
    if (D->cols > B->cols) return FAIL(BSPGEMM_ERR_INVALID, "D has more columns than B");
    return multiply_upper_bound(ctx, A, B, D, MaskMode::Insert, row_begin, row_end, out);
}

// --------------------------------------------------------------- gathered lengths -> row_ptr -
extern "C" bspgemm_status bspgemm_lengths_to_row_ptr(bspgemm_context *ctx, const int *d_lengths, int nranks, int width,
                                                     const int *bounds, int64_t *d_row_ptr, void *hip_stream)
{
    if (!ctx || !d_lengths || !bounds || !d_row_ptr || nranks < 1 || width < 0 || bounds[0] != 0)
        return FAIL(BSPGEMM_ERR_INVALID, "lengths_to_row_ptr");
    for (int r = 0; r < nranks; r++)
        if (bounds[r + 1] < bounds[r] || bounds[r + 1] - bounds[r] > width) return FAIL(BSPGEMM_ERR_INVALID, "bounds");
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);      // NULL is HIP's default stream, as for any launch
    // own scan scratch: this may run on another stream than a multiply that is using ctx->partials
    const size_t need = (size_t)width / 2048 + 2;
    if (need > ctx->stitch_partials_cap) {
        if (ctx->stitch_partials) HIPCHK(dev_free(ctx->stitch_partials));
        ctx->stitch_partials = nullptr;
        ctx->stitch_partials_cap = 0;
        HIPCHK(dev_alloc(&ctx->stitch_partials, need * sizeof(long long)));
        ctx->stitch_partials_cap = need;
    }
    long long *out = reinterpret_cast<long long *>(d_row_ptr);
    for (int r = 0; r < nranks; r++)          // shard r continues the row_ptr where shard r-1 ended
        launch_scan_counts(d_lengths + (size_t)r * width, bounds[r + 1] - bounds[r], out + bounds[r],
                           ctx->stitch_partials, r == 0 ? nullptr : out + bounds[r], s);
    HIPCHK(hipGetLastError());
    return BSPGEMM_OK;
}

// ------------------------------------------------------------------ products as operands -
extern "C" bspgemm_status bspgemm_matrix_from_result(bspgemm_context *ctx, const bspgemm_result *C, int cols,
                                                     bspgemm_matrix **out)
{
    if (!ctx || !C || !out || cols < 0 || C->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "matrix_from_result");
    *out = nullptr;
    if (C->nnz > INT_MAX) return FAIL(BSPGEMM_ERR_OVERFLOW, "product has more than INT_MAX nonzeros: not usable as an int32 operand");
    if (bspgemm_status st = use_device(ctx)) return st;
    bspgemm_matrix *m = nullptr;
    auto bail = [&](bspgemm_status st) { bspgemm_matrix_free(m); return st; };
    if (bspgemm_status st = operand_new(ctx, C->rows, cols, &m)) return bail(st);
    if (bspgemm_status st = operand_cols(m, C->nnz)) return bail(st);
    launch_narrow_row_ptr(C->d_row_ptr, m->d_row_ptr, C->rows + 1, ctx->stream);
    if (C->nnz > 0)
        HIPCHK_B(hipMemcpyAsync(m->d_col_idx, C->d_col_idx, (size_t)C->nnz * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    if (bspgemm_status st = operand_finish(m, C->nnz)) return bail(st);
    HIPCHK_B(hipStreamSynchronize(ctx->stream));
    *out = m;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_closure(bspgemm_context *ctx, const bspgemm_matrix *A, int max_iter,
                                          bspgemm_result **T, int *iterations)
{
    if (!ctx || !A || !T || A->ctx != ctx || A->rows != A->cols) return FAIL(BSPGEMM_ERR_INVALID, "closure needs a square matrix");
    *T = nullptr;
    if (iterations) *iterations = 0;
    if (max_iter < 1) max_iter = 1;
    if (A->nnz + (long long)A->rows > INT_MAX) return FAIL(BSPGEMM_ERR_OVERFLOW, "A or I exceeds int32 nonzeros");
    if (bspgemm_status st = use_device(ctx)) return st;
    const int n = A->rows;
    bspgemm_matrix *cur = nullptr;                      // T0 = A | I
    {
        auto bail = [&](bspgemm_status st) { bspgemm_matrix_free(cur); return st; };
        if (bspgemm_status st = operand_new(ctx, n, n, &cur)) return bail(st);
        if (bspgemm_status st = operand_cols(cur, A->nnz + n)) return bail(st);
        launch_add_diagonal(A->d_row_ptr, A->d_col_idx, n, cur->d_row_ptr, cur->d_col_idx, ctx->stream);
        if (bspgemm_status st = operand_finish(cur, A->nnz + n)) return bail(st);
        HIPCHK_B(hipStreamSynchronize(ctx->stream));
    }
    long long prev_nnz = -1;      // nnz of the deduplicated T(k); unknown for T0 (may hold duplicates)
    bspgemm_result *C = nullptr;
    bspgemm_status st = BSPGEMM_OK;
    for (int it = 0; it < max_iter; it++) {
        bspgemm_result *next = nullptr;
        st = bspgemm_multiply(ctx, cur, cur, 0, n, &next);
        if (st) break;
        if (iterations) *iterations = it + 1;
        bspgemm_result_free(C);
        C = next;
        if (C->nnz == prev_nnz) break;                  // T*T == T: fixpoint (T contains I, so T <= T*T)
        prev_nnz = C->nnz;
        if (it + 1 == max_iter) break;
        bspgemm_matrix *nm = nullptr;
        st = bspgemm_matrix_from_result(ctx, C, n, &nm);
        if (st) break;
        bspgemm_matrix_free(cur);
        cur = nm;
    }
    bspgemm_matrix_free(cur);
    if (st) { bspgemm_result_free(C); return st; }
    *T = C;
    return BSPGEMM_OK;
}

// Transitive closure A+ (paths of length >= 1): T0 = A, T(k+1) = T(k) | T(k)*T(k) through the accumulating product, until
// nnz stops growing -- T(k) only grows, so equal nnz is equal sets.  The first step never ends it: T0 may hold repeats.
static bspgemm_status closure_transitive(bspgemm_context *ctx, const bspgemm_matrix *A, int max_iter, bspgemm_result **T,
                                         int *iterations)
{
    if (!ctx || !A || !T || A->ctx != ctx || A->rows != A->cols) return FAIL(BSPGEMM_ERR_INVALID, "closure needs a square matrix");
    *T = nullptr;
    if (iterations) *iterations = 0;
    if (max_iter < 1) max_iter = 1;
    if (bspgemm_status st = use_device(ctx)) return st;
    const int n = A->rows;
    const bspgemm_matrix *cur = A;                      // T(k) as an operand (T0: A itself, not owned)
    bspgemm_matrix *owned = nullptr;
    long long prev_nnz = -1;
    bspgemm_result *C = nullptr;
    bspgemm_status st = BSPGEMM_OK;
    for (int it = 0; it < max_iter; it++) {
        bspgemm_result *next = nullptr;
        st = bspgemm_multiply_accumulate(ctx, cur, cur, cur, 0, n, &next);
        if (st) break;
        if (iterations) *iterations = it + 1;
        bspgemm_result_free(C);
        C = next;
        if (C->nnz == prev_nnz) break;                  // T | T*T == T: fixpoint
        prev_nnz = C->nnz;
        if (it + 1 == max_iter) break;
        bspgemm_matrix *nm = nullptr;
        st = bspgemm_matrix_from_result(ctx, C, n, &nm);
        if (st) break;
        bspgemm_matrix_free(owned);
        owned = nm;
        cur = nm;
    }
    bspgemm_matrix_free(owned);
    if (st) { bspgemm_result_free(C); return st; }
    *T = C;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_closure_ex(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags, int max_iter,
                                             bspgemm_result **T, int *iterations)
{
    if (T) *T = nullptr;
    if (flags & ~BSPGEMM_CLOSURE_TRANSITIVE) return FAIL(BSPGEMM_ERR_INVALID, "unknown closure flags");
    if (flags & BSPGEMM_CLOSURE_TRANSITIVE) return closure_transitive(ctx, A, max_iter, T, iterations);
    return bspgemm_closure(ctx, A, max_iter, T, iterations);
}

// ------------------------------------------------------------------ sharding helper ------
extern "C" bspgemm_status bspgemm_row_work_prefix(bspgemm_context *ctx, const bspgemm_matrix *A,
                                                  const bspgemm_matrix *B, int64_t *prefix_host)
{
    if (!prefix_host) return FAIL(BSPGEMM_ERR_INVALID, "prefix_host is NULL");
    if (bspgemm_status st = check_operands(ctx, A, B, 0, A ? A->rows : 0)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    const int R = A->rows;
    if (bspgemm_status st = ensure_rows(ctx, (size_t)R + 1)) return st;
    if (bspgemm_status st = ensure_deg8(B)) return st;
    launch_row_products(A->d_row_ptr, A->d_col_idx, B->d_row_ptr, B->d_deg8, 0, R, ctx->F, ctx->stream);
    launch_scan_and_bin(ctx->F, R, 0, A->d_row_ptr, ctx->Fprefix, ctx->partials, ctx->bin_tiles, ctx->bin_count,
                        ctx->rec, ctx->recpre, ctx->cnt, 0, nullptr, mid_cap_for_cols(B->cols), rank_cap_for_cols(B->cols), 0, ctx->stream);
    HIPCHK(hipMemcpyAsync(prefix_host, ctx->Fprefix, ((size_t)R + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_partition_rows(bspgemm_context *ctx, const bspgemm_matrix *A,
                                                 const bspgemm_matrix *B, int parts, int *bounds)
{
    if (!bounds || parts <= 0 || !A) return FAIL(BSPGEMM_ERR_INVALID, "partition_rows");
    const int R = A->rows;
    int64_t *prefix = static_cast<int64_t *>(malloc(((size_t)R + 1) * sizeof(int64_t)));
    if (!prefix) return FAIL(BSPGEMM_ERR_ALLOC, "prefix");
    bspgemm_status st = bspgemm_row_work_prefix(ctx, A, B, prefix);
    if (st == BSPGEMM_OK) {
        // cost of a row = its products + a constant for the per-row overhead
        const long long per_row = 32;
        const long long total = prefix[R] + per_row * R;
        bounds[0] = 0;
        int r = 0;
        for (int p = 1; p < parts; p++) {
            const long long target = total / parts * p;
            while (r < R && prefix[r] + per_row * r < target) r++;
            bounds[p] = r;
        }
        bounds[parts] = R;
    }
    free(prefix);
    return st;
}

