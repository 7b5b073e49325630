// dropin.hip -- the int32 drop-ins with the reference's own argument lists and ownership rules:
// SpGEMM_hip <-> SpGEMM_omp (final/SpGEMM_mpi_omp.c:71-74), SpGEMM_hip_bigslice <-> SpGEMM_bigslice (:15-18),
// SpGEMM_hip_mat <-> SpGEMM_mat (Matlab/inc/BSpGEMM.h:2-4), SpGEMM_hip_masked <-> SpGEMM_masked (:232-235).
// Host arrays in, malloc'ed / caller-owned host arrays out; everything in between is the native handle API.
#include "internal.hpp"
#include "early_dest.hpp"

#include <mutex>

using namespace bsp;

// ------------------------------------------------------------------ int32 drop-ins -------
static std::mutex g_dropin_mu;
static bspgemm_context *g_dropin_ctx = nullptr;
static int g_dropin_device = -1;

extern "C" int bspgemm_dropin_set_device(int device)
{
    std::lock_guard<std::mutex> lk(g_dropin_mu);
    if (g_dropin_ctx && g_dropin_device != device) {
        bspgemm_destroy(g_dropin_ctx);
        g_dropin_ctx = nullptr;
    }
    g_dropin_device = device;
    return BSPGEMM_OK;
}

static bspgemm_status dropin_ctx(bspgemm_context **out)
{
    if (!g_dropin_ctx) {
        int dev = g_dropin_device;
        if (dev < 0) {
            const char *e = getenv("BSPGEMM_DEVICE");
            dev = e ? atoi(e) : 0;
        }
        bspgemm_status st = bspgemm_create(dev, &g_dropin_ctx);
        if (st) return st;
        g_dropin_device = dev;
    }
    *out = g_dropin_ctx;
    return BSPGEMM_OK;
}

int dropin_fail(const char *fn, bspgemm_status st)
{
    fprintf(stderr, "%s: %s: %s\n", fn, bspgemm_status_string(st), bspgemm_last_error());
    return (int)st;
}

// A's rows [r0, r1) and B (brows x Bm) onto the device.  view_ok: A * A through the same host arrays (the reference's own
// call, :322) uploads once, B is a view of A's device copy.  On failure the caller frees whatever *A and *B hold.
bspgemm_status dropin_upload(bspgemm_context *ctx, const int *Acol, const int *Arow, int r0, int r1, const int *Bcol,
                             const int *Brow, int brows, int Bm, bool view_ok, bspgemm_matrix **A, bspgemm_matrix **B)
{
    if (bspgemm_status st = bspgemm_matrix_upload(ctx, r1 - r0, brows, Arow + r0, Acol, A)) return st;
    if (view_ok && Bcol == Acol && Brow == Arow && r0 == 0 && r1 >= brows)
        return bspgemm_matrix_wrap_device(ctx, brows, Bm, (long long)Brow[brows] - Brow[0], (*A)->d_row_ptr, (*A)->d_col_idx, B);
    return bspgemm_matrix_upload(ctx, brows, Bm, Brow, Bcol, B);
}

// ------------------------------------------------------------------ the shared body, in stages ---
// Whose memory the result's col_idx goes to.  Malloced: *Ccol = malloc(nnz), the caller frees it (SpGEMM_omp :115).
// CallerGrown: the caller's *Ccol of *Csize entries, realloc'ed when too small (bigslice :28-31).  CallerExact: the caller's
// buffer has the exact size (SpGEMM_mat).
enum class Dest { Malloced, CallerGrown, CallerExact };

// The pin hooks of the early destination.  hipHostRegister needs the device on the helper's own thread; g_dropin_device
// is the drop-in context's (the caller holds g_dropin_mu for the whole call).
static bool pin_piece(void *p, size_t bytes)
{
    if (hipSetDevice(g_dropin_device) == hipSuccess && hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
static void unpin_piece(void *p) { (void)hipHostUnregister(p); }

// Bytes of the early destination for an upper bound of nnz(C) (-1: none taken), 0: not to be used.  It is sized by the
// BOUND, which heavy merging can leave far above nnz(C): it is only used while it stays below half of the host memory that
// is free right now (and below INT_MAX entries); otherwise the result is malloc'ed with its true size after the multiply,
// as before.
static size_t early_bytes(long long bound)
{
    if (bound < 0 || bound > INT_MAX) return 0;
    const long pages = sysconf(_SC_AVPHYS_PAGES), psize = sysconf(_SC_PAGESIZE);
    if (pages > 0 && psize > 0 && (double)bound * sizeof(int) > 0.5 * (double)pages * (double)psize) return 0;
    return (size_t)(bound > 0 ? bound : 1) * sizeof(int);
}

// A destination allocated after the multiply (old: the caller's block to grow, or NULL).  A multi-GB block would be faulted
// in page by page inside the device-to-host copy: it gets huge pages and is touched from all host threads first (measured
// on a 5.3 GB result: download 425 -> 320 ms with the advice alone).
static int *alloc_late(int *old, size_t bytes)
{
    int *p = static_cast<int *>(realloc(old, bytes));
    if (!p || bytes < ((size_t)64 << 20)) return p;
    advise_huge_pages(p, bytes);
    bspgemm_par_prefault(p, bytes);
    return p;
}

// Stage 4: where col_idx goes, one policy per Dest; NULL: no memory.  *from_early: it is the early block, still owned by
// `early`, which otherwise has dropped its block here (before the late malloc).
static int *dropin_destination(Dest dest, int **Ccol, int *Csize, long long nnz, long long bound, EarlyDest &early, bool *from_early)
{
    const size_t entries = (size_t)(nnz > 0 ? nnz : 1);
    *from_early = false;
    switch (dest) {
    case Dest::Malloced:
        // the helper has malloc'ed (or failed) long before the multiply is over: block() waits for that one pointer
        if (early.block() && nnz <= bound) { *from_early = true; return early.block(); }
        early.drop();
        return alloc_late(nullptr, entries * sizeof(int));
    case Dest::CallerGrown:
        if (*Ccol && Csize && *Csize >= nnz) return *Ccol;
        if (int *grown = alloc_late(*Ccol, entries * sizeof(int))) {
            *Ccol = grown;                              // published at once: realloc has freed or moved the old block
            if (Csize) *Csize = (int)entries;
            return grown;
        }
        return nullptr;
    case Dest::CallerExact:
        break;
    }
    return *Ccol;
}

// Stage 5, early destination: col_idx piece by piece behind the helper, which is stopped once the last needed piece is
// queued (pieces beyond nnz(C) are abandoned).  A copy that fails after others were queued must not leave a DMA writing
// into memory that is about to be unpinned and freed: EVERY exit drains the stream first (early_dest.hpp).
static bspgemm_status download_early(bspgemm_context *ctx, const bspgemm_result *C, EarlyDest &early, int64_t *rp64)
{
    const size_t need = (size_t)C->nnz * sizeof(int), piece = early.piece;
    hipStream_t s = ctx->stream;
    char *dst = reinterpret_cast<char *>(early.block());
    auto queue = [&]() -> bspgemm_status {
        HIPCHK(hipMemcpyAsync(rp64, C->d_row_ptr, ((size_t)C->rows + 1) * sizeof(long long), hipMemcpyDeviceToHost, s));
        for (size_t k = 0, off = 0; off < need; k++, off += piece) {
            if (!early.wait_piece(k)) return FAIL(BSPGEMM_ERR_ALLOC, "early destination");
            const size_t len = (need - off < piece) ? need - off : piece;
            HIPCHK(hipMemcpyAsync(dst + off, reinterpret_cast<const char *>(C->d_col_idx) + off, len, hipMemcpyDeviceToHost, s));
        }
        return BSPGEMM_OK;
    };
    const bspgemm_status st = queue();
    early.stop();                                       // (joins the helper; nothing is unpinned yet)
    const hipError_t e = hipStreamSynchronize(s);
    if (st) return st;
    HIPCHK(e);
    return BSPGEMM_OK;
}

// Stages 4-6 for a finished product: destination, download, hand-over.  After a failure `early` still owns its block.
static bspgemm_status dropin_deliver(bspgemm_context *ctx, const bspgemm_result *C, Dest dest, int **Ccol, int *Crow, int *Csize,
                                     long long bound, EarlyDest &early)
{
    if (C->nnz > INT_MAX) return FAIL(BSPGEMM_ERR_OVERFLOW, "nnz(C) > INT_MAX: use the int64 handle API");
    bool from_early;
    int *dst = dropin_destination(dest, Ccol, Csize, C->nnz, bound, early, &from_early);
    int64_t *rp64 = static_cast<int64_t *>(malloc(((size_t)C->rows + 1) * sizeof(int64_t)));
    bspgemm_status st = (dst && rp64) ? BSPGEMM_OK : FAIL(BSPGEMM_ERR_ALLOC, "host result");
    if (!st) st = from_early ? download_early(ctx, C, early, rp64) : bspgemm_result_download(ctx, C, rp64, dst);
    if (!st) {                                          // hand-over (the stream is drained: the early block may be unpinned)
        dropin_crow(rp64, C->rows, Crow);
        *Ccol = from_early ? early.release((size_t)C->nnz * sizeof(int)) : dst;
    } else if (dest == Dest::Malloced && !from_early) {
        free(dst);
    }
    free(rp64);
    return st;
}

// Shared body: C rows [r0,r1) of A*B (masked by F when Frow is given) with host int32 arrays in the reference's
// conventions.  The call the reference's driver makes (:322: malloc'ed result, no mask) sizes the result by an upper bound
// from one host pass over A and has it faulted in and PINNED IN PLACE by EarlyDest's helper thread while the operands are
// uploaded and multiplied -- the download is then DMA at the link's rate into the caller's own memory.  (It used to be a
// pageable copy started after the multiply: 172 of 200 ms on BASELINE config 3, the 5.3 GB result moving at 31 GB/s.)
static bspgemm_status dropin_run(const int *Acol, const int *Arow, int r0, int r1, const int *Bcol, const int *Brow, int Bm,
                                 int **Ccol, int *Crow, int *Csize, Dest dest, const int *Fcol = nullptr, const int *Frow = nullptr)
{
    // ---- argument check and bound
    if (!Acol || !Arow || !Bcol || !Brow || !Crow || !Ccol || r0 < 0 || r1 < r0 || Bm < 0)
        return FAIL(BSPGEMM_ERR_INVALID, "drop-in arguments");
    std::lock_guard<std::mutex> lk(g_dropin_mu);
    bspgemm_context *ctx;
    if (bspgemm_status st = dropin_ctx(&ctx)) return st;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    const int rows = r1 - r0, brows = dropin_b_rows(Acol, Arow, r0, r1);
    const long long bound = (dest == Dest::Malloced && !Frow) ? bspgemm_par_output_bound(Acol, Arow, r0, r1, Brow, brows, Bm > 0 ? Bm : 1) : -1;
    const size_t ebytes = early_bytes(bound);
    const bool pin = ebytes >= ((size_t)1 << 20) && hipSetDevice(ctx->device) == hipSuccess;
    EarlyDest early(pin ? pin_piece : nullptr, pin ? unpin_piece : nullptr);
    if (ebytes) early.start(ebytes);
    const double t1 = now();
    // ---- operands: A, B (a view of A for A * A), the mask
    bspgemm_matrix *A = nullptr, *B = nullptr, *Fm = nullptr;
    bspgemm_result *C = nullptr;
    bspgemm_status st = dropin_upload(ctx, Acol, Arow, r0, r1, Bcol, Brow, brows, Bm, true, &A, &B);
    if (!st && Frow) st = bspgemm_matrix_upload(ctx, rows, Bm, Frow + r0, Fcol, &Fm);
    const double t2 = now();
    // ---- multiply
    if (!st) st = Fm ? bspgemm_multiply_masked(ctx, A, B, Fm, 0, rows, &C) : bspgemm_multiply(ctx, A, B, 0, rows, &C);
    const double t3 = now();
    // ---- destination, download, hand-over; an early block that was not handed over goes here (nothing is in flight)
    if (!st) st = dropin_deliver(ctx, C, dest, Ccol, Crow, Csize, bound, early);
    early.drop();
    const double t4 = now();
    bspgemm_result_free(C);
    bspgemm_matrix_free(A);
    bspgemm_matrix_free(B);
    bspgemm_matrix_free(Fm);
    if (ctx->dropin_timing)
        fprintf(stderr, "[bspgemm drop-in] scan A %.1f ms, upload %.1f, multiply %.1f, download %.1f, free %.1f\n",
                t1 - t0, t2 - t1, t3 - t2, t4 - t3, now() - t4);
    return st;
}

extern "C" int SpGEMM_hip(int *Acol, int *Arow, int An, int *Bcol, int *Brow, int Bm,
                          int **Ccol, int *Crow, int tBlock)
{
    (void)tBlock;
    if (Ccol) *Ccol = nullptr;
    bspgemm_status st = dropin_run(Acol, Arow, 0, An, Bcol, Brow, Bm, Ccol, Crow, nullptr, Dest::Malloced);
    return st ? dropin_fail("SpGEMM_hip", st) : 0;
}

extern "C" int SpGEMM_hip_bigslice(int *Acol, int *Arow, int An, int *Bcol, int *Brow, int Bm,
                                   int **Ccol, int *Crow, int *Csize, int start_row, int end_row)
{
    (void)An;
    bspgemm_status st = dropin_run(Acol, Arow, start_row, end_row, Bcol, Brow, Bm, Ccol, Crow, Csize, Dest::CallerGrown);
    return st ? dropin_fail("SpGEMM_hip_bigslice", st) : 0;
}

extern "C" int SpGEMM_hip_mat(int *Acol, int *Arow, int An, int *Bcol, int *Brow, int Bm,
                              int *Ccol, int *Crow)
{
    int *p = Ccol;
    bspgemm_status st = dropin_run(Acol, Arow, 0, An, Bcol, Brow, Bm, &p, Crow, nullptr, Dest::CallerExact);
    return st ? dropin_fail("SpGEMM_hip_mat", st) : 0;
}

extern "C" int SpGEMM_hip_masked(int *Acol, int *Arow, int An, int *Bcol, int *Brow, int Bm,
                                 int *Fcol, int *Frow, int **Ccol, int *Crow, int *Csize)
{
    if (!Fcol || !Frow) return dropin_fail("SpGEMM_hip_masked", FAIL(BSPGEMM_ERR_INVALID, "mask is NULL"));
    bspgemm_status st = dropin_run(Acol, Arow, 0, An, Bcol, Brow, Bm, Ccol, Crow, Csize, Dest::CallerGrown, Fcol, Frow);
    return st ? dropin_fail("SpGEMM_hip_masked", st) : 0;
}

