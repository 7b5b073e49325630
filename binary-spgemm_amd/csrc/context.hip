// context.hip -- the handle side of the C ABI (include/bspgemm.h): errors, the per-GPU context and its
// workspaces, device-resident operands, the builder of derived ones and their tables, the cache of freed result buffers,
// result accessors, statistics.  No CPU compute path exists in this library: without a gfx950 device
// every compute entry point fails with BSPGEMM_ERR_NO_DEVICE.
#include "internal.hpp"

#include <mutex>
#include <unordered_map>

using namespace bsp;

// ------------------------------------------------------------------ errors ---------------
thread_local char bspgemm_err_text[512] = "";

extern "C" const char *bspgemm_last_error(void) { return g_err; }

extern "C" const char *bspgemm_status_string(bspgemm_status s)
{
    switch (s) {
    case BSPGEMM_OK: return "ok";
    case BSPGEMM_ERR_INVALID: return "invalid argument";
    case BSPGEMM_ERR_ALLOC: return "allocation failed";
    case BSPGEMM_ERR_HIP: return "HIP runtime error";
    case BSPGEMM_ERR_NO_DEVICE: return "no gfx950 device (this library has no CPU fallback)";
    case BSPGEMM_ERR_OVERFLOW: return "result exceeds the int32 drop-in interface";
    case BSPGEMM_ERR_IO: return "file I/O error";
    case BSPGEMM_ERR_FORMAT: return "Matrix Market banner rejected";
    case BSPGEMM_ERR_SIZE: return "Matrix Market size line or entry rejected";
    case BSPGEMM_ERR_COMM: return "RCCL error";
    }
    return "unknown status";
}

// ------------------------------------------------------------------ device memory -------
// The one gate for device memory (internal.hpp: dev_alloc / dev_free): every array the library keeps on a GPU is allocated
// and freed here, so that the live set can be counted and the n-th request can be made to fail (include/bspgemm.h, "test
// hooks").  Process-wide and locked: contexts of several threads share it.  Off the timed path: a steady-state multiply
// allocates nothing (kept workspaces, result cache).  The state is never destroyed: the drop-in context may free after exit().
namespace {
constexpr int kHookFill = 1, kHookGuard = 2;
constexpr size_t kGuardZone = 256;                          // bytes in front of and behind a guarded allocation
constexpr int kGuardByte = 0xC5;                            // (neither byte of the two poison words of tests/test_gpu_dirty_state.py)
struct DevRec {
    size_t bytes;                                           // as requested: what live_bytes counts
    int guarded_on;                                         // -1: no zones; else the device whose memory it is
};
struct DevGate {
    std::mutex mu;
    std::unordered_map<void *, DevRec> live;
    long long requests = 0, live_bytes = 0, fired = 0, countdown = 0;
    int hooks = 0;                                          // kHookFill | kHookGuard: the one word a request reads under the lock
    uint32_t fill_word = 0;
    long long damaged_freed = 0;                            // guarded allocations that were freed with a changed zone (sticky)
    char first_damage[160] = "";
};
DevGate &dev_gate()
{
    static DevGate *g = new DevGate();
    return *g;
}

// `bytes` at p become copies of `word`; a trailing 1-3 bytes take its low bytes.  s NULL: the null stream.  No synchronisation.
hipError_t fill_words(void *p, size_t bytes, uint32_t word, hipStream_t s)
{
    if (!p || bytes == 0) return hipSuccess;
    const size_t words = bytes / 4;
    if (words)
        if (hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)word, words, s)) return e;
    for (size_t k = words * 4; k < bytes; k++)
        if (hipError_t e = hipMemsetAsync(static_cast<char *>(p) + k, (int)((word >> (8 * (k & 3))) & 0xff), 1, s)) return e;
    return hipSuccess;
}

// The zones of the guarded allocation whose caller pointer is p: 0 intact, 1 changed (*front, *off: the first changed
// byte), -1 the read-back failed.  The device is drained first: a store in flight counts.
int guard_zones_changed(const void *p, const DevRec &r, bool *front, int *off)
{
    unsigned char z[2 * kGuardZone];
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != r.guarded_on) (void)hipSetDevice(r.guarded_on);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(z, static_cast<const char *>(p) - kGuardZone, kGuardZone, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(z + kGuardZone, static_cast<const char *>(p) + r.bytes, kGuardZone, hipMemcpyDeviceToHost);
    if (cur != r.guarded_on) (void)hipSetDevice(cur);
    if (e != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (size_t k = 0; k < 2 * kGuardZone; k++)
        if (z[k] != (unsigned char)kGuardByte) {
            *front = k < kGuardZone;
            *off = (int)(k % kGuardZone);
            return 1;
        }
    return 0;
}

void note_damage(DevGate &g, const DevRec &r, int changed, bool front, int off)   // g.mu held
{
    if (g.first_damage[0]) return;
    if (changed < 0) snprintf(g.first_damage, sizeof g.first_damage, "guard zones of an allocation of %zu bytes could not be read back", r.bytes);
    else snprintf(g.first_damage, sizeof g.first_damage, "guard damaged: allocation of %zu bytes, %s zone, offset %d", r.bytes,
                  front ? "front" : "back", off);
}
}  // namespace

hipError_t dev_alloc_bytes(void **p, size_t bytes)
{
    DevGate &g = dev_gate();
    *p = nullptr;
    int hooks;
    uint32_t word;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.requests++;
        if (g.countdown > 0 && --g.countdown == 0) {        // the injected failure: no HIP call, no sticky HIP error
            g.fired++;
            return hipErrorOutOfMemory;
        }
        hooks = g.hooks;
        word = g.fill_word;
    }
    DevRec rec{bytes, -1};
    void *q = nullptr;
    if (hooks == 0 || bytes == 0) {                         // the plain request: hipMalloc and nothing else
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
    } else {                                                // test hooks (include/bspgemm.h): zones around it, poison inside
        const bool guard = hooks & kHookGuard;
        char *base = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), bytes + (guard ? 2 * kGuardZone : 0));
        if (e != hipSuccess) return e;
        q = guard ? base + kGuardZone : base;
        if (guard) {
            e = hipGetDevice(&rec.guarded_on);
            if (e == hipSuccess) e = hipMemsetAsync(base, kGuardByte, kGuardZone, nullptr);
            if (e == hipSuccess) e = hipMemsetAsync(base + kGuardZone + bytes, kGuardByte, kGuardZone, nullptr);
        }
        if (e == hipSuccess && (hooks & kHookFill)) e = fill_words(q, bytes, word, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { (void)hipFree(base); return e; }
    }
    if (q) {
        std::lock_guard<std::mutex> lk(g.mu);
        g.live[q] = rec;
        g.live_bytes += (long long)bytes;
    }
    *p = q;
    return hipSuccess;
}

hipError_t dev_free(void *p)
{
    if (!p) return hipSuccess;
    DevGate &g = dev_gate();
    DevRec rec{0, -1};
    {
        std::lock_guard<std::mutex> lk(g.mu);
        auto it = g.live.find(p);
        if (it != g.live.end()) {
            rec = it->second;
            g.live_bytes -= (long long)rec.bytes;
            g.live.erase(it);
        }
    }
    if (rec.guarded_on < 0) return hipFree(p);
    bool front = false;
    int off = 0;
    if (const int changed = guard_zones_changed(p, rec, &front, &off)) {
        std::lock_guard<std::mutex> lk(g.mu);
        g.damaged_freed++;
        note_damage(g, rec, changed, front, off);
    }
    return hipFree(static_cast<char *>(p) - kGuardZone);
}

// bytes of the live allocation at p as it was requested; 0: not the gate's (NULL, a wrapped array)
static size_t dev_alloc_size(const void *p)
{
    DevGate &g = dev_gate();
    std::lock_guard<std::mutex> lk(g.mu);
    auto it = g.live.find(const_cast<void *>(p));
    return it == g.live.end() ? 0 : it->second.bytes;
}

static void set_hook(int bit, bool on, uint32_t word)
{
    DevGate &g = dev_gate();
    std::lock_guard<std::mutex> lk(g.mu);
    if (bit == kHookGuard && on && !(g.hooks & kHookGuard)) {   // a new guarded stretch starts clean
        g.damaged_freed = 0;
        g.first_damage[0] = 0;
    }
    g.hooks = on ? (g.hooks | bit) : (g.hooks & ~bit);
    if (bit == kHookFill) g.fill_word = word;
}

extern "C" void bspgemm_debug_fill_alloc(int on, uint32_t word) { set_hook(kHookFill, on != 0, word); }
extern "C" void bspgemm_debug_guard_alloc(int on) { set_hook(kHookGuard, on != 0, 0); }

extern "C" int64_t bspgemm_debug_check_guards(void)
{
    DevGate &g = dev_gate();
    std::lock_guard<std::mutex> lk(g.mu);
    long long damaged = g.damaged_freed;
    for (const auto &kv : g.live) {
        if (kv.second.guarded_on < 0) continue;
        bool front = false;
        int off = 0;
        if (const int changed = guard_zones_changed(kv.first, kv.second, &front, &off)) {
            damaged++;
            note_damage(g, kv.second, changed, front, off);
        }
    }
    if (damaged) snprintf(g_err, sizeof g_err, "%s", g.first_damage);
    return damaged;
}

extern "C" void bspgemm_debug_fail_alloc(int nth)
{
    DevGate &g = dev_gate();
    std::lock_guard<std::mutex> lk(g.mu);
    g.countdown = nth > 0 ? nth : 0;
}

extern "C" void bspgemm_debug_alloc_state(int64_t out[4])
{
    if (!out) return;
    DevGate &g = dev_gate();
    std::lock_guard<std::mutex> lk(g.mu);
    out[0] = g.requests;
    out[1] = (int64_t)g.live.size();
    out[2] = g.live_bytes;
    out[3] = g.fired;
}

// Frees an operand's derived tables and forgets them: deg8 and the blocked table when `all`, the padded copy always.  The
// states and nnz_pad are the caller's.
static void drop_derived(const bspgemm_matrix *m, bool all)
{
    if (all) {
        dev_free(m->d_deg8);
        dev_free(m->d_blk16);
        m->d_deg8 = nullptr;
        m->d_blk16 = nullptr;
    }
    dev_free(m->d_col_pad); dev_free(m->d_row_ptr_pad); dev_free(m->d_ext);
    m->d_col_pad = nullptr; m->d_row_ptr_pad = nullptr; m->d_ext = nullptr;
}

bspgemm_status ensure_deg8(const bspgemm_matrix *m)
{
    if (m->d_deg8) return BSPGEMM_OK;
    HIPCHK(dev_alloc(&m->d_deg8, (size_t)m->rows + 1));
    launch_deg8(m->d_row_ptr, m->rows, m->d_deg8, m->ctx->stream);
    if (hipError_t e = hipGetLastError()) {                // (an unbuilt table must not pass for a built one)
        hipStreamSynchronize(m->ctx->stream);
        dev_free(m->d_deg8);
        m->d_deg8 = nullptr;
        HIPCHK(e);
    }
    return BSPGEMM_OK;
}

// The padded copy of B.col_idx (rows on 64-byte boundaries).  OPT-IN (BSPGEMM_OPT_PADDED_ROWS, default off): it cuts the
// bytes the gather moves by 22 % on the bench matrix (9.4 -> 7.3 GB, tools/gather_traffic_model.py) and the numeric phase by
// nothing there (3.336 -> 3.327 / 3.314 ms, profiles/r04_ab_padded_rows.log); with rows of exactly 16 entries (uniform
// matrices: every row is one aligned sector) it is worth 8-9 % of the numeric phase (profiles/r04_alignment_probe.log).
// Value -1 decides per operand: at least 2^20 nonzeros, a mean row length of 8 or more, the padded copy at most twice the
// original and below 2^31 entries.
bspgemm_status ensure_pad(const bspgemm_matrix *m)
{
    if (m->pad_state) return BSPGEMM_OK;
    m->pad_state = 2;
    bspgemm_context *ctx = m->ctx;
    const int force = ctx->pad_rows;
    if (force == 0 || m->rows <= 0 || m->nnz <= 0) return BSPGEMM_OK;
    if (force < 0 && (m->nnz < (1ll << 20) || m->nnz < 8ll * m->rows)) return BSPGEMM_OK;
    hipStream_t s = ctx->stream;
    const size_t rows = (size_t)m->rows;
    int *plen = nullptr;
    long long *pp64 = nullptr, *partials = nullptr;
    auto drop = [&] { dev_free(plen); dev_free(pp64); dev_free(partials); };
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        drop();
        drop_derived(m, false);
        if (st != BSPGEMM_OK) m->pad_state = 0;                // a failed build decides nothing: the next use as B tries again
        return st;
    };
    HIPCHK_B(dev_alloc(&plen, rows * sizeof(int)));
    HIPCHK_B(dev_alloc(&pp64, (rows + 1) * sizeof(long long)));
    HIPCHK_B(dev_alloc(&partials, (rows / 2048 + 4) * sizeof(long long)));
    launch_pad_lengths(m->d_row_ptr, m->rows, plen, s);
    launch_scan_counts(plen, m->rows, pp64, partials, nullptr, s);
    long long total = 0;
    HIPCHK_B(hipMemcpyAsync(&total, pp64 + rows, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));
    if (total > 0x7fffffffll - 64 || (force < 0 && total > 2 * m->nnz)) { drop(); return BSPGEMM_OK; }   // (stays "not for this operand")
    hipError_t e = dev_alloc(&m->d_col_pad, ((size_t)total + 64) * sizeof(int));
    if (e == hipSuccess) e = dev_alloc(&m->d_row_ptr_pad, (rows + 1) * sizeof(int));
    if (e == hipSuccess) e = dev_alloc(&m->d_ext, rows * sizeof(int2));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (force == 1) { snprintf(g_err, sizeof g_err, "padded copy of col_idx: %s", hipGetErrorString(e)); return bail(BSPGEMM_ERR_ALLOC); }
        (void)bail(BSPGEMM_OK);                                // optional: an operand that does not fit twice is simply not padded
        return BSPGEMM_OK;
    }
    launch_narrow_row_ptr(pp64, m->d_row_ptr_pad, m->rows + 1, s);
    launch_pad_copy(m->d_row_ptr, m->d_col_idx, m->d_row_ptr_pad, m->rows, m->d_col_pad, m->d_ext, s);
    HIPCHK_B(hipGetLastError());
    HIPCHK_B(hipStreamSynchronize(s));
    drop();
    m->nnz_pad = total;
    m->pad_state = 1;
    return BSPGEMM_OK;
}

// Whether products with `m` as B go through the blocked table.  It pays when B.row_ptr is several
// times an XCD's 4 MB L2 (R-MAT scale 22: 16.8 MB against a table of 4.2 MB) and the operand is not
// dominated by rows of 63+ nonzeros, whose lengths the table clamps: a quarter of the nonzeros in such
// rows at the most.  Measured at 2^21 rows (prepass phase, table forbidden / forced): R-MAT
// (0.30,0.25,0.25,0.20) edge factor 16, 0.4 % of the nonzeros in clamped rows, 0.52 / 0.30 ms; R-MAT
// (0.45,0.22,0.22,0.11) edge factor 4, 15 % (a third of the look-ups fall through to B.row_ptr),
// 0.33 / 0.14 ms.  Graph500 skew (77 %, nine look-ups of ten fall through) stays with B.row_ptr: the bound is
// a cautious one, on the upper quarter of its rows (the whole product does not fit a card) the forced table
// was faster as well, 0.22 / 0.06 ms.
// Decided once per operand: one 8-byte read-back when the table is built.
bspgemm_status ensure_blk16(const bspgemm_matrix *m)
{
    if (m->blk16_state) return BSPGEMM_OK;
    m->blk16_state = 2;
    const int force = m->ctx->rw_blk;                              // 0 never, 1 always, -1 decide per operand
    if (force == 0 || (force < 0 && m->rows < (1 << 21))) return BSPGEMM_OK;
    const size_t ints = (size_t)4 * (((size_t)m->rows + 15) / 16 + 1);   // 16-byte entries (hipMalloc aligns them), one spare
    hipStream_t s = m->ctx->stream;
    auto bail = [&](bspgemm_status st) {                           // a failed build decides nothing: the next use as B tries again
        hipStreamSynchronize(s);
        dev_free(m->d_blk16);
        m->d_blk16 = nullptr;
        m->blk16_state = 0;
        return st;
    };
    HIPCHK_B(dev_alloc(&m->d_blk16, (ints + 4) * sizeof(int)));
    unsigned long long *d_clamped = reinterpret_cast<unsigned long long *>(m->d_blk16 + ints);
    HIPCHK_B(hipMemsetAsync(d_clamped, 0, sizeof(unsigned long long), s));
    launch_blk16(m->d_row_ptr, m->pad_state == 1 ? m->d_row_ptr_pad : nullptr, m->rows, m->d_blk16, d_clamped, s);
    HIPCHK_B(hipGetLastError());
    unsigned long long clamped = 0;
    HIPCHK_B(hipMemcpyAsync(&clamped, d_clamped, sizeof(clamped), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));
    if (force == 1 || clamped * 4ull <= (unsigned long long)m->nnz) m->blk16_state = 1;
    return BSPGEMM_OK;
}

bspgemm_status use_device(bspgemm_context *ctx)
{
    HIPCHK(hipSetDevice(ctx->device));
    return BSPGEMM_OK;
}

extern "C" int bspgemm_device_count(void)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return ndev;
}

extern "C" bspgemm_status bspgemm_create(int device, bspgemm_context **out)
{
    if (!out) return FAIL(BSPGEMM_ERR_INVALID, "ctx is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return FAIL(BSPGEMM_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return FAIL(BSPGEMM_ERR_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_err, sizeof g_err, "device %d is %s; libbspgemm carries gfx950 code only", device,
                 prop.gcnArchName);
        return BSPGEMM_ERR_NO_DEVICE;
    }
    bspgemm_context *ctx = new (std::nothrow) bspgemm_context();
    if (!ctx) return FAIL(BSPGEMM_ERR_ALLOC, "context");
    auto bail = [&](bspgemm_status st) { bspgemm_destroy(ctx); return st; };   // (it takes a half-built context)
    ctx->device = device;
    HIPCHK_B(hipSetDevice(device));
    HIPCHK_B(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
    HIPCHK_B(hipHostMalloc(reinterpret_cast<void **>(&ctx->h), sizeof(HostScalars), hipHostMallocDefault));
    HIPCHK_B(dev_alloc(&ctx->d_prep, sizeof(PrepScalars)));
    HIPCHK_B(dev_alloc(&ctx->d_small, sizeof(SmallScalars)));
    HIPCHK_B(dev_alloc(&ctx->d_small_tiles, sizeof(SmallTiles)));
    HIPCHK_B(dev_alloc(&ctx->d_err, 64));
    HIPCHK_B(hipMemset(ctx->d_err, 0, 64));
    HIPCHK_B(dev_alloc(&ctx->bin_count, kNumBins * sizeof(int)));
    for (auto &sl : ctx->slots) {
        for (auto &e : sl.ev) HIPCHK_B(hipEventCreate(&e));
        for (auto &ph : sl.ev_cls) for (auto &c : ph) for (auto &e : c) HIPCHK_B(hipEventCreate(&e));
    }
    HIPCHK_B(hipStreamCreateWithFlags(&ctx->stream_b, hipStreamNonBlocking));
    HIPCHK_B(hipStreamCreateWithFlags(&ctx->stream_c, hipStreamNonBlocking));
    HIPCHK_B(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    for (auto &t : ctx->ev_tile) for (auto &e : t) HIPCHK_B(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->cache_budget = prop.totalGlobalMem / 4;
    if (const char *e = getenv("BSPGEMM_FLOW"))
        ctx->flow = !strcmp(e, "exact") ? BSPGEMM_FLOW_EXACT : (!strcmp(e, "upper-bound") || !strcmp(e, "ub")) ? BSPGEMM_FLOW_UPPER_BOUND : BSPGEMM_FLOW_AUTO;
    if (const char *e = getenv("BSPGEMM_CLASS_TIMING")) ctx->class_timing = atoi(e) != 0;
    if (const char *e = getenv("BSPGEMM_CLASS_STREAMS")) { const int n = atoi(e); ctx->class_streams = n < 1 ? 1 : (n > 3 ? 3 : n); }
    ctx->check = getenv("BSPGEMM_CHECK") != nullptr;
    if (const char *e = getenv("BSPGEMM_RW_BLK")) ctx->rw_blk = atoi(e) ? 1 : 0;
    if (const char *e = getenv("BSPGEMM_SMALL")) ctx->small = atoi(e) ? 1 : 0;
    if (const char *e = getenv("BSPGEMM_PAD_ROWS")) { const int v = atoi(e); ctx->pad_rows = v < 0 ? -1 : (v ? 1 : 0); }
    if (const char *e = getenv("BSPGEMM_SHARED_SLOTS")) { const int v = atoi(e); ctx->shared_slots = v < 0 ? -1 : (v > kSharedSlotsMax ? kSharedSlotsMax : v); }
    ctx->debug_alloc = getenv("BSPGEMM_DEBUG_ALLOC") != nullptr;
    ctx->dropin_timing = getenv("BSPGEMM_DROPIN_TIMING") != nullptr;
    ctx->kcore_timing = getenv("BSPGEMM_KCORE_TIMING") != nullptr;
    ctx->scc_timing = getenv("BSPGEMM_SCC_TIMING") != nullptr;
    ctx->color_timing = getenv("BSPGEMM_COLOR_TIMING") != nullptr;
    ctx->bfs_tree_timing = getenv("BSPGEMM_BFS_TREE_TIMING") != nullptr;
    ctx->lp_timing = getenv("BSPGEMM_LP_TIMING") != nullptr;
    ctx->pr_timing = getenv("BSPGEMM_PR_TIMING") != nullptr;
    ctx->bc_timing = getenv("BSPGEMM_BC_TIMING") != nullptr;
    ctx->match_timing = getenv("BSPGEMM_MATCH_TIMING") != nullptr;
    ctx->sssp_timing = getenv("BSPGEMM_SSSP_TIMING") != nullptr;
    ctx->extract_timing = getenv("BSPGEMM_EXTRACT_TIMING") != nullptr;
    if (const char *e = getenv("BSPGEMM_LCC_TIMING")) ctx->lcc_timing = atoi(e) == 2 ? 2 : 1;
    if (ctx->debug_alloc)
        fprintf(stderr, "[bspgemm] device %d: %s, %zu MiB, %d CUs; result cache budget %zu MiB\n", device,
                prop.gcnArchName, (size_t)(prop.totalGlobalMem >> 20), prop.multiProcessorCount, ctx->cache_budget >> 20);
    *out = ctx;
    return BSPGEMM_OK;
}

extern "C" void bspgemm_destroy(bspgemm_context *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    dev_free(ctx->F); dev_free(ctx->Fprefix); dev_free(ctx->partials);
    dev_free(ctx->cnt); dev_free(ctx->bin_tiles); dev_free(ctx->bin_count); dev_free(ctx->tmp); dev_free(ctx->tmpv);
    dev_free(ctx->rec); dev_free(ctx->recpre); dev_free(ctx->ab); dev_free(ctx->tile_row); dev_free(ctx->Fmask); dev_free(ctx->hpartials);
    dev_free(ctx->hub_rec); dev_free(ctx->hub_pre);
    if (ctx->h) hipHostFree(ctx->h);
    dev_free(ctx->d_prep);
    dev_free(ctx->d_err);
    dev_free(ctx->d_small);
    dev_free(ctx->d_small_tiles);
    dev_free(ctx->chunk_row);
    for (auto &sl : ctx->slots) {
        for (auto &e : sl.ev) if (e) hipEventDestroy(e);
        for (auto &ph : sl.ev_cls) for (auto &c : ph) for (auto &e : c) if (e) hipEventDestroy(e);
    }
    for (auto &c : ctx->cache) if (c.p) dev_free(c.p);
    if (ctx->stream_b) { hipStreamSynchronize(ctx->stream_b); hipStreamDestroy(ctx->stream_b); }
    if (ctx->stream_c) { hipStreamSynchronize(ctx->stream_c); hipStreamDestroy(ctx->stream_c); }
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    dev_free(ctx->stitch_partials);
    for (auto &t : ctx->ev_tile) for (auto &e : t) if (e) hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" bspgemm_status bspgemm_set_stream(bspgemm_context *ctx, void *hip_stream)
{
    if (!ctx) return FAIL(BSPGEMM_ERR_INVALID, "ctx is NULL");
    if (bspgemm_status st = use_device(ctx)) return st;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (hip_stream) {
        if (ctx->own_stream) hipStreamDestroy(ctx->stream);
        ctx->stream = static_cast<hipStream_t>(hip_stream);
        ctx->own_stream = false;
    } else if (!ctx->own_stream) {
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_synchronize(bspgemm_context *ctx)
{
    if (!ctx) return FAIL(BSPGEMM_ERR_INVALID, "ctx is NULL");
    if (bspgemm_status st = use_device(ctx)) return st;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_debug_scribble(bspgemm_context *ctx, uint32_t word)
{
    if (!ctx) return FAIL(BSPGEMM_ERR_INVALID, "debug_scribble: ctx is NULL");
    if (bspgemm_status st = use_device(ctx)) return st;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream_b));
    HIPCHK(hipStreamSynchronize(ctx->stream_c));
    // every scratch array the context keeps between calls, each to the size it was allocated with (the gate knows it);
    // d_err is state (zeroed once in bspgemm_create; the kernels only ever OR a bit into it) and stays as it is
    void *const scratch[] = {ctx->F, ctx->Fmask, ctx->Fprefix, ctx->partials, ctx->hpartials, ctx->cnt, ctx->bin_tiles, ctx->rec,
                             ctx->recpre, ctx->hub_rec, ctx->hub_pre, ctx->ab, ctx->tile_row, ctx->tmp, ctx->tmpv, ctx->chunk_row,
                             ctx->d_prep, ctx->d_small, ctx->d_small_tiles, ctx->bin_count, ctx->stitch_partials};
    for (void *p : scratch) HIPCHK(fill_words(p, dev_alloc_size(p), word, ctx->stream));
    for (const auto &c : ctx->cache) HIPCHK(fill_words(c.p, dev_alloc_size(c.p), word, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return BSPGEMM_OK;
}

// ------------------------------------------------------------------ operands -------------
// The three steps of a derived operand (internal.hpp).  Nothing here touches the stream but operand_finish's one launch.
bspgemm_status operand_new(bspgemm_context *ctx, int rows, int cols, bspgemm_matrix **out)
{
    bspgemm_matrix *m = *out = new (std::nothrow) bspgemm_matrix{ctx, rows, cols, 0, nullptr, nullptr, true};
    if (!m) return FAIL(BSPGEMM_ERR_ALLOC, "matrix");
    HIPCHK(dev_alloc(&m->d_row_ptr, ((size_t)rows + 1) * sizeof(int)));
    return BSPGEMM_OK;
}

bspgemm_status operand_cols(bspgemm_matrix *m, long long cap)
{
    // +1 int of slack on col_idx so an empty matrix still has a valid pointer
    HIPCHK(dev_alloc(&m->d_col_idx, ((size_t)cap + 1) * sizeof(int)));
    return BSPGEMM_OK;
}

bspgemm_status operand_finish(bspgemm_matrix *m, long long nnz)
{
    m->nnz = nnz;
    return ensure_deg8(m);
}

bspgemm_status check_operand(const bspgemm_context *ctx, const bspgemm_matrix *A, const char *who, unsigned flags)
{
    const char *what = nullptr;
    if (A->ctx != ctx) what = ": operand belongs to another context";
    else if ((flags & NEED_SQUARE) && A->rows != A->cols) what = " needs a square matrix";
    else if ((flags & NEED_ENTRIES_CONSISTENT) && A->nnz > 0 && (A->rows <= 0 || !A->d_col_idx)) what = ": nonzeros without rows";
    if (!what) return BSPGEMM_OK;
    snprintf(g_err, sizeof g_err, "%s%s", who, what);
    return BSPGEMM_ERR_INVALID;
}

size_t flag_scratch_carve(int *tmp, size_t at, long long E, bool lbs, FlagScratch *sc)
{
    const size_t W = select_words(E);
    if (W > (size_t)INT_MAX) return 0;
    auto take = [&](size_t ints) { const size_t o = at; at += (ints + 3) & ~(size_t)3; return o; };
    const size_t o_flags = take(2 * W), o_pre = take(2 * (W + 1)), o_part = take(2 * (W / 2048 + 4)), o_cnt = take(W);
    const size_t o_lbs = take(lbs ? W * 64 : 0);
    if (sc) {
        sc->flags = reinterpret_cast<unsigned long long *>(tmp + o_flags);
        sc->pre = reinterpret_cast<long long *>(tmp + o_pre);
        sc->part = reinterpret_cast<long long *>(tmp + o_part);
        sc->cnt = tmp + o_cnt;
        sc->lbs = lbs ? tmp + o_lbs : nullptr;
        sc->words = (int)W;
    }
    return at;
}

extern "C" bspgemm_status bspgemm_matrix_upload(bspgemm_context *ctx, int rows, int cols,
                                                const int *row_ptr, const int *col_idx,
                                                bspgemm_matrix **out)
{
    if (!ctx || !out || !row_ptr || rows < 0 || cols < 0) return FAIL(BSPGEMM_ERR_INVALID, "matrix_upload");
    *out = nullptr;
    const long long base = row_ptr[0];
    const long long nnz = (long long)row_ptr[rows] - base;
    if (nnz < 0 || (nnz > 0 && !col_idx)) return FAIL(BSPGEMM_ERR_INVALID, "row_ptr not ascending / col_idx NULL");
    if (bspgemm_status st = use_device(ctx)) return st;
    bspgemm_matrix *m = nullptr;
    auto bail = [&](bspgemm_status st) { bspgemm_matrix_free(m); return st; };   // handle + device arrays
    if (bspgemm_status st = operand_new(ctx, rows, cols, &m)) return bail(st);
    if (bspgemm_status st = operand_cols(m, nnz)) return bail(st);
    HIPCHK_B(hipMemcpyAsync(m->d_row_ptr, row_ptr, ((size_t)rows + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (nnz > 0)
        HIPCHK_B(hipMemcpyAsync(m->d_col_idx, col_idx + base, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    launch_rebase_i32(m->d_row_ptr, rows + 1, (int)base, ctx->stream);
    if (bspgemm_status st = operand_finish(m, nnz)) return bail(st);
    HIPCHK_B(hipStreamSynchronize(ctx->stream));
    *out = m;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_matrix_wrap_device(bspgemm_context *ctx, int rows, int cols, int64_t nnz,
                                                     const int *d_row_ptr, const int *d_col_idx,
                                                     bspgemm_matrix **out)
{
    if (!ctx || !out || !d_row_ptr || rows < 0 || cols < 0 || nnz < 0) return FAIL(BSPGEMM_ERR_INVALID, "matrix_wrap_device");
    bspgemm_matrix *m = new (std::nothrow) bspgemm_matrix{ctx, rows, cols, (long long)nnz,
                                                          const_cast<int *>(d_row_ptr),
                                                          const_cast<int *>(d_col_idx), false};
    if (!m) return FAIL(BSPGEMM_ERR_ALLOC, "matrix");
    *out = m;
    return BSPGEMM_OK;
}

extern "C" void bspgemm_matrix_free(bspgemm_matrix *m)
{
    if (!m) return;
    hipSetDevice(m->ctx->device);
    if (m->owned) {
        dev_free(m->d_row_ptr);
        dev_free(m->d_col_idx);
    }
    drop_derived(m, true);
    delete m;
}
extern "C" bspgemm_status bspgemm_matrix_download(bspgemm_context *ctx, const bspgemm_matrix *m, int *row_ptr, int *col_idx)
{
    if (!ctx || !m || m->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "matrix_download");
    if (bspgemm_status st = use_device(ctx)) return st;
    if (row_ptr)
        HIPCHK(hipMemcpyAsync(row_ptr, m->d_row_ptr, ((size_t)m->rows + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (col_idx && m->nnz > 0)
        HIPCHK(hipMemcpyAsync(col_idx, m->d_col_idx, (size_t)m->nnz * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_matrix_invalidate(bspgemm_matrix *m)
{
    if (!m) return FAIL(BSPGEMM_ERR_INVALID, "matrix is NULL");
    if (bspgemm_status st = use_device(m->ctx)) return st;
    HIPCHK(hipStreamSynchronize(m->ctx->stream));          // a multiply may still be reading the tables
    drop_derived(m, true);
    m->blk16_state = 0;
    m->pad_state = 0;
    m->nnz_pad = 0;
    return BSPGEMM_OK;
}

extern "C" const char *bspgemm_build_info(void)
{
    return "libbspgemm: HIP kernels for gfx950 only; flows upper-bound (default), exact; small-product path; "
           "timing-only ablation switches: none (BSP_ABLATE=0); tuning constants are compile-time";
}

extern "C" int bspgemm_matrix_rows(const bspgemm_matrix *m) { return m ? m->rows : 0; }
extern "C" int bspgemm_matrix_cols(const bspgemm_matrix *m) { return m ? m->cols : 0; }
extern "C" int64_t bspgemm_matrix_nnz(const bspgemm_matrix *m) { return m ? m->nnz : 0; }

// ------------------------------------------------------------------ workspace ------------
bspgemm_status ensure_rows(bspgemm_context *ctx, size_t rows)
{
    if (rows <= ctx->rows_cap) return BSPGEMM_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->F); dev_free(ctx->Fprefix); dev_free(ctx->partials); dev_free(ctx->cnt); dev_free(ctx->bin_tiles);
    dev_free(ctx->rec); dev_free(ctx->recpre); dev_free(ctx->Fmask); dev_free(ctx->hpartials);
    ctx->F = ctx->Fprefix = ctx->partials = ctx->recpre = ctx->Fmask = ctx->hpartials = nullptr;
    ctx->cnt = ctx->bin_tiles = nullptr;
    ctx->rec = nullptr;
    ctx->rows_cap = 0;
    const size_t cap = rows + rows / 8 + 64;
    const size_t tiles = cap / 2048 + 2;
    HIPCHK(dev_alloc(&ctx->F, cap * sizeof(long long)));
    HIPCHK(dev_alloc(&ctx->Fmask, cap * sizeof(long long)));
    HIPCHK(dev_alloc(&ctx->Fprefix, (cap + 1) * sizeof(long long)));
    HIPCHK(dev_alloc(&ctx->partials, (tiles + 1) * sizeof(long long)));
    HIPCHK(dev_alloc(&ctx->hpartials, (tiles + 1) * sizeof(long long)));
    HIPCHK(dev_alloc(&ctx->cnt, cap * sizeof(int)));
    HIPCHK(dev_alloc(&ctx->bin_tiles, (tiles + 1) * kNumBins * sizeof(int)));
    HIPCHK(dev_alloc(&ctx->rec, cap * sizeof(RowRec)));
    HIPCHK(dev_alloc(&ctx->recpre, cap * sizeof(long long)));
    // (each on its own: a call that got hub_rec and failed on hub_pre must not leave hub_pre NULL for good)
    if (!ctx->hub_rec) HIPCHK(dev_alloc(&ctx->hub_rec, kHeavySortMax * sizeof(RowRec)));
    if (!ctx->hub_pre) HIPCHK(dev_alloc(&ctx->hub_pre, kHeavySortMax * sizeof(long long)));
    ctx->rows_cap = cap;
    return BSPGEMM_OK;
}

static void result_cache_drop(bspgemm_context *ctx)
{
    for (auto &c : ctx->cache) if (c.p) { dev_free(c.p); c.p = nullptr; }
}

// The one grower of the flat workspaces: `*p` holds at least `need` elements of `elem` bytes afterwards, with a sixteenth
// and `slack` elements to spare.  `retry`: an out-of-memory drops the cache of freed results, which may hold what is
// missing, and asks once more.  A failure leaves *p NULL and *cap 0.
static bspgemm_status grow(bspgemm_context *ctx, void **p, size_t *cap, size_t need, size_t elem, size_t slack, bool retry)
{
    if (need <= *cap) return BSPGEMM_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(*p);
    *p = nullptr;
    *cap = 0;
    const size_t n = need + need / 16 + slack;
    hipError_t e = dev_alloc_bytes(p, n * elem);
    if (e == hipErrorOutOfMemory && retry) {
        result_cache_drop(ctx);
        (void)hipGetLastError();
        e = dev_alloc_bytes(p, n * elem);
    }
    HIPCHK(e);
    *cap = n;
    return BSPGEMM_OK;
}
template <class T>
static bspgemm_status grow(bspgemm_context *ctx, T **p, size_t *cap, size_t need, size_t slack, bool retry)
{
    return grow(ctx, reinterpret_cast<void **>(p), cap, need, sizeof(T), slack, retry);
}

bspgemm_status ensure_ab(bspgemm_context *ctx, size_t pairs) { return grow(ctx, &ctx->ab, &ctx->ab_cap, pairs, 64, false); }

// the flat prepass's first row per tile: `items` = nonzeros + rows of the row range (csrc/prepass.hip k_tile_rows)
bspgemm_status ensure_tile_rows(bspgemm_context *ctx, size_t items)
{
    return grow(ctx, &ctx->tile_row, &ctx->tile_row_cap, items / kRowWorkTile + 2, 64, false);
}

bspgemm_status ensure_tmp(bspgemm_context *ctx, size_t ints) { return grow(ctx, &ctx->tmp, &ctx->tmp_cap, ints, 1024, true); }

// the counting product's values workspace: grows like tmp
bspgemm_status ensure_tmpv(bspgemm_context *ctx, size_t ints) { return grow(ctx, &ctx->tmpv, &ctx->tmpv_cap, ints, 1024, true); }

bspgemm_status ensure_chunk_rows(bspgemm_context *ctx, size_t entries)
{
    return grow(ctx, &ctx->chunk_row, &ctx->chunk_cap, entries, 64, false);
}

// result buffers: best fit from the context's cache of freed results, else hipMalloc
static int result_cache_find(const bspgemm_context *ctx, size_t bytes)
{
    int best = -1;
    for (int i = 0; i < 8; i++) {
        const auto &c = ctx->cache[i];
        if (c.p && c.bytes >= bytes && c.bytes <= 2 * bytes + (1 << 20) &&
            (best < 0 || c.bytes < ctx->cache[best].bytes))
            best = i;
    }
    return best;
}
bool result_cached(const bspgemm_context *ctx, size_t bytes) { return result_cache_find(ctx, bytes) >= 0; }

hipError_t result_alloc(bspgemm_context *ctx, void **out, size_t bytes)
{
    const int best = result_cache_find(ctx, bytes);
    if (best >= 0) {
        *out = ctx->cache[best].p;
        ctx->cache[best].p = nullptr;
        return hipSuccess;
    }
    const bool dbg = ctx->debug_alloc;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = dev_alloc(out, bytes);
    if (dbg) {
        fprintf(stderr, "[bspgemm] hipMalloc(%zu) %.3f ms; cache:", bytes,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        for (const auto &c : ctx->cache) if (c.p) fprintf(stderr, " %zu", c.bytes);
        fprintf(stderr, "\n");
    }
    if (e == hipErrorOutOfMemory) {                     // drop the cache and retry once
        result_cache_drop(ctx);
        (void)hipGetLastError();
        e = dev_alloc(out, bytes);
    }
    return e;
}

bspgemm_status counted_result_new(bspgemm_context *ctx, int rows, long long entries, bspgemm_result **out)
{
    bspgemm_result *R = *out = new (std::nothrow) bspgemm_result{ctx, rows, entries, nullptr, nullptr, entries};
    if (!R) return FAIL(BSPGEMM_ERR_ALLOC, "result");
    HIPCHK(result_alloc(ctx, reinterpret_cast<void **>(&R->d_row_ptr), result_bytes_rowptr(rows)));
    HIPCHK(result_alloc(ctx, reinterpret_cast<void **>(&R->d_col_idx), result_bytes_colidx(entries)));
    HIPCHK(result_alloc(ctx, reinterpret_cast<void **>(&R->d_values), result_bytes_colidx(entries)));
    return BSPGEMM_OK;
}

void result_release(bspgemm_context *ctx, void *p, size_t bytes)
{
    if (!p) return;
    // the cache is capped by BYTES as well as by slots: freed results of a large product must not
    // pin the memory the next one needs (the smallest buffers go first)
    const bool dbg = ctx->debug_alloc;
    size_t held = 0;
    for (const auto &c : ctx->cache) if (c.p) held += c.bytes;
    if (dbg && held + bytes > ctx->cache_budget)
        fprintf(stderr, "[bspgemm] result cache over budget: holds %zu, released %zu, budget %zu\n", held, bytes, ctx->cache_budget);
    while (held + bytes > ctx->cache_budget && held > 0) {
        int small = -1;
        for (int i = 0; i < 8; i++)
            if (ctx->cache[i].p && (small < 0 || ctx->cache[i].bytes < ctx->cache[small].bytes)) small = i;
        if (small < 0) break;
        held -= ctx->cache[small].bytes;
        dev_free(ctx->cache[small].p);
        ctx->cache[small].p = nullptr;
    }
    if (bytes > ctx->cache_budget) { dev_free(p); return; }
    int slot = -1;
    for (int i = 0; i < 8; i++)
        if (!ctx->cache[i].p) { slot = i; break; }
    if (slot < 0) {                                     // evict the smallest cached buffer
        slot = 0;
        for (int i = 1; i < 8; i++)
            if (ctx->cache[i].bytes < ctx->cache[slot].bytes) slot = i;
        if (ctx->cache[slot].bytes >= bytes) { dev_free(p); return; }
        dev_free(ctx->cache[slot].p);
    }
    ctx->cache[slot].p = p;
    ctx->cache[slot].bytes = bytes;
}

static void fill_stats(const bspgemm_context::StatSlot &sl, bspgemm_stats &st)
{
    memset(&st, 0, sizeof st);
    const int R = sl.R;
    st.rows = R;
    st.nnz_a = R > 0 ? (long long)sl.h.a_hi - sl.h.a_lo : 0;
    st.products = sl.products;
    st.nnz_c = sl.nnz_c;
    st.bytes_alg = 4ll * (R + 1) + 12ll * st.nnz_a + 4ll * st.products + 4ll * sl.nnz_c + 8ll * (R + 1);
    st.bytes_read_alg = st.bytes_alg - 4ll * sl.nnz_c - 8ll * (R + 1);
    static_assert(kMaxBins == BSPGEMM_MAX_BINS && kNumBins <= kMaxBins, "stats arrays hold every class");
    st.bins = kNumBins;
    for (int b = 0; b < kNumBins; b++) {
        st.rows_per_bin[b] = sl.h.bin_count[b];
        st.bin_cap[b] = b == 0 ? 0 : (b == kDenseBin ? 0x7fffffff : (b == kMidBin ? sl.mid_cap : (b == kRankBin ? (sl.rank_cap > kMaxWaveCap ? sl.rank_cap : kMaxWaveCap) : 64 * kWaveChunks[b])));
    }
    st.flow = sl.flow;
    st.prepass_kernel = sl.prepass_kernel;
    st.class_streams = sl.class_streams;
    st.small_path = sl.small ? 1 : 0;
    st.checked = sl.checked ? 1 : 0;
    st.padded_rows = sl.padded ? 1 : 0;
    hipEventElapsedTime(&st.ms_total, sl.ev[0], sl.ev[4]);
    hipEventElapsedTime(&st.ms_prepass, sl.ev[0], sl.ev[1]);
    hipEventElapsedTime(&st.ms_count, sl.ev[1], sl.ev[2]);
    hipEventElapsedTime(&st.ms_symbolic, sl.ev[0], sl.ev[2]);
    hipEventElapsedTime(&st.ms_numeric, sl.ev[2], sl.ev[3]);
    hipEventElapsedTime(&st.ms_stitch, sl.ev[3], sl.ev[4]);
    for (int ph = 0; ph < 2; ph++)
        for (int b = 1; b < kNumBins; b++)
            if (sl.cls_n[ph][b] > 0 && sl.cls_timed) {
                float ms = 0, t0 = 0;
                hipEventElapsedTime(&ms, sl.ev_cls[ph][b][0], sl.ev_cls[ph][b][1]);
                hipEventElapsedTime(&t0, sl.ev[0], sl.ev_cls[ph][b][0]);
                (ph == 0 ? st.ms_bin_count : st.ms_bin)[b] = ms;
                (ph == 0 ? st.t_bin_count : st.t_bin)[b] = t0;
            }
}

extern "C" bspgemm_status bspgemm_set_class_timing(bspgemm_context *ctx, int on)
{
    if (!ctx) return FAIL(BSPGEMM_ERR_INVALID, "set_class_timing");
    ctx->class_timing = on != 0;
    return BSPGEMM_OK;
}

// Every bspgemm_option once: where it lives, what bspgemm_set_option accepts and what it says when it refuses.
namespace {
enum OptKind { OPT_RANGE, OPT_LANES, OPT_FLAG, OPT_CLAMP };   // lo..hi; 0, 4, 16 or 64; any value, kept as 0/1; at least lo, clamped at hi
struct OptRow {
    bspgemm_option opt;
    int bspgemm_context::*field;
    OptKind kind;
    int lo, hi;
    const char *refusal;
};
const OptRow kOptions[] = {
    {BSPGEMM_OPT_CLASS_STREAMS, &bspgemm_context::class_streams, OPT_RANGE, 1, 3, "class streams: 1..3"},
    {BSPGEMM_OPT_BLOCKED_EXTENTS, &bspgemm_context::rw_blk, OPT_RANGE, -1, 1, "blocked extents: -1, 0 or 1"},
    {BSPGEMM_OPT_CHECK, &bspgemm_context::check, OPT_FLAG, 0, 1, ""},
    {BSPGEMM_OPT_SMALL_PATH, &bspgemm_context::small, OPT_RANGE, -1, 1, "small path: -1, 0 or 1"},
    {BSPGEMM_OPT_PADDED_ROWS, &bspgemm_context::pad_rows, OPT_RANGE, -1, 1, "padded rows: -1, 0 or 1"},
    {BSPGEMM_OPT_SHARED_SLOTS, &bspgemm_context::shared_slots, OPT_CLAMP, -1, kSharedSlotsMax, "shared slots: -1, 0 or a count"},
    {BSPGEMM_OPT_DOT_LIGHT, &bspgemm_context::dot_light, OPT_RANGE, 0, INT_MAX, "dot light: 0 or a row length"},
    {BSPGEMM_OPT_BFS_ALPHA, &bspgemm_context::bfs_alpha, OPT_RANGE, 1, INT_MAX, "bfs alpha: 1 or more"},
    {BSPGEMM_OPT_BFS_BETA, &bspgemm_context::bfs_beta, OPT_RANGE, 1, INT_MAX, "bfs beta: 1 or more"},
    {BSPGEMM_OPT_BFS_PUSH_LANES, &bspgemm_context::bfs_push_lanes, OPT_LANES, 0, 64, "bfs push lanes: 0, 4, 16 or 64"},
    {BSPGEMM_OPT_LP_MIN_CLASS, &bspgemm_context::lp_min_class, OPT_RANGE, 0, 3, "lp min class: 0..3"},
    {BSPGEMM_OPT_PR_MIN_CLASS, &bspgemm_context::pr_min_class, OPT_RANGE, 0, 3, "pr min class: 0..3"},
    {BSPGEMM_OPT_BC_LANES, &bspgemm_context::bc_lanes, OPT_LANES, 0, 64, "bc lanes: 0, 4, 16 or 64"},
    {BSPGEMM_OPT_EXTRACT_LANES, &bspgemm_context::extract_lanes, OPT_LANES, 0, 64, "extract lanes: 0, 4, 16 or 64"},
    {BSPGEMM_OPT_MATCH_LANES, &bspgemm_context::match_lanes, OPT_LANES, 0, 64, "match lanes: 0, 4, 16 or 64"},
};
const OptRow *find_option(bspgemm_option opt)
{
    for (const OptRow &r : kOptions) if (r.opt == opt) return &r;
    return nullptr;
}
}  // namespace

extern "C" bspgemm_status bspgemm_set_option(bspgemm_context *ctx, bspgemm_option opt, int value)
{
    if (!ctx) return FAIL(BSPGEMM_ERR_INVALID, "set_option: ctx is NULL");
    const OptRow *r = find_option(opt);
    if (!r) return FAIL(BSPGEMM_ERR_INVALID, "unknown option");
    bool ok = true;
    switch (r->kind) {
    case OPT_RANGE: ok = value >= r->lo && value <= r->hi; break;
    case OPT_LANES: ok = value == 0 || value == 4 || value == 16 || value == 64; break;
    case OPT_FLAG: value = value != 0; break;
    case OPT_CLAMP: ok = value >= r->lo; if (value > r->hi) value = r->hi; break;
    }
    if (!ok) return FAIL(BSPGEMM_ERR_INVALID, r->refusal);
    ctx->*(r->field) = value;
    return BSPGEMM_OK;
}

extern "C" int bspgemm_get_option(const bspgemm_context *ctx, bspgemm_option opt)
{
    if (!ctx) return INT_MIN;
    const OptRow *r = find_option(opt);
    return r ? ctx->*(r->field) : INT_MIN;
}

extern "C" int bspgemm_matrix_uses_padded_rows(const bspgemm_matrix *m)
{
    if (!m || m->pad_state == 0) return -1;
    return m->pad_state == 1 ? 1 : 0;
}

extern "C" int bspgemm_matrix_uses_blocked_table(const bspgemm_matrix *m)
{
    if (!m || m->blk16_state == 0) return -1;
    return m->blk16_state == 1 ? 1 : 0;
}

extern "C" bspgemm_status bspgemm_set_flow(bspgemm_context *ctx, int flow)
{
    if (!ctx || flow < BSPGEMM_FLOW_AUTO || flow > BSPGEMM_FLOW_EXACT) return FAIL(BSPGEMM_ERR_INVALID, "set_flow");
    ctx->flow = flow;
    return BSPGEMM_OK;
}

extern "C" int bspgemm_result_rows(const bspgemm_result *C) { return C ? C->rows : 0; }
extern "C" int64_t bspgemm_result_nnz(const bspgemm_result *C) { return C ? C->nnz : 0; }
extern "C" const int64_t *bspgemm_result_row_ptr_device(const bspgemm_result *C)
{
    return C ? reinterpret_cast<const int64_t *>(C->d_row_ptr) : nullptr;
}
extern "C" const int *bspgemm_result_col_idx_device(const bspgemm_result *C) { return C ? C->d_col_idx : nullptr; }
extern "C" const int *bspgemm_result_values_device(const bspgemm_result *C) { return C ? C->d_values : nullptr; }

extern "C" bspgemm_status bspgemm_result_download(bspgemm_context *ctx, const bspgemm_result *C,
                                                  int64_t *row_ptr, int *col_idx)
{
    if (!ctx || !C) return FAIL(BSPGEMM_ERR_INVALID, "result_download");
    if (bspgemm_status st = use_device(ctx)) return st;
    if (row_ptr)
        HIPCHK(hipMemcpyAsync(row_ptr, C->d_row_ptr, ((size_t)C->rows + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    // (a pinned-staging pipeline with OpenMP copies out of it was measured 3x SLOWER than this
    // plain pageable copy for a 5.3 GB result: user-space first-touch faults of the fresh
    // destination cost more than the runtime's in-kernel pinning of the same pages)
    if (col_idx && C->nnz > 0)
        HIPCHK(hipMemcpyAsync(col_idx, C->d_col_idx, (size_t)C->nnz * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_result_download_values(bspgemm_context *ctx, const bspgemm_result *C, int *values)
{
    if (!ctx || !C || !values || C->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "result_download_values");
    if (!C->d_values) return FAIL(BSPGEMM_ERR_INVALID, "result_download_values: the result holds a pattern only");
    if (bspgemm_status st = use_device(ctx)) return st;
    if (C->nnz > 0)
        HIPCHK(hipMemcpyAsync(values, C->d_values, (size_t)C->nnz * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return BSPGEMM_OK;
}

extern "C" void bspgemm_result_free(bspgemm_result *C)
{
    if (!C) return;
    hipSetDevice(C->ctx->device);
    result_release(C->ctx, C->d_row_ptr, result_bytes_rowptr(C->rows));
    result_release(C->ctx, C->d_col_idx, result_bytes_colidx(C->col_cap));
    result_release(C->ctx, C->d_values, result_bytes_colidx(C->col_cap));   // (NULL: pattern only)
    delete C;
}

extern "C" bspgemm_status bspgemm_stats_at(const bspgemm_context *ctx, int age, bspgemm_stats *out)
{
    if (!ctx || !out || age < 0 || age >= bspgemm_context::kStatSlots) return FAIL(BSPGEMM_ERR_INVALID, "stats_at");
    const int k = (ctx->slot_head - age % bspgemm_context::kStatSlots + bspgemm_context::kStatSlots) % bspgemm_context::kStatSlots;
    if (!ctx->slots[k].used) return FAIL(BSPGEMM_ERR_INVALID, "no multiply of that age has completed on this context");
    fill_stats(ctx->slots[k], *out);
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_last_stats(const bspgemm_context *ctx, bspgemm_stats *out)
{
    return bspgemm_stats_at(ctx, 0, out);
}

