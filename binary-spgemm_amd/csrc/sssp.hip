// sssp.hip -- edge weights as a handle (bspgemm_weights_*) and single-source shortest paths over them, everything
// device-resident: bspgemm_sssp (include/bspgemm.h).  No product.  w[k] is the uint32 length of STORED entry k of A, that is
// of col_idx[k]; nothing is sorted or deduplicated, so the alignment is never disturbed: a repeated entry relaxes more than
// once and the smallest length wins, a self-loop never shortens anything.  dist(v) is a MINIMUM over walks, in uint64, so it
// is a unique function of (A, w, source) whatever the bucket width, the lanes, the hub split and the scheduling do.
//
// The search is delta-stepping in its near-far form with SYNCHRONOUS rounds.  T is the exclusive upper end of the open
// bucket.  A vertex is dirty from the moment it is lowered until its row is walked; the frontier ("near list") of a round
// is the dirty vertices below T.  The arrays, all in the context's workspace behind one WsCursor:
//     cnt          the counter block (SsspCnt)
//     dist[n]      u64, the tentative distances: lowered by atomicMin only
//     snap[n]      u64, dist as it was when the vertex was last settled: what a walk of its row adds the lengths to
//     pend[n]      1: dirty and at or above T (waits for a later bucket)
//     stamp[n]     the last round in which the vertex was listed as a candidate
//     near[2][n]   two near lists that the rounds ping-pong
//     cand[n]      the vertices lowered in the round
//     parent[n]    only with parent_host
//     chunk[cap]   the hub chunk records {vertex, chunk number} of the near list that is read next
//     k_sssp_init      per vertex: dist = snap = ~0, pend = stamp = 0; the source: 0, near list 0, its chunk records
//     k_sssp_relax<W>  W lanes per vertex u of the near list, striding over u's stored row, kSsspDeep steps in flight.  For
//                      entry k -> v: nd = snap[u] + w[k] and a device-scope 64-bit atomicMin(&dist[v], nd), behind a plain
//                      load of dist[v] that filters.  The lane whose atomic returned old > nd has lowered v and lists it as
//                      a candidate if atomicExch(&stamp[v], round) != round, so a vertex is listed once per round.  Reading
//                      snap[u], never dist[u], makes the round a pure function of the state before it: u may itself be
//                      lowered while it is walked, and neither the distances after the round nor the counters depend on
//                      who saw that.  The finishing lane clears pend[u].  A row longer than kSsspChunk is not walked here
//     k_sssp_hub       one workgroup per chunk record, the same walk over the chunk's entries
//     k_sssp_settle    a bounded grid strides to the candidate count, which it reads from the counter block (the relax and
//                      hub launches wrote it).  One thread per candidate v: snap[v] = dist[v], final for the round; below T
//                      v goes to the OTHER near list, with its row length added to `walked` and, for a hub, its chunk
//                      records taken by hub_chunks_emit; otherwise pend[v] = 1.  One atomic per counter and workgroup.
//                      Then the round's one read-back: the counter block
//     k_sssp_min, k_sssp_scan   when the near list comes back empty: the exact minimum m of snap over the pending vertices
//                      (one atomicMin per workgroup), then the scan launch computes T = (m / delta + 1) * delta from it as
//                      the host does after the read-back, and moves the pending vertices below T to the near list.  No
//                      pending vertex: the search is over.  Every opened bucket is non-empty
//     k_sssp_parent    entry-parallel in select's geometry (sel_rows.hpp), after the distances are final: a tight entry
//                      (u, v), dist[u] + w[k] == dist[v], sends atomicMin(&parent[v], u)
//     k_sssp_finish    per vertex: reached, the largest finite distance, parent = -1 where nobody is tight, the source's own
// Invariants.  dist only falls.  After a settle launch snap[v] == dist[v] for every vertex lowered so far.  In-bucket round
// k finalises the vertices at in-bucket depth k of the shortest-path forest, so a bucket takes at most (vertices finalised
// in it) + 1 rounds and the search at most 2 n + 2: the host caps the loop there and never spins.  The ORDER inside a list
// or among the chunk records depends on scheduling and changes nothing: a launch consumes all of them, and a minimum does
// not depend on the order of its operands.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores.  Every decision
// rests on values stored by an EARLIER launch (snap[], pend[], the lists, the chunk records and their sizes, the candidate
// count, the pending minimum) or on the return value of a device-scope atomic (atomicMin on dist[], atomicExch on stamp[],
// the appends' cursors).  The one exception is the filter in front of the atomicMin: a plain 8-byte load of dist[v], which
// may be stale.  dist[v] only falls, so a stale value is only ever LARGER than the true one: the filter passes a superset of
// the entries that can lower v and the atomic decides.  The load is one aligned 8-byte request and cannot tear.  No kernel
// waits for another workgroup: every loop is bounded by the thread's own row or chunk, or by a count that an earlier launch
// stored.
//
// Cost.  Three launches at most and one synchronisation per round, two more launches per opened bucket.  A row is walked
// AGAIN whenever its vertex is lowered after it was walked (info.entries_walked is that sum): a small delta walks fewer
// entries in more rounds, delta = UINT64_MAX is Bellman-Ford in one bucket.
#include "internal.hpp"
#include "sel_rows.hpp"
#include "hub_chunks.hpp"

struct bspgemm_weights {
    bspgemm_context *ctx;
    const bspgemm_matrix *A;            // the operand's identity: the handle and its col_idx when the weights were bound
    const int *A_col;
    long long nnz;
    bsp::u32 *d_w;                      // NULL when nnz == 0
    bsp::u64 sum;
};

namespace bsp {

constexpr int kSsspThreads = 256;
constexpr int kSsspWaves = kSsspThreads / 64;
constexpr int kSsspListThreads = 1024;  // the settle and the scan launch: one atomic per counter and WORKGROUP, as match.hip
constexpr int kSsspSettleBlocks = 256;  // the settle's grid at most: it strides to the candidate count
constexpr int kSsspChunk = 4096;        // the longest row left to one group of lanes; entries per chunk of a longer one
constexpr int kSsspDeep = 4;            // steps of a row in flight per trip of the walk, as kMatchDeep
constexpr u64 kSsspInf = ~0ull;

struct SsspCnt {
    int2 next[2];           // {entries, chunk records} appended for near list 0 / 1 by the launch that writes it
    int cand[2];            // the candidates of the odd / even rounds
    unsigned canon;         // the canonical check's word (kSetErrRange: a column outside [0, n))
    int reached;
    u64 walked;             // the row lengths of every vertex ever put on a near list
    u64 improved;           // the candidates of every round
    u64 minp;               // the smallest snap of a pending vertex; ~0: none
    u64 dist_max;
};

// ------------------------------------------------------------------ weights ---------------
// bspgemm_weights_hashed as an op of sel_walk_entries: w[p] of entry p = (r, c), and the lane's share of the sum
struct WeightHash {
    u32 *__restrict__ w;
    u32 seed, wmin;
    u64 span;                           // wmax - wmin + 1
    bool symmetric;
    u64 sum;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int) {}
    __device__ __forceinline__ void entry(int r, long long p, int c, int)
    {
        const u32 a = symmetric ? (u32)min(r, c) : (u32)r, b = symmetric ? (u32)max(r, c) : (u32)c;
        const u32 x = wmin + (u32)((u64)mix32(mix32(a ^ seed) ^ b) % span);
        w[p] = x;
        sum += x;
    }
};

__global__ __launch_bounds__(kSelThreads) void k_weights_hash(const int *__restrict__ rp, const int *__restrict__ col, int rows,
                                                             long long E, bool vec, const int *__restrict__ tile_row,
                                                             u32 *__restrict__ w, u32 seed, u32 wmin, u64 span, bool symmetric,
                                                             u64 *total)
{
    WeightHash op = {w, seed, wmin, span, symmetric, 0};
    sel_walk_entries<true>(rp, col, rows, E, vec, tile_row, op);
    const u64 s = wave_sum(op.sum);
    if (lane_id() == 0 && s) atomicAdd(total, s);
}

// ------------------------------------------------------------------ the search ------------
__global__ __launch_bounds__(kSsspThreads) void k_sssp_init(int n, int source, const int *__restrict__ rp, u64 *__restrict__ dist,
                                                           u64 *__restrict__ snap, int *__restrict__ pend,
                                                           unsigned *__restrict__ stamp, int *__restrict__ parent,
                                                           int *__restrict__ near0, SsspCnt *cnt, int2 *__restrict__ chunk,
                                                           int chunk_cap)
{
    const long long v = (long long)blockIdx.x * kSsspThreads + threadIdx.x;
    if (v >= n) return;
    const u64 d = v == source ? 0 : kSsspInf;
    dist[v] = d;
    snap[v] = d;
    pend[v] = 0;
    stamp[v] = 0u;
    if (parent) parent[v] = INT_MAX;
    if (v == source) {                                       // (the block was zeroed by the host)
        const int len = rp[v + 1] - rp[v];
        near0[0] = source;
        cnt->next[0].x = 1;
        cnt->walked = (u64)len;
        cnt->minp = kSsspInf;
        const int k = hub_chunks_over<kSsspChunk>(len);
        if (k) hub_chunks_emit(source, k, &cnt->next[0].y, chunk, chunk_cap);
    }
}

// The walk of the entries pos, pos + stride, ... below e of a row whose vertex has the settled distance su.  Called by every
// lane of the wave, with pos >= e where a lane has nothing: the trips are wave-uniform, so wave_append has its full wave.
// kSsspDeep steps per trip, stage by stage (columns and lengths, then dist[], then the atomics), so that a long row pays
// the dependent memory latencies once per kSsspDeep * stride entries.  A column outside [0, n) is skipped BEFORE it indexes
// anything: the canonical check that runs in front of the search reports it, and the host reads its word with the first
// read-back.
__device__ __forceinline__ void sssp_walk(long long pos, long long e, int stride, u64 su, const int *__restrict__ col,
                                          const u32 *__restrict__ wt, int n, u64 *dist, unsigned *stamp, unsigned round, int *cand,
                                          int *cand_size)
{
    const int lane = lane_id();
    for (; __ballot(pos < e); pos += (long long)stride * kSsspDeep) {
        int x[kSsspDeep];
        u64 nd[kSsspDeep], dv[kSsspDeep];
        bool in[kSsspDeep];
#pragma unroll
        for (int j = 0; j < kSsspDeep; j++) {
            const long long p = pos + (long long)stride * j;
            in[j] = p < e;
            x[j] = in[j] ? col[p] : 0;
            nd[j] = su + (in[j] ? wt[p] : 0u);
            in[j] = in[j] && (unsigned)x[j] < (unsigned)n;
        }
#pragma unroll
        for (int j = 0; j < kSsspDeep; j++) dv[j] = in[j] ? dist[x[j]] : 0;   // (the filter: stale means larger)
#pragma unroll
        for (int j = 0; j < kSsspDeep; j++) {
            bool first = false;
            if (in[j] && dv[j] > nd[j] && atomicMin(&dist[x[j]], nd[j]) > nd[j])
                first = atomicExch(&stamp[x[j]], round) != round;
            wave_append(first, x[j], cand, cand_size, n, lane);          // (once per vertex and round: at most n entries)
        }
    }
}

// W lanes per vertex of `list` (fsize entries, from the host).  snap[] was stored by earlier launches.  nx: the near list
// that this round's settle appends to; the host has read its size pair already.  The pending minimum is reset here as well:
// the launches that use it come after a settle.
template <int W>
__global__ __launch_bounds__(kSsspThreads) void k_sssp_relax(int fsize, const int *__restrict__ list, const int *__restrict__ rp,
                                                            const int *__restrict__ col, const u32 *__restrict__ wt, int n,
                                                            const u64 *__restrict__ snap, u64 *dist, int *__restrict__ pend,
                                                            unsigned *stamp, unsigned round, int *cand, SsspCnt *cnt, int nx)
{
    GroupRow<W, kSsspThreads> g;
    if (g.t == 0) {
        cnt->next[nx] = make_int2(0, 0);
        cnt->minp = kSsspInf;
    }
    u64 su = 0;
    g.template row<kSsspChunk>(fsize, list, 0, rp, [&, sub = g.sub](int u) {
        su = snap[u];
        if (sub == 0) pend[u] = 0;
    });
    sssp_walk(g.pos, g.e, W, su, col, wt, n, dist, stamp, round, cand, &cnt->cand[round & 1]);
}

// one workgroup per chunk record chunk[blockIdx.x]
__global__ __launch_bounds__(kSsspThreads) void k_sssp_hub(const int2 *__restrict__ chunk, const int *__restrict__ rp,
                                                          const int *__restrict__ col, const u32 *__restrict__ wt, int n,
                                                          const u64 *__restrict__ snap, u64 *dist, unsigned *stamp, unsigned round,
                                                          int *cand, SsspCnt *cnt)
{
    const int2 rec = chunk[blockIdx.x];
    long long b, e;
    hub_chunk_range<kSsspChunk>(rp, rec, b, e);
    sssp_walk(b + threadIdx.x, e, kSsspThreads, snap[rec.x], col, wt, n, dist, stamp, round, cand, &cnt->cand[round & 1]);
}

// What the settle and the scan launch do for the vertices they put on a near list (`take`), in workgroups of
// kSsspListThreads: block_list_append (hub_chunks.hpp).  A vertex is listed once per launch at most.  The barrier frees `sh`
// for the settle's next trip.
typedef ListBlock<kSsspListThreads, false> SsspBlock;

__device__ __forceinline__ void sssp_list(bool take, int u, const int *__restrict__ rp, int n, int *list, SsspCnt *c, int nx,
                                          int2 *chunk, int chunk_cap, SsspBlock &sh)
{
    block_list_append<kSsspListThreads, kSsspChunk, false>(take, false, u, rp, n, list, &c->next[nx], &c->walked, nullptr, chunk,
                                                           chunk_cap, sh);
    __syncthreads();
}

// par: the round's parity, whose candidate count the relax and hub launches left; the other count is reset for the next
// round.  dist[] is final for the round: those launches were earlier ones.
__global__ __launch_bounds__(kSsspListThreads) void k_sssp_settle(int n, const int *__restrict__ rp, const u64 *__restrict__ dist,
                                                                 u64 *__restrict__ snap, int *__restrict__ pend,
                                                                 const int *__restrict__ cand, int *__restrict__ next, SsspCnt *cnt,
                                                                 int par, int nx, u64 T, int2 *__restrict__ chunk, int chunk_cap)
{
    __shared__ SsspBlock sh;
    const int total = min(cnt->cand[par], n);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt->cand[par ^ 1] = 0;
        cnt->improved += (u64)total;
    }
    for (long long base = (long long)blockIdx.x * kSsspListThreads; base < total; base += (long long)gridDim.x * kSsspListThreads) {
        const long long t = base + threadIdx.x;
        int v = 0;
        bool take = false;
        if (t < total) {
            v = cand[t];
            const u64 d = dist[v];
            snap[v] = d;
            take = d < T;
            if (!take) pend[v] = 1;
        }
        sssp_list(take, v, rp, n, next, cnt, nx, chunk, chunk_cap, sh);
    }
}

__global__ __launch_bounds__(kSsspThreads) void k_sssp_min(int n, const int *__restrict__ pend, const u64 *__restrict__ snap,
                                                          SsspCnt *cnt)
{
    __shared__ u64 part[kSsspWaves];
    const long long v = (long long)blockIdx.x * kSsspThreads + threadIdx.x;
    u64 m = v < n && pend[v] ? snap[v] : kSsspInf;
    m = block_min<kSsspThreads>(m, part);
    if (threadIdx.x == 0 && m != kSsspInf) atomicMin(&cnt->minp, m);
}

// the bucket that holds the pending minimum m: its exclusive upper end.  Host and device.  No overflow: m < 2^63 (at most
// 2^31 edges of less than 2^32 each), and a delta above m gives delta itself.
__host__ __device__ __forceinline__ u64 sssp_bucket_end(u64 m, u64 delta) { return (m / delta + 1) * delta; }

// the pending minimum was completed by the launch before
__global__ __launch_bounds__(kSsspListThreads) void k_sssp_scan(int n, const int *__restrict__ rp, int *__restrict__ pend,
                                                               const u64 *__restrict__ snap, int *__restrict__ next, SsspCnt *cnt,
                                                               int nx, u64 delta, int2 *__restrict__ chunk, int chunk_cap)
{
    __shared__ SsspBlock sh;
    const u64 m = cnt->minp;
    if (m == kSsspInf) return;                               // (every thread of the grid)
    const u64 T = sssp_bucket_end(m, delta);
    const long long v = (long long)blockIdx.x * kSsspListThreads + threadIdx.x;
    const bool take = v < n && pend[v] && snap[v] < T;
    if (take) pend[v] = 0;
    sssp_list(take, take ? (int)v : 0, rp, n, next, cnt, nx, chunk, chunk_cap, sh);
}

// the tight entries as an op of sel_walk_entries
struct TightParent {
    const u32 *__restrict__ wt;
    const u64 *__restrict__ dist;
    int *parent;
    int n;
    u64 du;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int u) { du = dist[u]; }
    __device__ __forceinline__ void entry(int u, long long p, int v, int)
    {
        if (du == kSsspInf || (unsigned)v >= (unsigned)n) return;
        if (du + wt[p] == dist[v]) atomicMin(&parent[v], u);
    }
};

__global__ __launch_bounds__(kSelThreads) void k_sssp_parent(const int *__restrict__ rp, const int *__restrict__ col, int n,
                                                            long long E, bool vec, const int *__restrict__ tile_row,
                                                            const u32 *__restrict__ wt, const u64 *__restrict__ dist, int *parent)
{
    TightParent op = {wt, dist, parent, n, kSsspInf};
    sel_walk_entries<false>(rp, col, n, E, vec, tile_row, op);
}

__global__ __launch_bounds__(kSsspThreads) void k_sssp_finish(int n, int source, const u64 *__restrict__ dist, int *__restrict__ parent,
                                                             SsspCnt *cnt)
{
    __shared__ u64 part[kSsspWaves];
    __shared__ int wsum[kSsspWaves];
    const long long v = (long long)blockIdx.x * kSsspThreads + threadIdx.x;
    const u64 d = v < n ? dist[v] : kSsspInf;
    const bool reached = d != kSsspInf;
    if (v < n && parent) {
        const int p = parent[v];
        parent[v] = v == source ? source : (!reached || p == INT_MAX ? -1 : p);
    }
    // (open code: a block_max in the manner of block_min brings a barrier of its own and more registers)
    const u64 m = wave_max(reached ? d : 0ull);
    if (lane_id() == 0) part[threadIdx.x >> 6] = m;
    block_add<kSsspThreads>(reached, &cnt->reached, nullptr, wsum);      // (its barriers cover part[] too)
    if (threadIdx.x == 0) {
        u64 mm = part[0];
#pragma unroll
        for (int q = 1; q < kSsspWaves; q++) mm = max(mm, part[q]);
        if (mm) atomicMax(&cnt->dist_max, mm);
    }
}

}  // namespace bsp

using namespace bsp;

// ------------------------------------------------------------------ weights: the host side ---
static bspgemm_status weights_new(bspgemm_context *ctx, const bspgemm_matrix *A, const char *who, bspgemm_weights **W)
{
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    bspgemm_weights *w = new (std::nothrow) bspgemm_weights{ctx, A, A->d_col_idx, A->nnz, nullptr, 0};
    if (!w) return FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_weights: out of host memory");
    if (A->nnz > 0) {
        const hipError_t e = dev_alloc(&w->d_w, (size_t)A->nnz * sizeof(u32));
        if (e != hipSuccess) {
            delete w;
            HIPCHK(e);
        }
    }
    *W = w;
    return BSPGEMM_OK;
}

extern "C" void bspgemm_weights_free(bspgemm_weights *W)
{
    if (!W) return;
    if (W->d_w) {
        hipStreamSynchronize(W->ctx->stream);
        dev_free(W->d_w);
    }
    delete W;
}

extern "C" bspgemm_status bspgemm_weights_upload(bspgemm_context *ctx, const bspgemm_matrix *A, const uint32_t *w_host,
                                                 bspgemm_weights **W)
{
    static const char who[] = "bspgemm_weights_upload";
    if (W) *W = nullptr;
    if (!ctx || !A || !W || (!w_host && A->nnz > 0)) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_weights_upload: NULL argument");
    bspgemm_weights *w = nullptr;
    if (bspgemm_status st = weights_new(ctx, A, who, &w)) return st;
    auto bail = [&](bspgemm_status st) { bspgemm_weights_free(w); return st; };
    if (w->nnz > 0) {
        HIPCHK_B(hipMemcpyAsync(w->d_w, w_host, (size_t)w->nnz * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
        for (long long k = 0; k < w->nnz; k++) w->sum += w_host[k];
        HIPCHK_B(hipStreamSynchronize(ctx->stream));        // (w_host is the caller's again)
    }
    *W = w;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_weights_hashed(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned seed, uint32_t wmin,
                                                 uint32_t wmax, unsigned flags, bspgemm_weights **W)
{
    static const char who[] = "bspgemm_weights_hashed";
    if (W) *W = nullptr;
    if (!ctx || !A || !W) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_weights_hashed: NULL argument");
    if (flags & ~(unsigned)BSPGEMM_WEIGHTS_SYMMETRIC) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_weights_hashed: unknown flags");
    if (wmin > wmax) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_weights_hashed: wmin > wmax");
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    // the sum's device word and the tile rows first: the workspace answers an out-of-memory once by itself
    if (A->nnz > 0) {
        if (bspgemm_status st = ensure_tmp(ctx, 4)) return st;
        if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)A->nnz)) return st;
    }
    bspgemm_weights *w = nullptr;
    if (bspgemm_status st = weights_new(ctx, A, who, &w)) return st;
    auto bail = [&](bspgemm_status st) { bspgemm_weights_free(w); return st; };
    if (w->nnz > 0) {
        hipStream_t s = ctx->stream;
        u64 *d_sum = reinterpret_cast<u64 *>(ctx->tmp);
        HIPCHK_B(hipMemsetAsync(d_sum, 0, sizeof(u64), s));
        launch_select_tile_rows(A->d_row_ptr, A->rows, ctx->tile_row, s);
        hipLaunchKernelGGL(k_weights_hash, dim3(select_tiles(w->nnz)), dim3(kSelThreads), 0, s, A->d_row_ptr, A->d_col_idx, A->rows,
                           w->nnz, aligned16(A->d_col_idx), ctx->tile_row, w->d_w, (u32)seed, (u32)wmin,
                           (u64)wmax - (u64)wmin + 1, (flags & BSPGEMM_WEIGHTS_SYMMETRIC) != 0, d_sum);
        HIPCHK_B(round_fetch(&w->sum, d_sum, sizeof(u64), s));
    }
    *W = w;
    return BSPGEMM_OK;
}

extern "C" bspgemm_status bspgemm_weights_download(bspgemm_context *ctx, const bspgemm_weights *W, uint32_t *w_host)
{
    if (!ctx || !W || W->ctx != ctx || (!w_host && W->nnz > 0)) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_weights_download");
    if (bspgemm_status st = use_device(ctx)) return st;
    if (W->nnz > 0) {
        HIPCHK(hipMemcpyAsync(w_host, W->d_w, (size_t)W->nnz * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return BSPGEMM_OK;
}

extern "C" int64_t bspgemm_weights_nnz(const bspgemm_weights *W) { return W ? W->nnz : 0; }
extern "C" uint64_t bspgemm_weights_sum(const bspgemm_weights *W) { return W ? W->sum : 0; }

// ------------------------------------------------------------------ the search: the host side ---
// delta = max(1, c * (sum / nnz) / max(1, nnz / n)), integer divisions in exactly this order (include/bspgemm.h)
static u64 sssp_default_delta(u64 sum, long long nnz, long long n)
{
    if (nnz <= 0) return 1;
    const u64 mean_w = sum / (u64)nnz, mean_deg = (u64)std::max(1ll, nnz / n);
    return std::max<u64>(1, (u64)BSPGEMM_SSSP_DELTA_C * mean_w / mean_deg);
}

extern "C" bspgemm_status bspgemm_sssp(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_weights *W, int source,
                                       const bspgemm_sssp_params *params, uint64_t *dist_host, int *parent_host,
                                       bspgemm_sssp_info *info)
{
    static const char who[] = "bspgemm_sssp";
    if (info) memset(info, 0, sizeof *info);
    if (!ctx || !A || !W) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_sssp: NULL argument");
    if (source < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_sssp: negative source");
    const int forced_w = params ? params->lanes : 0;
    if (forced_w != 0 && forced_w != 4 && forced_w != 16 && forced_w != 64)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_sssp: lanes must be 0, 4, 16 or 64");
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_SQUARE | NEED_ENTRIES_CONSISTENT)) return st;
    if (W->ctx != ctx) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_sssp: W belongs to another context");
    if (W->A != A || W->A_col != A->d_col_idx || W->nnz != A->nnz)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_sssp: W was not made for this operand");
    const int n = A->rows;
    if (n == 0) return BSPGEMM_OK;
    if (source >= n) {
        snprintf(g_err, sizeof g_err, "%s: source %d outside [0, %d)", who, source, n);
        return BSPGEMM_ERR_INVALID;
    }
    // BSPGEMM_SSSP_TIMING: host clocks around the stages; every launch is then synchronised
    StageClock clk(ctx->sssp_timing, ctx->stream);
    double ms_relax = 0, ms_hub = 0, ms_settle = 0, ms_adv = 0, ms_back = 0, ms_parent = 0;
    if (bspgemm_status st = use_device(ctx)) return st;
    const long long E = A->nnz;
    const u64 delta = params && params->delta ? params->delta : sssp_default_delta(W->sum, E, n);
    // the lanes per near-list vertex of the call: a QUARTER of the mean stored degree, the rule of match.hip -- no group walks
    // more than kSsspChunk entries, so a hub is no serial tail
    const int Wl = forced_w ? forced_w : lanes_for_mean(E, n, 4);
    // The workspace grows ONCE, before anything is launched.  A row longer than the chunk size has fewer than 2 len / chunk
    // chunks, so all hubs together have fewer than 2 nnz / chunk records.
    const size_t n4 = ws_pad4((size_t)n), chunk_cap = (size_t)(2 * E / kSsspChunk + 1);
    SsspCnt *d_cnt = nullptr;
    u64 *dist = nullptr, *snap = nullptr;
    int *pend = nullptr, *near[2] = {nullptr, nullptr}, *cand = nullptr, *parent = nullptr;
    unsigned *stamp = nullptr;
    int2 *chunk = nullptr;
    auto carve = [&](int *tmp) {
        return WsCursor(tmp).take(d_cnt, 1).take(dist, n4).take(snap, n4).take(pend, n4).take(stamp, n4).take(near[0], n4)
            .take(near[1], n4).take(cand, n4).take_if(parent_host != nullptr, parent, n4).take(chunk, chunk_cap).ints();
    };
    if (bspgemm_status st = ensure_tmp(ctx, carve(nullptr))) return st;
    if (E > 0)
        if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return st;
    carve(ctx->tmp);
    hipStream_t s = ctx->stream;
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); return st; };
    const dim3 block(kSsspThreads), lblock(kSsspListThreads);
    const dim3 vgrid = grid_for(n, kSsspThreads), lgrid = grid_for(n, kSsspListThreads);
    const dim3 sgrid(std::min(lgrid.x, (unsigned)kSsspSettleBlocks));
    const int *rp = A->d_row_ptr, *col = A->d_col_idx;
    const u32 *wt = W->d_w;
    SsspCnt h;
    clk.start();
    HIPCHK_B(round_reset(d_cnt, sizeof(SsspCnt), s));
    launch_canonical_check(rp, col, n, n, E, 0, ctx->tile_row, &d_cnt->canon, s);   // (read with the first read-back)
    hipLaunchKernelGGL(k_sssp_init, vgrid, block, 0, s, n, source, rp, dist, snap, pend, stamp, parent, near[0], d_cnt, chunk,
                       (int)chunk_cap);
    HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));
    HIPCHK_B(clk.lap(ms_back));
    if (h.canon & kSetErrRange) return bail(fail_bad_column(who, n));
    int2 head = h.next[0];                                  // {entries, chunk records} of the near list that is read next
    int cur = 0, buckets = 1;
    long long rounds = 0, hub_chunks = 0;
    u64 T = delta;                                          // the first bucket: [0, delta)
    const long long cap_rounds = 2ll * n + 2;
    for (;;) {
        if (!frontier_head_ok(head, 0, n, chunk_cap)) return bail(fail_stuck(who));
        if (head.x == 0) {                                  // ADVANCE: the bucket of the smallest pending vertex
            clk.start();
            hipLaunchKernelGGL(k_sssp_min, vgrid, block, 0, s, n, pend, snap, d_cnt);
            hipLaunchKernelGGL(k_sssp_scan, lgrid, lblock, 0, s, n, rp, pend, snap, near[cur], d_cnt, cur, delta, chunk,
                               (int)chunk_cap);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_adv, true));
            HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));
            HIPCHK_B(clk.lap(ms_back));
            if (h.minp == kSsspInf) break;                  // nothing is pending: done
            T = sssp_bucket_end(h.minp, delta);
            buckets++;
            head = h.next[cur];
            if (!frontier_head_ok(head, 1, n, chunk_cap)) return bail(fail_stuck(who));
        }
        if (rounds >= cap_rounds) return bail(fail_stuck(who));
        rounds++;
        hub_chunks += head.y;
        const int fsize = head.x;
        const unsigned round = (unsigned)rounds;
        double ms_round = 0;
        clk.start();
        dispatch_lanes(Wl, [&](auto w) {
            hipLaunchKernelGGL(k_sssp_relax<decltype(w)::value>, grid_for((long long)fsize * Wl, kSsspThreads), block, 0, s, fsize,
                               near[cur], rp, col, wt, n, snap, dist, pend, stamp, round, cand, d_cnt, cur ^ 1);
        });
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(clk.lap(ms_relax, true));
        ms_round += clk.last;
        if (head.y > 0) {
            hipLaunchKernelGGL(k_sssp_hub, dim3((unsigned)head.y), block, 0, s, chunk, rp, col, wt, n, snap, dist, stamp, round, cand,
                               d_cnt);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_hub, true));
            ms_round += clk.last;
        }
        hipLaunchKernelGGL(k_sssp_settle, sgrid, lblock, 0, s, n, rp, dist, snap, pend, cand, near[cur ^ 1], d_cnt, (int)(round & 1),
                           cur ^ 1, T, chunk, (int)chunk_cap);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(clk.lap(ms_settle, true));
        clk.longest(ms_round + clk.last, (int)rounds, fsize);
        HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));      // the round's one synchronisation
        HIPCHK_B(clk.lap(ms_back));
        cur ^= 1;
        head = h.next[cur];
    }
    clk.start();
    if (parent && E > 0) {
        launch_select_tile_rows(rp, n, ctx->tile_row, s);
        hipLaunchKernelGGL(k_sssp_parent, dim3(select_tiles(E)), dim3(kSelThreads), 0, s, rp, col, n, E, aligned16(col),
                           ctx->tile_row, wt, dist, parent);
    }
    hipLaunchKernelGGL(k_sssp_finish, vgrid, block, 0, s, n, source, dist, parent, d_cnt);
    HIPCHK_B(hipGetLastError());
    HIPCHK_B(clk.lap(ms_parent, true));
    HIPCHK_B(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
    // the caller's arrays last: a call that fails leaves them as they were
    if (dist_host) HIPCHK_B(hipMemcpyAsync(dist_host, dist, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, s));
    if (parent_host) HIPCHK_B(hipMemcpyAsync(parent_host, parent, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));
    HIPCHK_B(clk.lap(ms_back));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: n %d nnz %lld source %d delta %llu reached %d entries walked %llu improved %llu hub chunks %lld "
                        "(%d lanes) | total %.3f ms = %lld relax launches %.3f + hub launches %.3f + settle launches %.3f + %d "
                        "advances (min and scan) %.3f + read-backs %.3f + parent pass %.3f + rest | longest round %.3f ms (round "
                        "%d, %d near vertices)\n",
                who, n, E, source, (unsigned long long)delta, h.reached, (unsigned long long)h.walked,
                (unsigned long long)h.improved, hub_chunks, Wl, clk.total(), rounds, ms_relax, ms_hub, ms_settle, buckets, ms_adv,
                ms_back, ms_parent, clk.max_ms, clk.max_tag[0], clk.max_tag[1]);
    if (info) {
        info->delta = delta;
        info->dist_max = h.dist_max;
        info->reached = h.reached;
        info->entries_walked = (int64_t)h.walked;
        info->improved = (int64_t)h.improved;
        info->hub_chunks = hub_chunks;
        info->rounds = (int)rounds;
        info->buckets = buckets;
        info->lanes = Wl;
    }
    return BSPGEMM_OK;
}
