// betweenness.hip -- betweenness centrality (Brandes) from a list of sources, exact in 64-bit integers, everything
// device-resident: bspgemm_betweenness (include/bspgemm.h, which holds the definition).  No product, no
// transpose: both sweeps read rows of A only.  The arrays, all in the context's workspace, grown once before anything is
// launched (about 44 n bytes):
//     level[n]   -1 = unreached (int32)                     sigma[n]  shortest-path counts, exact u64
//     delta[n]   the dependencies, 2^32 = 1.0 (u64)          c[n]      c(w) = (double)(2^32 + delta(w)) / (double) sigma(w)
//     bc[n]      the sums over the sources (u64)             order[n]  the levels of the current source back to back:
//     chunk[]    {hub, chunk number} for every kBcHubChunk              Brandes' stack; the host keeps the offsets
//                entries of a reached row longer than that, in the order of the levels like order[]
// and BcCounters, all CUMULATIVE over a source so that no launch resets anything: the entries of order[], the chunk records,
// the out-degree sum of the appended vertices, the error bits; the host subtracts what it read a level before.
//     k_bc_init          per vertex, once per call: level = -1, sigma = delta = bc = 0
//     k_bc_degrees       the sources' out-degrees, read back once per call
//     k_bc_source        level(s) = 0, sigma(s) = 1, order[0] = s, the counters, s's chunk records
//     k_bc_forward<W>    level d from the slice of order[] that holds level d - 1, W lanes per vertex striding over its row of
//                        A.  Entry (u, w): level[w] == -1 (plain load) -> old = atomicCAS(&level[w], -1, d); old == -1 is the
//                        winner, which appends w behind order[] (one atomic per wave), adds w's out-degree and, for a row
//                        longer than kBcHubChunk, takes its chunk records from a cursor.  Then, where level[w] is d (the
//                        load, or the CAS's return value): old = atomicAdd(&sigma[w], sigma[u]) at device scope, and bit 63
//                        of old + sigma[u] raises the overflow bit.  Rows longer than kBcHubChunk are skipped here:
//     k_bc_forward_chunk one workgroup per chunk record of the level, the same entry step
//     k_bc_leaf          the last level: delta = 0, c = 2^32 / sigma
//     k_bc_backward<W>   level d = depth - 1 .. 0 over the same slice: each lane sums (u64) floor(c[w] * (double) sigma[v])
//                        over its entries with level[w] == d + 1, an integer shuffle reduction joins the W lanes, and the
//                        finishing lane stores delta[v] and c[v] and adds to bc[v] when v is not the source.  No atomics.
//     k_bc_backward_chunk, k_bc_hub_finish   the hubs of the level: every chunk adds its partial sum to delta[v] by ONE
//                        device-scope atomicAdd, and a later launch, one lane per record, finishes the hubs (records with
//                        chunk number 0)
//     k_bc_reset         over order[0 .. reached): the call's largest sigma, then level = -1, sigma = delta = 0, so a source
//                        costs what it reaches
//
// Why the bits are unique.  level(w) is the BFS distance: exactly the unreached w with an in-neighbour in the frontier win a
// CAS.  sigma(w) is a sum of the frontier's final sigma(u) over the entries (u, w), A being duplicate-free; integer addition
// commutes.  Every backward summand is a pure function of c(w) and sigma(v), which are final when it is computed (c(w) by
// the launch of level d + 1, sigma by the forward sweep), and the two double operations are single correctly rounded ones
// (__ddiv_rn, __dmul_rn: nothing to fuse with); the summands are integers, so lane width, chunking and order change nothing.
// The order INSIDE a level of order[] depends on scheduling, and nothing that is returned depends on it.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is not refreshed by other CUs' stores, so every decision rests
// on the return value of a device-scope atomic or on a value from before the launch.  The one plain load of a word that the
// same launch changes is level[w] in the forward kernels: the launch stores only d there, over -1.  A value in [0, d) is
// from an earlier launch and final; d is true whenever it is seen; a stale -1 leads to the CAS, whose return value decides.
// sigma[u], c[w], sigma[v] and delta[hub] are read plainly only by launches behind the ones that wrote them.  No kernel
// waits for another workgroup: every loop is bounded by a row, a chunk or a count that the host passed in.
//
// Cost.  One read-back per forward level (32 bytes) and one per call for the sources' out-degrees; the backward sweep has
// none, the host knows every offset.
#include "internal.hpp"
#include "hub_chunks.hpp"
#include "wave.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace bsp {

constexpr int kBcThreads = 256;
constexpr int kBcWaves = kBcThreads / 64;
constexpr int kBcHubChunk = 4096;       // the longest row left to one group of lanes; entries per chunk of a longer one
                                        // (tests/bc_ref.py mirrors it)
constexpr unsigned kBcErrRange = 1u;    // a column outside [0, n) met by a forward launch
constexpr unsigned kBcErrOverflow = 2u; // an add on sigma reached 2^63
constexpr u64 kBcOne = 1ull << 32;

struct BcCounters {
    u64 deg;                            // the out-degree sum of the vertices appended for this source
    u64 sigma_max;                      // over the call
    int tail;                           // entries of order[] for this source
    int ctail;                          // chunk records for this source
    unsigned err;                       // kBcErrRange | kBcErrOverflow
    unsigned canon;                     // the canonical check (kSetErrRange, kSetErrOrder)
};

// what every forward launch gets.  level and order are loaded plainly and changed in the same launch (at other places, or
// as described above): neither const nor __restrict__.
struct BcFwd {
    int n, d;
    const int *rpA;
    int *level;
    u64 *sigma;
    int *order;
    int2 *chunk;
    int chunk_cap;
    BcCounters *cnt;
};

// what every backward launch gets.  c is read (level d + 1) and written (level d) in the same launch, at different places.
struct BcBwd {
    int n, d, src;
    const int *rpA;
    const int *level;
    const u64 *sigma;
    u64 *delta;
    double *c;
    u64 *bc;
};

// one entry (u, w) of the frontier, su = sigma(u).  Whole wave; `live` lanes hold an entry.
__device__ __forceinline__ void bc_forward_entry(const BcFwd &a, bool live, int w, u64 su, long long &dsum, unsigned &err, int lane)
{
    bool take = false;
    if (live) {
        if ((unsigned)w >= (unsigned)a.n) {                  // before w indexes anything
            err |= kBcErrRange;
        } else {
            int lv = a.level[w];
            if (lv == -1) {
                const int old = atomicCAS(&a.level[w], -1, a.d);
                take = old == -1;
                lv = take ? a.d : old;
            }
            if (lv == a.d) {
                const u64 old = atomicAdd(&a.sigma[w], su);
                if ((old + su) >> 63) err |= kBcErrOverflow;
            }
            if (take) {
                const int len = a.rpA[w + 1] - a.rpA[w];
                dsum += len;
                const int k = hub_chunks_over<kBcHubChunk>(len);
                if (k) hub_chunks_emit(w, k, &a.cnt->ctail, a.chunk, a.chunk_cap);
            }
        }
    }
    // (a vertex is appended once per source, so order[] never passes n entries; the list is read plainly by this launch)
    wave_append(take, w, a.order, &a.cnt->tail, a.n, lane);
}

// the end of a forward launch: the wave's out-degree sum and error bits, one atomic each per wave.  Whole wave.
__device__ __forceinline__ void bc_forward_end(long long dsum, unsigned err, BcCounters *cnt, int lane)
{
    dsum = wave_sum(dsum);
    const unsigned bits = (__ballot(err & kBcErrRange) ? kBcErrRange : 0u) | (__ballot(err & kBcErrOverflow) ? kBcErrOverflow : 0u);
    if (lane == 0) {
        if (dsum) atomicAdd(&cnt->deg, (u64)dsum);
        if (bits) atomicOr(&cnt->err, bits);
    }
}

__global__ __launch_bounds__(kBcThreads) void k_bc_init(int n, int *__restrict__ level, u64 *__restrict__ sigma,
                                                       u64 *__restrict__ delta, u64 *__restrict__ bc)
{
    const long long v = (long long)blockIdx.x * kBcThreads + threadIdx.x;
    if (v >= n) return;
    level[v] = -1;
    sigma[v] = 0;
    delta[v] = 0;
    bc[v] = 0;
}

// the sources were tested against [0, n) on the host
__global__ __launch_bounds__(kBcThreads) void k_bc_degrees(int ns, const int *__restrict__ src, const int *__restrict__ rpA,
                                                          int *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kBcThreads + threadIdx.x;
    if (i < ns) out[i] = rpA[src[i] + 1] - rpA[src[i]];
}

// one workgroup.  len: the source's out-degree, from k_bc_degrees
__global__ __launch_bounds__(kBcThreads) void k_bc_source(int src, int len, int *__restrict__ level, u64 *__restrict__ sigma,
                                                         int *__restrict__ order, int2 *__restrict__ chunk, int chunk_cap,
                                                         BcCounters *cnt)
{
    const int k = hub_chunks_over<kBcHubChunk>(len);
    if (threadIdx.x == 0) {
        level[src] = 0;
        sigma[src] = 1;
        order[0] = src;
        cnt->deg = (u64)len;
        cnt->tail = 1;
        cnt->ctail = k;
        cnt->err = 0;
    }
    for (int j = threadIdx.x; j < k && j < chunk_cap; j += kBcThreads) chunk[j] = make_int2(src, j);
}

// W lanes per vertex of order[first .. first + fsize)
template <int W>
__global__ __launch_bounds__(kBcThreads) void k_bc_forward(BcFwd a, int fsize, int first, const int *__restrict__ colA)
{
    const int lane = lane_id();
    GroupRow<W, kBcThreads> g;
    u64 su = 0;
    g.template row<kBcHubChunk>(fsize, a.order, first, a.rpA, [&](int u) { su = a.sigma[u]; });
    const long long e = g.e;
    long long pos = g.pos;
    long long dsum = 0;
    unsigned err = 0;
    // the groups of a wave have different trip counts: the loop runs to the wave's longest with the other lanes
    // predicated off, because the append needs the whole wave
    while (__ballot(pos < e) != 0) {                         // (wave-uniform)
        const bool live = pos < e;
        const int w = live ? colA[pos] : 0;
        bc_forward_entry(a, live, w, su, dsum, err, lane);
        pos += W;
    }
    bc_forward_end(dsum, err, a.cnt, lane);
}

// one workgroup per chunk record chunk[cfirst + blockIdx.x]
__global__ __launch_bounds__(kBcThreads) void k_bc_forward_chunk(BcFwd a, int cfirst, const int *__restrict__ colA)
{
    const int lane = lane_id();
    const int2 rec = a.chunk[cfirst + blockIdx.x];
    long long b, e;
    hub_chunk_range<kBcHubChunk>(a.rpA, rec, b, e);
    const u64 su = a.sigma[rec.x];
    long long dsum = 0;
    unsigned err = 0;
    for (long long pos = b + threadIdx.x; __ballot(pos < e) != 0; pos += kBcThreads) {   // (wave-uniform)
        const bool live = pos < e;
        const int w = live ? colA[pos] : 0;
        bc_forward_entry(a, live, w, su, dsum, err, lane);
    }
    bc_forward_end(dsum, err, a.cnt, lane);
}

// (u64) floor(c(w) * (double) sigma(v)) for a successor w one level down, else 0.  The columns were tested by the forward
// launch that walked this row; bounded all the same.
__device__ __forceinline__ u64 bc_summand(const BcBwd &a, int w, double sv)
{
    if ((unsigned)w >= (unsigned)a.n || a.level[w] != a.d + 1) return 0;
    return __double2ull_rz(__dmul_rn(a.c[w], sv));           // (the product is >= 0: truncation is the floor)
}

// v's owner finishes v: delta(v) = s is final
__device__ __forceinline__ void bc_finish_vertex(const BcBwd &a, int v, u64 s)
{
    a.delta[v] = s;
    a.c[v] = __ddiv_rn(__ull2double_rn(kBcOne + s), __ull2double_rn(a.sigma[v]));
    if (v != a.src && s) a.bc[v] += s;
}

__global__ __launch_bounds__(kBcThreads) void k_bc_leaf(BcBwd a, int fsize, int first, const int *__restrict__ order)
{
    const long long t = (long long)blockIdx.x * kBcThreads + threadIdx.x;
    if (t < fsize) bc_finish_vertex(a, order[first + t], 0);
}

template <int W>
__global__ __launch_bounds__(kBcThreads) void k_bc_backward(BcBwd a, int fsize, int first, const int *__restrict__ order,
                                                           const int *__restrict__ colA)
{
    // (open code: with GroupRow of hub_chunks.hpp the same instructions come out in another order)
    const long long t = (long long)blockIdx.x * kBcThreads + threadIdx.x;
    const long long f = t / W;
    const int sub = (int)(t % W);
    bool mine = false;
    int v = 0;
    long long pos = 0, e = 0;
    double sv = 0.0;
    if (f < fsize) {
        v = order[first + f];
        const long long b = a.rpA[v];
        e = a.rpA[v + 1];
        mine = e - b <= kBcHubChunk;                         // (else: the chunks' row, finished by k_bc_hub_finish)
        if (!mine) e = b;
        pos = b + sub;
        sv = __ull2double_rn(a.sigma[v]);
    }
    u64 s = 0;
#pragma unroll 4
    for (; pos < e; pos += W) s += bc_summand(a, colA[pos], sv);
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // (open code: a helper compiles to other code here)
    if (mine && sub == 0) bc_finish_vertex(a, v, s);
}

// one workgroup per chunk record chunk[cfirst + blockIdx.x]: the chunk's sum to delta[hub] by one atomic
__global__ __launch_bounds__(kBcThreads) void k_bc_backward_chunk(BcBwd a, int cfirst, const int2 *__restrict__ chunk,
                                                                 const int *__restrict__ colA)
{
    __shared__ u64 part[kBcWaves];
    const int2 rec = chunk[cfirst + blockIdx.x];
    long long b, e;
    hub_chunk_range<kBcHubChunk>(a.rpA, rec, b, e);
    const double sv = __ull2double_rn(a.sigma[rec.x]);
    u64 s = 0;
#pragma unroll 4
    for (long long pos = b + threadIdx.x; pos < e; pos += kBcThreads) s += bc_summand(a, colA[pos], sv);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);      // (open code: wave_sum compiles to other code here)
    if (lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
#pragma unroll
        for (int q = 0; q < kBcWaves; q++) t += part[q];
        if (t) atomicAdd(&a.delta[rec.x], t);
    }
}

// delta[hub] is complete: the chunks were an earlier launch.  One lane per record; the record of chunk 0 stands for the hub.
__global__ __launch_bounds__(kBcThreads) void k_bc_hub_finish(BcBwd a, int nchunks, int cfirst, const int2 *__restrict__ chunk)
{
    const long long t = (long long)blockIdx.x * kBcThreads + threadIdx.x;
    if (t >= nchunks) return;
    const int2 rec = chunk[cfirst + t];
    if (rec.y == 0) bc_finish_vertex(a, rec.x, a.delta[rec.x]);
}

// Also the call's largest sigma: the wave's maximum goes to the counter by one atomic, and only where it beats what an
// agent-scope load of the counter shows (the counter only grows, so a stale value costs an atomic and nothing else).  In an
// earlier form every finishing wave of the backward sweep sent its maximum: with 64 lanes per vertex that was one atomic
// per vertex on one address, 40 of the 48 ms of a source on R-MAT scale 22.
__global__ __launch_bounds__(kBcThreads) void k_bc_reset(int reached, const int *__restrict__ order, int *__restrict__ level,
                                                        u64 *__restrict__ sigma, u64 *__restrict__ delta, BcCounters *cnt)
{
    const long long t = (long long)blockIdx.x * kBcThreads + threadIdx.x;
    u64 sg = 0;
    if (t < reached) {
        const int v = order[t];
        sg = sigma[v];
        level[v] = -1;
        sigma[v] = 0;
        delta[v] = 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sg = max(sg, (u64)__shfl_xor(sg, off, 64));   // (open code: wave_max compares the other way round)
    if (lane_id() == 0 && sg > __hip_atomic_load(&cnt->sigma_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&cnt->sigma_max, sg);
}

// The lanes per vertex of a level: the smallest W at or above a QUARTER of its mean out-degree.  The push of bfs_tree.hip
// takes the smallest W at or above the mean, because there a frontier hub is a serial tail of degree / W steps; here no
// group walks more than kBcHubChunk entries, and with the mean rule (64 lanes on every big level of an R-MAT of mean degree
// 16) the forward sweep measured 2.2 times and the backward sweep 3 times slower than with 4 lanes.
static int bc_lanes(long long m_f, long long n_f) { return lanes_for_mean(m_f, n_f, 4); }

static void launch_forward(int W, const BcFwd &a, int fsize, int first, const int *colA, hipStream_t s)
{
    const dim3 grid = grid_for((long long)fsize * W, kBcThreads), block(kBcThreads);
    dispatch_lanes(W, [&](auto w) { hipLaunchKernelGGL(k_bc_forward<decltype(w)::value>, grid, block, 0, s, a, fsize, first, colA); });
}

static void launch_backward(int W, const BcBwd &a, int fsize, int first, const int *order, const int *colA, hipStream_t s)
{
    const dim3 grid = grid_for((long long)fsize * W, kBcThreads), block(kBcThreads);
    dispatch_lanes(W, [&](auto w) {
        hipLaunchKernelGGL(k_bc_backward<decltype(w)::value>, grid, block, 0, s, a, fsize, first, order, colA);
    });
}

// a level of the current source, as the host knows it after the level's read-back
struct BcLevelRec {
    int off, size;                      // its slice of order[]
    int coff, chunks;                   // its slice of chunk[]
    long long m;                        // the out-degree sum of its vertices
};

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_betweenness(bspgemm_context *ctx, const bspgemm_matrix *A, int nsources, const int *sources,
                                              uint64_t *bc_fixed_host, double *bc_host, bspgemm_bc_info *info)
{
    static const char who[] = "bspgemm_betweenness";
    if (info) memset(info, 0, sizeof *info);
    // everything below is refused before an operand is dereferenced
    if (!ctx || !A) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_betweenness: NULL argument");
    if (nsources < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_betweenness: nsources < 0");
    if (nsources > 0 && !sources) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_betweenness: NULL sources with nsources > 0");
    for (int i = 0; i < nsources; i++)
        if (sources[i] < 0) {
            snprintf(g_err, sizeof g_err, "%s: source %d (sources[%d]) is negative", who, sources[i], i);
            return BSPGEMM_ERR_INVALID;
        }
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_SQUARE)) return st;
    const int n = A->rows;
    for (int i = 0; i < nsources; i++)
        if (sources[i] >= n) {
            snprintf(g_err, sizeof g_err, "%s: source %d (sources[%d]) outside [0, %d)", who, sources[i], i, n);
            return BSPGEMM_ERR_INVALID;
        }
    if ((long long)nsources * n >= (1ll << 31)) {
        snprintf(g_err, sizeof g_err, "%s: nsources * n = %lld is 2^31 or more", who, (long long)nsources * n);
        return BSPGEMM_ERR_INVALID;
    }
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    if (n == 0) {                                            // no vertex: nothing to write, every count 0
        if (info) info->sources = nsources;
        return BSPGEMM_OK;
    }

    // BSPGEMM_BC_TIMING: host clocks around the stages; every launch group is then synchronised
    StageClock clk(ctx->bc_timing, ctx->stream);
    clk.max_tag[0] = -1;
    double ms_check = 0, ms_fwd = 0, ms_back = 0, ms_bwd = 0, ms_hub = 0, ms_out = 0;
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const int forced_w = ctx->bc_lanes;

    // The workspace grows ONCE here: to what the canonicalisation takes (two transposes) or, if that is more, to the
    // call's own state, which is set up only after the canonical A is there.
    const size_t n4 = ws_pad4((size_t)n), ns4 = ws_pad4((size_t)nsources);
    const size_t chunk_cap = 2 * (size_t)(A->nnz / kBcHubChunk) + 2;   // sum of ceil(len / chunk) over the rows longer than a chunk
    BcCounters *d_cnt = nullptr;
    u64 *sigma = nullptr, *delta = nullptr, *bc = nullptr;
    double *c = nullptr;
    int *level = nullptr, *order = nullptr, *d_src = nullptr, *d_deg = nullptr;
    int2 *chunk = nullptr;
    auto carve = [&](int *tmp) {
        return WsCursor(tmp).take(d_cnt, 1).take(sigma, n4).take(delta, n4).take(c, n4).take(bc, n4).take(level, n4).take(order, n4)
            .take(chunk, chunk_cap).take(d_src, ns4).take(d_deg, ns4).ints();
    };
    const size_t total = std::max(carve(nullptr), transpose_workspace_ints(A->nnz, n));
    if (bspgemm_status st = ensure_tmp(ctx, total)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)A->nnz)) return st;

    bspgemm_matrix *mineA = nullptr;                         // the canonical A that the call owns
    u64 *h_fixed = nullptr;                                  // the sums for bc_host where the caller takes no fixed ones
    int *h_deg = nullptr;                                    // the sources' out-degrees
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_matrix_free(mineA);
        free(h_fixed);
        free(h_deg);
        if (info) memset(info, 0, sizeof *info);
        return st;
    };

    // the canonical check and its read-back: the call's first synchronisation
    clk.start();
    carve(ctx->tmp);
    BcCounters h = {};
    HIPCHK_B(hipMemsetAsync(d_cnt, 0, sizeof(BcCounters), s));
    launch_graph_canonical_checks(ctx, A, nullptr, &d_cnt->canon, s);
    HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));
    if (h.canon & kSetErrRange) return bail(fail_bad_column(who, n));
    int canonicalised = 0;
    if (h.canon & kSetErrOrder) {
        if (bspgemm_status st = operand_canonical(ctx, A, &mineA)) return bail(st);
        if (bspgemm_status st = ensure_tmp(ctx, total)) return bail(st);   // (there already, see above)
        A = mineA;
        canonicalised = 1;
    }
    HIPCHK_B(clk.lap(ms_check, true));
    if (!bc_fixed_host && bc_host) {
        h_fixed = static_cast<u64 *>(malloc((size_t)n * sizeof(u64)));
        if (!h_fixed) return bail(FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_betweenness: host sums"));
    }
    if (nsources > 0) {
        h_deg = static_cast<int *>(malloc((size_t)nsources * sizeof(int)));
        if (!h_deg) return bail(FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_betweenness: host degrees"));
    }

    carve(ctx->tmp);                                         // (again: the canonicalisation may have moved the workspace)
    const dim3 block(kBcThreads);

    clk.start();
    HIPCHK_B(hipMemsetAsync(d_cnt, 0, sizeof(BcCounters), s));
    hipLaunchKernelGGL(k_bc_init, grid_for(n, kBcThreads), block, 0, s, n, level, sigma, delta, bc);
    HIPCHK_B(hipGetLastError());
    if (nsources > 0) {
        HIPCHK_B(hipMemcpyAsync(d_src, sources, (size_t)nsources * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_bc_degrees, grid_for(nsources, kBcThreads), block, 0, s, nsources, d_src, A->d_row_ptr, d_deg);
        HIPCHK_B(round_fetch(h_deg, d_deg, (size_t)nsources * sizeof(int), s));
    }
    (void)clk.lap(ms_back);

    long long reached = 0, edges_forward = 0, hub_chunks = 0;
    int depth_max = 0, levels = 0;
    std::vector<BcLevelRec> L;
    try {
        for (int i = 0; i < nsources; i++) {
            const int src = sources[i];
            const host_clock::time_point t_src = host_clock::now();
            if (h_deg[i] < 0 || h_deg[i] > A->nnz) return bail(fail_stuck(who));
            L.clear();
            L.push_back(BcLevelRec{0, 1, 0, hub_chunks_over<kBcHubChunk>(h_deg[i]), h_deg[i]});
            if ((size_t)L[0].chunks > chunk_cap) return bail(fail_stuck(who));
            hipLaunchKernelGGL(k_bc_source, dim3(1), block, 0, s, src, h_deg[i], level, sigma, order, chunk, (int)chunk_cap, d_cnt);
            HIPCHK_B(hipGetLastError());
            int tail = 1, ctail = L[0].chunks;
            long long deg = L[0].m;

            // ---- forward: level d from level d - 1, while that one has entries to walk
            for (int d = 1; L.back().m > 0; d++) {
                if (d > n) return bail(fail_stuck(who));     // defensive: a level holds at least one new vertex
                const BcLevelRec f = L.back();
                const BcFwd a = {n, d, A->d_row_ptr, level, sigma, order, chunk, (int)chunk_cap, d_cnt};
                clk.start();
                launch_forward(forced_w ? forced_w : bc_lanes(f.m, f.size), a, f.size, f.off, A->d_col_idx, s);
                HIPCHK_B(hipGetLastError());
                HIPCHK_B(clk.lap(ms_fwd, true));
                if (f.chunks) {
                    hipLaunchKernelGGL(k_bc_forward_chunk, dim3((unsigned)f.chunks), block, 0, s, a, f.coff, A->d_col_idx);
                    HIPCHK_B(hipGetLastError());
                    HIPCHK_B(clk.lap(ms_hub, true));
                }
                levels++;
                edges_forward += f.m;
                hub_chunks += f.chunks;
                HIPCHK_B(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
                HIPCHK_B(hipStreamSynchronize(s));           // the level's one synchronisation
                (void)clk.lap(ms_back);
                if (h.err & kBcErrRange) return bail(fail_bad_column(who, n));
                if (h.err & kBcErrOverflow) {
                    snprintf(g_err, sizeof g_err, "%s: a shortest-path count of 2^63 or more from source %d (sources[%d]) at level %d",
                             who, src, i, d);
                    return bail(BSPGEMM_ERR_OVERFLOW);
                }
                const BcLevelRec nx = {tail, h.tail - tail, ctail, h.ctail - ctail, (long long)h.deg - deg};
                if (nx.size < 0 || h.tail > n || nx.chunks < 0 || (size_t)h.ctail > chunk_cap || nx.m < 0 || (long long)h.deg > A->nnz)
                    return bail(fail_stuck(who));
                if (nx.size == 0) break;
                L.push_back(nx);
                tail = h.tail;
                ctail = h.ctail;
                deg = (long long)h.deg;
            }
            const int depth = (int)L.size() - 1;

            // ---- backward: no read-backs, the host knows every offset
            BcBwd b = {n, depth, src, A->d_row_ptr, level, sigma, delta, c, bc};
            clk.start();
            hipLaunchKernelGGL(k_bc_leaf, grid_for(L[depth].size, kBcThreads), block, 0, s, b, L[depth].size, L[depth].off, order);
            for (int d = depth - 1; d >= 0; d--) {
                const BcLevelRec &f = L[d];
                b.d = d;
                launch_backward(forced_w ? forced_w : bc_lanes(f.m, f.size), b, f.size, f.off, order, A->d_col_idx, s);
                if (f.chunks) {
                    HIPCHK_B(clk.lap(ms_bwd, true));            // (timed: the hub launches are a lap of their own)
                    hipLaunchKernelGGL(k_bc_backward_chunk, dim3((unsigned)f.chunks), block, 0, s, b, f.coff, chunk, A->d_col_idx);
                    hipLaunchKernelGGL(k_bc_hub_finish, grid_for(f.chunks, kBcThreads), block, 0, s, b, f.chunks, f.coff, chunk);
                    hub_chunks += f.chunks;
                    HIPCHK_B(clk.lap(ms_hub, true));
                }
            }
            hipLaunchKernelGGL(k_bc_reset, grid_for(tail, kBcThreads), block, 0, s, tail, order, level, sigma, delta, d_cnt);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_bwd, true));
            clk.longest(ms_since(t_src), i);
            reached += tail;
            depth_max = std::max(depth_max, depth);
        }
    } catch (const std::bad_alloc &) {
        return bail(FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_betweenness: host level records"));
    }

    // the read-out: the sums and the largest path count, behind the call's last synchronisation
    clk.start();
    u64 *fixed = bc_fixed_host ? reinterpret_cast<u64 *>(bc_fixed_host) : h_fixed;
    if (fixed) HIPCHK_B(hipMemcpyAsync(fixed, bc, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));
    if (bc_host)
        for (int v = 0; v < n; v++) bc_host[v] = std::ldexp((double)fixed[v], -32);
    if (clk.on) {
        (void)clk.lap(ms_out);
        fprintf(stderr, "[bspgemm] %s: n %d nnz %lld sources %d reached %lld depth %d levels %d hub chunks %lld (%d lanes) | total %.3f ms = "
                        "canonical check %.3f + forward launches %.3f + read-backs %.3f + backward launches %.3f + hub launches %.3f + "
                        "read-out %.3f + rest | slowest source %.3f ms (sources[%d])\n",
                who, n, (long long)A->nnz, nsources, reached, depth_max, levels, hub_chunks, forced_w, clk.total(), ms_check, ms_fwd,
                ms_back, ms_bwd, ms_hub, ms_out, clk.max_ms, clk.max_tag[0]);
    }
    bspgemm_matrix_free(mineA);
    free(h_fixed);
    free(h_deg);
    if (info) {
        info->sigma_max = (uint64_t)h.sigma_max;
        info->reached = reached;
        info->edges_forward = edges_forward;
        info->hub_chunks = hub_chunks;
        info->sources = nsources;
        info->depth_max = depth_max;
        info->levels = levels;
        info->canonicalised = canonicalised;
    }
    return BSPGEMM_OK;
}
