// pagerank.hip -- PageRank in unsigned 64-bit fixed point, everything device-resident: bspgemm_pagerank (include/bspgemm.h,
// which holds the definition).  No product, no sort, no intersection: a pull iteration is a gather-and-sum
// over the rows of AT, a push iteration an entry-parallel walk of A with 64-bit atomics.  The arrays, all in the context's
// workspace, grown once before anything is launched:
//     r[n]        the ranks, 2^62 = 1.0                               c[2][n]   c(u) = floor(r(u) / outdeg(u)), 0 for a
//     acc[n]      64-bit accumulators: the hubs' partial sums (PULL),           dangling u: an iteration reads one and
//                 every vertex's s(v) (PUSH); zero between iterations           writes the other
//     list[4][n]  the vertices of each in-degree class, built once per call (PULL)
//     chunk[]     {hub, chunk number} for every kPrHubChunk entries of a hub's row (PULL)
// and PrCounters: three dangling words, two delta words, the mass, the dangling count, the canonical checks' error word,
// the list sizes.
//     k_pr_init       per vertex: r = q, c[0] = q / outdeg, acc = 0; the dangling count and the first dangling sum
//     k_pr_classify   per vertex: class = max(own, BSPGEMM_OPT_PR_MIN_CLASS), own = 0 for an in-degree d <= kPrLaneCap (0
//                     included), 1 for d <= kPrWaveCap, 2 for d <= kPrGroupCap, else 3; appended to its class list (ballot,
//                     one atomicAdd per wave and class); a hub takes ceil(d / kPrHubChunk) chunk records from a cursor
//     k_pr_lane       one lane per vertex of list 0: up to kPrLaneCap gathers of c[u]
//     k_pr_wave<W>    W = 64 or 16 lanes per vertex of list 1 (16 where the class's rows have at most 32 entries in the mean:
//                     four vertices per wave): the lanes stride over the row of AT and reduce across their group
//     k_pr_group      one workgroup per vertex of list 2: the same, joined through LDS
//     k_pr_hub_chunk  one workgroup per chunk record: the chunk's sum goes to acc[hub] by ONE device-scope atomicAdd
//     k_pr_finish     a later launch, one lane per hub: s = acc[v], acc[v] = 0; PUSH's finish too, over every vertex
//     k_pr_push       per stored entry (u, v) of A, in select's geometry (sel_rows.hpp): atomicAdd(&acc[v], c[u])
//     k_pr_mass       at the end: the sum of r
// Whoever finishes v (pr_vertex) computes r_t(v) = B + floor(D * (share + s) / 2^32), adds |r_t - r_{t-1}| to its delta,
// stores r[v] and c_next[v] = r_t(v) / outdeg(v), and adds r_t(v) to the NEXT dangling sum when v is dangling: there is no
// separate contribution pass, and the 64-by-32-bit division happens once per vertex and iteration.  The deltas and
// dangling sums of a workgroup are joined (wave shuffles, then LDS) and reach the counters by one atomic per workgroup;
// the vertex-parallel kernels run grid-stride loops over at most kPrMaxBlocks workgroups, so a counter takes a few
// thousand atomics per launch however many vertices there are.
//
// The words an iteration reads and writes.  Iteration t = 1, 2, ... reads dang[(t - 1) % 3] (plain load: written by
// EARLIER launches only), adds to dang[t % 3] and delta[t & 1], and its first launch zeroes dang[(t + 1) % 3] and
// delta[(t + 1) & 1], which nothing else touches in iteration t: the first was last read in iteration t - 1, the second
// was read by the host (tolerance > 0) before iteration t was issued.  c_in = c[(t - 1) & 1] is only read, c_out = c[t & 1]
// and r[v] are written by v's one owner.  acc is touched by atomics only in the launch that accumulates and read and
// zeroed plainly by the finishing launch behind it.  Launches of one stream run in order, nothing reads plainly what the
// same launch writes, no kernel waits for another workgroup: every loop is bounded by a row, a list size or a chunk
// count that the host passed in.  Integer addition commutes, so pull, push, every class and every split of a hub row
// give the same bits.  With tolerance == 0 the loop has no read-back and no synchronisation; with tolerance > 0 one
// 8-byte read-back per iteration.
#include "internal.hpp"
#include "hub_chunks.hpp"
#include "sel_rows.hpp"

#include <algorithm>
#include <cmath>

namespace bsp {

constexpr int kPrThreads = 256;
constexpr int kPrWaves = kPrThreads / 64;
constexpr int kPrLaneCap = 8;           // the longest row of AT one lane sums (tests/pagerank_ref.py mirrors the caps)
constexpr int kPrWaveCap = 256;         // the longest row one wave sums: four gathers per lane
constexpr int kPrGroupCap = 4096;       // the longest row one workgroup sums: sixteen gathers per thread
constexpr int kPrHubChunk = 4096;       // entries of a hub's row that one workgroup sums
constexpr int kPrClasses = 4;
constexpr int kPrMaxBlocks = 2048;      // workgroups of a grid-stride launch: eight per CU of a 256-CU device

struct PrCounters {
    u64 dang[3];                        // the dangling sums, rotated
    u64 delta[2];                       // the L1 changes, alternating
    u64 mass;
    u64 ndangling;
    u64 wave_entries;                   // the entries of the wave class's rows: their mean picks the lanes per row
    u64 pad;
    unsigned canon;                     // the canonical checks: two bits per operand (kSetErrRange, kSetErrOrder), A / AT
    int chunks;                         // chunk records handed out
    int size[kPrClasses];               // vertices of the class lists
};

// what every launch of an iteration gets
struct PrArgs {
    int n;
    u64 B, D;
    const int *rpA;                     // outdeg(v) = rpA[v + 1] - rpA[v]: A is canonical
    const u64 *c_in;
    u64 *c_out, *r;
    const u64 *dang_in;
    u64 *dang_out, *delta;
    u64 *zero0, *zero1;                 // the first launch of an iteration: the words of the iteration after it; else NULL
};

struct PrSums {
    u64 delta, dang;
};

__device__ __forceinline__ void pr_begin(const PrArgs &a)
{
    if (a.zero0 && blockIdx.x == 0 && threadIdx.x == 0) {
        *a.zero0 = 0;
        *a.zero1 = 0;
    }
}

// floor(D * x / 2^32) for D <= 2^32 and x < 2^63: exact, and every term stays in 64 bits
__device__ __forceinline__ u64 pr_scale(u64 D, u64 x) { return D * (x >> 32) + ((D * (x & 0xffffffffull)) >> 32); }

// v's owner finishes v: s = the sum of c(u) over v's in-neighbours
__device__ __forceinline__ void pr_vertex(const PrArgs &a, int v, u64 s, u64 share, PrSums &sums)
{
    const u64 rn = a.B + pr_scale(a.D, share + s);
    const u64 ro = a.r[v];
    sums.delta += rn > ro ? rn - ro : ro - rn;
    a.r[v] = rn;
    const unsigned od = (unsigned)(a.rpA[v + 1] - a.rpA[v]);
    a.c_out[v] = od ? rn / (u64)od : 0;
    if (!od) sums.dang += rn;
}

// the workgroup's sums to the two counters, one atomic each.  Every thread of the workgroup, once, at the kernel's end.
// (The join through LDS is written out here and in pr_group_sum: the two sums share one barrier here, and there the wave
// sum stands in front of the leading barrier; a shared workgroup sum compiles to other code in both.)
__device__ __forceinline__ void pr_commit(PrSums sums, u64 *delta, u64 *dang)
{
    __shared__ u64 red[2][kPrWaves];
    const u64 d = wave_sum(sums.delta), g = wave_sum(sums.dang);
    if (lane_id() == 0) {
        red[0][threadIdx.x >> 6] = d;
        red[1][threadIdx.x >> 6] = g;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 ds = 0, gs = 0;
#pragma unroll
        for (int q = 0; q < kPrWaves; q++) {
            ds += red[0][q];
            gs += red[1][q];
        }
        if (ds) atomicAdd(delta, ds);
        if (gs) atomicAdd(dang, gs);
    }
}

// cnt was zeroed by the host
__global__ __launch_bounds__(kPrThreads) void k_pr_init(int n, u64 q, const int *__restrict__ rpA, u64 *__restrict__ r,
                                                       u64 *__restrict__ c0, u64 *__restrict__ acc, PrCounters *cnt)
{
    PrSums sums = {0, 0};                                    // (delta: the dangling count here)
    for (long long v = (long long)blockIdx.x * kPrThreads + threadIdx.x; v < n; v += (long long)gridDim.x * kPrThreads) {
        const unsigned od = (unsigned)(rpA[v + 1] - rpA[v]);
        r[v] = q;
        c0[v] = od ? q / (u64)od : 0;
        acc[v] = 0;
        if (!od) {
            sums.delta += 1;
            sums.dang += q;
        }
    }
    pr_commit(sums, &cnt->ndangling, &cnt->dang[0]);
}

__device__ __forceinline__ int pr_class_of(int d)
{
    return d <= kPrLaneCap ? 0 : d <= kPrWaveCap ? 1 : d <= kPrGroupCap ? 2 : 3;
}

// list: kPrClasses lists, `stride` ints apart; chunk: chunk_cap records
__global__ __launch_bounds__(kPrThreads) void k_pr_classify(int n, int min_class, const int *__restrict__ rpT,
                                                           int *__restrict__ list, size_t stride, int2 *__restrict__ chunk,
                                                           int chunk_cap, PrCounters *cnt)
{
    const int lane = lane_id();
    const long long v = (long long)blockIdx.x * kPrThreads + threadIdx.x;
    int cls = -1;
    PrSums sums = {0, 0};                                    // (delta: the entries of the wave class here)
    if (v < n) {
        const int d = rpT[v + 1] - rpT[v];
        cls = max(pr_class_of(d), min_class);
        if (cls == 1) sums.delta = (u64)d;
        if (cls == 3 && d > 0) hub_chunks_emit((int)v, hub_chunks_of<kPrHubChunk>(d), &cnt->chunks, chunk, chunk_cap);
    }
#pragma unroll
    for (int c = 0; c < kPrClasses; c++) wave_append(cls == c, (int)v, list + c * stride, &cnt->size[c], n, lane);
    pr_commit(sums, &cnt->wave_entries, &cnt->wave_entries); // (the second sum is 0: no atomic)
}

// ---------------------------------------------------------------- PULL -------------------------------------------------
// The columns of AT are in [0, n): the canonical check tested a given AT before the first launch, and a transpose that the
// call made holds nothing else.
__global__ __launch_bounds__(kPrThreads) void k_pr_lane(PrArgs a, int count, const int *__restrict__ list,
                                                       const int *__restrict__ rpT, const int *__restrict__ colT)
{
    pr_begin(a);
    const u64 share = *a.dang_in / (u64)a.n;
    PrSums sums = {0, 0};
    for (long long i = (long long)blockIdx.x * kPrThreads + threadIdx.x; i < count; i += (long long)gridDim.x * kPrThreads) {
        const int v = list[i];
        const long long b = rpT[v];
        const int d = min(rpT[v + 1] - (int)b, kPrLaneCap);  // (the list holds rows of at most kPrLaneCap entries)
        int u[kPrLaneCap];
#pragma unroll
        for (int j = 0; j < kPrLaneCap; j++) u[j] = j < d ? colT[b + j] : 0;
        u64 s = 0;
#pragma unroll
        for (int j = 0; j < kPrLaneCap; j++) s += j < d ? a.c_in[u[j]] : 0;
        pr_vertex(a, v, s, share, sums);
    }
    pr_commit(sums, a.delta, a.dang_out);
}

// W lanes per vertex of list 1, 64 / W vertices per wave: the lanes of a group stride over the row and join by shuffles
// inside the group.  The outer loop is wave-uniform (the shuffles need the whole wave); the groups' rows differ in length.
template <int W>
__global__ __launch_bounds__(kPrThreads) void k_pr_wave(PrArgs a, int count, const int *__restrict__ list,
                                                       const int *__restrict__ rpT, const int *__restrict__ colT)
{
    constexpr int G = 64 / W;
    pr_begin(a);
    const u64 share = *a.dang_in / (u64)a.n;
    const int lane = lane_id(), sub = lane & (W - 1);
    PrSums sums = {0, 0};
    for (long long i0 = ((long long)blockIdx.x * kPrWaves + (threadIdx.x >> 6)) * G; i0 < count;
         i0 += (long long)gridDim.x * kPrWaves * G) {
        const long long i = i0 + lane / W;
        const bool live = i < count;
        const int v = live ? list[i] : 0;
        const long long e = live ? rpT[v + 1] : 0;
        u64 s = 0;
#pragma unroll 4
        for (long long p = live ? (long long)rpT[v] + sub : 0; p < e; p += W) s += a.c_in[colT[p]];
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // (open code: a helper compiles to other code here)
        if (live && sub == 0) pr_vertex(a, v, s, share, sums);
    }
    pr_commit(sums, a.delta, a.dang_out);
}

// the sum of c_in[colT[b .. e)] by the whole workgroup, in every thread's return value; `part`: kPrWaves words of LDS
__device__ __forceinline__ u64 pr_group_sum(const u64 *__restrict__ c_in, const int *__restrict__ colT, long long b, long long e,
                                            u64 *part)
{
    u64 s = 0;
#pragma unroll 4
    for (long long p = b + threadIdx.x; p < e; p += kPrThreads) s += c_in[colT[p]];
    s = wave_sum(s);
    __syncthreads();                                         // (the words' readers of the round before are done)
    if (lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int q = 0; q < kPrWaves; q++) t += part[q];
    return t;
}

__global__ __launch_bounds__(kPrThreads) void k_pr_group(PrArgs a, int count, const int *__restrict__ list,
                                                        const int *__restrict__ rpT, const int *__restrict__ colT)
{
    __shared__ u64 part[kPrWaves];
    pr_begin(a);
    const u64 share = *a.dang_in / (u64)a.n;
    PrSums sums = {0, 0};
    for (int i = blockIdx.x; i < count; i += gridDim.x) {    // (uniform over the workgroup)
        const int v = list[i];
        const u64 s = pr_group_sum(a.c_in, colT, rpT[v], rpT[v + 1], part);
        if (threadIdx.x == 0) pr_vertex(a, v, s, share, sums);
    }
    pr_commit(sums, a.delta, a.dang_out);
}

// one workgroup per chunk record: a hub costs what its entries cost
__global__ __launch_bounds__(kPrThreads) void k_pr_hub_chunk(PrArgs a, int nchunks, const int2 *__restrict__ chunk,
                                                            const int *__restrict__ rpT, const int *__restrict__ colT, u64 *acc)
{
    __shared__ u64 part[kPrWaves];
    pr_begin(a);
    for (int i = blockIdx.x; i < nchunks; i += gridDim.x) {  // (uniform over the workgroup)
        const int2 rec = chunk[i];
        long long b, e;
        hub_chunk_range<kPrHubChunk>(rpT, rec, b, e);
        const u64 s = pr_group_sum(a.c_in, colT, b, e, part);
        if (threadIdx.x == 0 && s) atomicAdd(&acc[rec.x], s);
    }
}

// acc is complete: the chunks were an earlier launch.  Also PUSH's finish (list == NULL: every vertex).
__global__ __launch_bounds__(kPrThreads) void k_pr_finish(PrArgs a, int count, const int *__restrict__ list, u64 *__restrict__ acc)
{
    pr_begin(a);
    const u64 share = *a.dang_in / (u64)a.n;
    PrSums sums = {0, 0};
    for (long long i = (long long)blockIdx.x * kPrThreads + threadIdx.x; i < count; i += (long long)gridDim.x * kPrThreads) {
        const int v = list ? list[i] : (int)i;
        const u64 s = acc[v];
        acc[v] = 0;
        pr_vertex(a, v, s, share, sums);
    }
    pr_commit(sums, a.delta, a.dang_out);
}

// ---------------------------------------------------------------- PUSH -------------------------------------------------
struct PrPushOp {
    const u64 *__restrict__ c_in;
    u64 *acc;
    int n, cur;
    u64 cu;
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int u)
    {
        if (u == cur) return;                                // (the walk enters the row again at every step)
        cur = u;
        cu = c_in[u];
    }
    __device__ __forceinline__ void entry(int, long long, int v, int)
    {
        if (cu && (unsigned)v < (unsigned)n) atomicAdd(&acc[v], cu);   // (v in [0, n): the canonical check; bounded all the same)
    }
};

__global__ __launch_bounds__(kSelThreads) void k_pr_push(PrArgs a, const int *__restrict__ colA, long long E, bool vec,
                                                        const int *__restrict__ tile_row, u64 *acc)
{
    pr_begin(a);
    PrPushOp op = {a.c_in, acc, a.n, -1, 0};
    sel_walk_entries<false>(a.rpA, colA, a.n, E, vec, tile_row, op);
}

__global__ __launch_bounds__(kPrThreads) void k_pr_mass(int n, const u64 *__restrict__ r, PrCounters *cnt)
{
    PrSums sums = {0, 0};
    for (long long v = (long long)blockIdx.x * kPrThreads + threadIdx.x; v < n; v += (long long)gridDim.x * kPrThreads)
        sums.delta += r[v];
    pr_commit(sums, &cnt->mass, &cnt->mass);                 // (the second sum is 0: no atomic)
}

static dim3 pr_grid(long long items, int per_block)
{
    const long long blocks = (items + per_block - 1) / per_block;
    return dim3((unsigned)std::max(1ll, std::min(blocks, (long long)kPrMaxBlocks)));
}

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_pagerank(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT,
                                           bspgemm_pr_method method, double damping, int max_iter, double tolerance,
                                           uint64_t *rank_fixed_host, double *rank_host, bspgemm_pr_info *info)
{
    static const char who[] = "bspgemm_pagerank";
    if (info) memset(info, 0, sizeof *info);
    // everything below is refused before an operand is dereferenced
    if (!ctx || !A) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_pagerank: NULL argument");
    if (method != BSPGEMM_PR_AUTO && method != BSPGEMM_PR_PULL && method != BSPGEMM_PR_PUSH)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_pagerank: unknown method");
    if (!(damping >= 0.0 && damping <= 1.0)) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_pagerank: damping outside [0, 1]");
    if (max_iter < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_pagerank: max_iter < 0");
    if (!(tolerance >= 0.0)) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_pagerank: tolerance < 0");
    if (bspgemm_status st = check_graph_operand(ctx, A, who, NEED_SQUARE)) return st;
    const int n = A->rows;
    const bool pull = method != BSPGEMM_PR_PUSH;             // AUTO is PULL (include/bspgemm.h)
    if (!pull) AT = nullptr;                                 // ignored
    if (bspgemm_status st = check_transposed_operand(ctx, A, AT, who)) return st;
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_ENTRIES_CONSISTENT)) return st;
    const u64 thr = tolerance >= 4.0 ? ~0ull : (u64)std::floor(std::ldexp(tolerance, 62));
    if (n == 0) {                                            // no vertex: every sum is empty, every delta 0
        if (info) {
            info->iterations = tolerance > 0 ? std::min(max_iter, 1) : max_iter;
            info->converged = tolerance > 0 && max_iter > 0;
            info->method = pull ? BSPGEMM_PR_PULL : BSPGEMM_PR_PUSH;
        }
        return BSPGEMM_OK;
    }
    const u64 ONE = 1ull << 62, q = ONE / (u64)n;
    const u64 D = (u64)std::floor(damping * 4294967296.0 + 0.5);
    const u64 Dc = 4294967296ull - D;                        // ((2^32 - D) * q) >> 32 without leaving 64 bits, as pr_scale does it
    const u64 B = Dc * (q >> 32) + ((Dc * (q & 0xffffffffull)) >> 32);

    // BSPGEMM_PR_TIMING: host clocks around the stages; every class's launch is then synchronised
    StageClock clk(ctx->pr_timing, ctx->stream);
    double ms_check = 0, ms_tr = 0, ms_lists = 0, ms_iter = 0, ms_out = 0, ms_class[kPrClasses + 1] = {};
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const bool own_at = pull && !AT;

    // The workspace grows ONCE here: to what a transpose takes (the call may run up to two) or, if that is more, to the
    // call's own state, which is set up only after the last transpose has finished with the leading part.
    const long long nnz_max = std::max(A->nnz, AT ? AT->nnz : 0);
    const size_t n4 = ws_pad4((size_t)n);
    const size_t chunk_cap = pull ? (size_t)n + (size_t)(nnz_max / kPrHubChunk) + 1 : 0;
    if (chunk_cap > (size_t)INT_MAX) return FAIL(BSPGEMM_ERR_OVERFLOW, "bspgemm_pagerank: too many hub chunks");
    PrCounters *d_cnt = nullptr;
    u64 *r = nullptr, *c[2] = {nullptr, nullptr}, *acc = nullptr;
    int *list = nullptr;
    int2 *chunk = nullptr;
    auto carve = [&](int *tmp) {
        return WsCursor(tmp).take(d_cnt, 1).take(r, n4).take(c[0], n4).take(c[1], n4).take(acc, n4)
            .take(list, pull ? kPrClasses * n4 : 0).take(chunk, chunk_cap).ints();
    };
    const size_t total = std::max(carve(nullptr), transpose_workspace_ints(nnz_max, n));
    if (bspgemm_status st = ensure_tmp(ctx, total)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)nnz_max)) return st;

    bspgemm_matrix *mineA = nullptr, *mineT = nullptr;       // the canonical A, and the transpose or canonical AT, that the call owns
    u64 *h_fixed = nullptr;                                  // the ranks for rank_host where the caller takes no fixed ones
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_matrix_free(mineA);
        bspgemm_matrix_free(mineT);
        free(h_fixed);
        if (info) memset(info, 0, sizeof *info);
        return st;
    };

    // the canonical check of every distinct handle, and its read-back: the call's first synchronisation
    clk.start();
    carve(ctx->tmp);
    PrCounters h = {};
    HIPCHK_B(hipMemsetAsync(d_cnt, 0, sizeof(PrCounters), s));
    launch_graph_canonical_checks(ctx, A, AT, &d_cnt->canon, s);
    HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));
    (void)clk.lap(ms_check);
    if (h.canon & (kSetErrRange | (kSetErrRange << 2))) return bail(fail_bad_column_in(who, n, h.canon));
    const bool a_untidy = (h.canon & kSetErrOrder) != 0;
    const bool at_untidy = AT && (AT == A ? a_untidy : (h.canon & (kSetErrOrder << 2)) != 0);
    int canonicalised = (a_untidy ? 1 : 0) | (at_untidy ? 2 : 0), transposed = 0;
    if (own_at) {                                            // the transpose of any A is canonical, and so is its transpose
        if (bspgemm_status st = bspgemm_matrix_transpose(ctx, A, &mineT)) return bail(st);
        transposed = 1;
        if (a_untidy)
            if (bspgemm_status st = bspgemm_matrix_transpose(ctx, mineT, &mineA)) return bail(st);
        AT = mineT;
    } else {
        if (a_untidy)
            if (bspgemm_status st = operand_canonical(ctx, A, &mineA)) return bail(st);
        if (at_untidy) {
            if (AT == A) {
                AT = mineA;
            } else {
                if (bspgemm_status st = operand_canonical(ctx, AT, &mineT)) return bail(st);
                AT = mineT;
            }
        }
    }
    if (mineA) A = mineA;
    HIPCHK_B(clk.lap(ms_tr, true));
    if (bspgemm_status st = ensure_tmp(ctx, total)) return bail(st);   // (there already, see above)
    if (!rank_fixed_host && rank_host) {
        h_fixed = static_cast<u64 *>(malloc((size_t)n * sizeof(u64)));
        if (!h_fixed) return bail(FAIL(BSPGEMM_ERR_ALLOC, "bspgemm_pagerank: host ranks"));
    }

    carve(ctx->tmp);                                         // (again: the transposes may have moved the workspace)
    const long long E = A->nnz;
    const dim3 block(kPrThreads);
    int wave_lanes = 64;

    clk.start();
    HIPCHK_B(hipMemsetAsync(d_cnt, 0, sizeof(PrCounters), s));
    hipLaunchKernelGGL(k_pr_init, pr_grid(n, kPrThreads), block, 0, s, n, q, A->d_row_ptr, r, c[0], acc, d_cnt);
    HIPCHK_B(hipGetLastError());
    if (pull) {
        hipLaunchKernelGGL(k_pr_classify, dim3((unsigned)(((long long)n + kPrThreads - 1) / kPrThreads)), block, 0, s, n,
                           ctx->pr_min_class, AT->d_row_ptr, list, n4, chunk, (int)chunk_cap, d_cnt);
        HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));
        long long listed = 0;
        for (int k = 0; k < kPrClasses; k++) {
            if (h.size[k] < 0 || h.size[k] > n) return bail(fail_stuck(who));
            listed += h.size[k];
        }
        if (listed != n || h.chunks < 0 || (size_t)h.chunks > chunk_cap) return bail(fail_stuck(who));
        // the wave class: 16 lanes per row where its rows have 32 entries or fewer in the mean, else 64
        if (h.size[1] && h.wave_entries <= 32ull * (u64)h.size[1]) wave_lanes = 16;
    } else if (!pull && max_iter > 0 && E > 0) {
        launch_select_tile_rows(A->d_row_ptr, n, ctx->tile_row, s);
        HIPCHK_B(hipGetLastError());
    }
    HIPCHK_B(clk.lap(ms_lists, true));

    int iterations = 0, converged = 0;
    while (iterations < max_iter) {
        const int it = ++iterations;
        PrArgs a = {n, B, D, A->d_row_ptr, c[(it - 1) & 1], c[it & 1], r, &d_cnt->dang[(it - 1) % 3], &d_cnt->dang[it % 3],
                    &d_cnt->delta[it & 1], &d_cnt->dang[(it + 1) % 3], &d_cnt->delta[(it + 1) & 1]};
        StageClock cls(clk.on, s);                           // under BSPGEMM_PR_TIMING: a synchronisation behind every class
        auto lap = [&](int k) {
            a.zero0 = a.zero1 = nullptr;                     // (the launches behind the first)
            return cls.lap(ms_class[k], true);
        };
        if (pull) {
            if (h.size[0]) {
                hipLaunchKernelGGL(k_pr_lane, pr_grid(h.size[0], kPrThreads), block, 0, s, a, h.size[0], list, AT->d_row_ptr,
                                   AT->d_col_idx);
                HIPCHK_B(lap(0));
            }
            if (h.size[1]) {
                if (wave_lanes == 16)
                    hipLaunchKernelGGL(k_pr_wave<16>, pr_grid(h.size[1], kPrWaves * 4), block, 0, s, a, h.size[1], list + n4,
                                       AT->d_row_ptr, AT->d_col_idx);
                else
                    hipLaunchKernelGGL(k_pr_wave<64>, pr_grid(h.size[1], kPrWaves), block, 0, s, a, h.size[1], list + n4,
                                       AT->d_row_ptr, AT->d_col_idx);
                HIPCHK_B(lap(1));
            }
            if (h.size[2]) {
                hipLaunchKernelGGL(k_pr_group, pr_grid(h.size[2], 1), block, 0, s, a, h.size[2], list + 2 * n4, AT->d_row_ptr,
                                   AT->d_col_idx);
                HIPCHK_B(lap(2));
            }
            if (h.size[3]) {
                if (h.chunks) {
                    hipLaunchKernelGGL(k_pr_hub_chunk, pr_grid(h.chunks, 1), block, 0, s, a, h.chunks, chunk, AT->d_row_ptr,
                                       AT->d_col_idx, acc);
                    a.zero0 = a.zero1 = nullptr;
                }
                hipLaunchKernelGGL(k_pr_finish, pr_grid(h.size[3], kPrThreads), block, 0, s, a, h.size[3], list + 3 * n4, acc);
                HIPCHK_B(lap(3));
            }
        } else {
            if (E > 0) {
                hipLaunchKernelGGL(k_pr_push, dim3(select_tiles(E)), dim3(kSelThreads), 0, s, a, A->d_col_idx, E,
                                   aligned16(A->d_col_idx), ctx->tile_row, acc);
                a.zero0 = a.zero1 = nullptr;
            }
            hipLaunchKernelGGL(k_pr_finish, pr_grid(n, kPrThreads), block, 0, s, a, n, (const int *)nullptr, acc);
            HIPCHK_B(lap(kPrClasses));
        }
        HIPCHK_B(hipGetLastError());
        clk.longest(cls.total(), it);
        if (tolerance > 0) {                                 // the iteration's one read-back, 8 bytes
            u64 delta = 0;
            HIPCHK_B(hipMemcpyAsync(&delta, &d_cnt->delta[it & 1], sizeof delta, hipMemcpyDeviceToHost, s));
            HIPCHK_B(hipStreamSynchronize(s));
            if (delta <= thr) {
                converged = 1;
                break;
            }
        }
    }
    HIPCHK_B(clk.lap(ms_iter, true));

    // the read-out: the mass, the counters and the ranks, behind the call's one synchronisation of the tolerance == 0 form
    u64 *fixed = rank_fixed_host ? reinterpret_cast<u64 *>(rank_fixed_host) : h_fixed;
    hipLaunchKernelGGL(k_pr_mass, pr_grid(n, kPrThreads), block, 0, s, n, r, d_cnt);
    HIPCHK_B(hipGetLastError());
    if (fixed) HIPCHK_B(hipMemcpyAsync(fixed, r, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, s));
    const int sizes[kPrClasses] = {h.size[0], h.size[1], h.size[2], h.size[3]};
    HIPCHK_B(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));
    if (h.ndangling > (u64)n) return bail(fail_stuck(who));   // (the mass is no test: under a wrong AT it is whatever the sums wrap to)
    if (rank_host)
        for (int v = 0; v < n; v++) rank_host[v] = std::ldexp((double)fixed[v], -62);
    if (clk.on) {
        (void)clk.lap(ms_out);
        fprintf(stderr, "[bspgemm] %s: n %d nnz %lld %s classes %d/%d/%d/%d (%d lanes per wave-class row) chunks %d dangling %llu | total %.3f ms = canonical "
                        "check %.3f + transpose %.3f + classify %.3f + %d iterations %.3f (lane %.3f, wave %.3f, workgroup %.3f, "
                        "hub %.3f, push %.3f) + read-out %.3f + rest | longest iteration %.3f ms (iteration %d)\n",
                who, n, E, pull ? "pull" : "push", sizes[0], sizes[1], sizes[2], sizes[3], wave_lanes, pull ? h.chunks : 0,
                (unsigned long long)h.ndangling, clk.total(), ms_check, ms_tr, ms_lists, iterations, ms_iter, ms_class[0],
                ms_class[1], ms_class[2], ms_class[3], ms_class[4], ms_out, clk.max_ms, clk.max_tag[0]);
    }
    bspgemm_matrix_free(mineA);
    bspgemm_matrix_free(mineT);
    free(h_fixed);
    if (info) {
        info->mass = (uint64_t)h.mass;
        info->delta = (uint64_t)h.delta[iterations & 1];
        info->dangling = (int64_t)h.ndangling;
        if (pull)
            for (int k = 0; k < kPrClasses; k++) info->class_vertices[k] = sizes[k];
        info->iterations = iterations;
        info->converged = converged;
        info->method = pull ? BSPGEMM_PR_PULL : BSPGEMM_PR_PUSH;
        info->transposed = transposed;
        info->canonicalised = canonicalised;
    }
    return BSPGEMM_OK;
}
