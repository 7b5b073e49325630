// match.hip -- maximal matching with deterministic mates, everything device-resident: bspgemm_maximal_matching
// (include/bspgemm.h).  No product: the locally-dominant-edge algorithm on the simple undirected graph S =
// bspgemm_matrix_symmetrize(A, DROP_DIAGONAL) (sorted duplicate-free rows, no diagonal, every column in [0, n): the
// transpose inside symmetrize tests them).  An edge {a, b}, a < b, has a 32-bit key (the header gives the formula) and the
// edges are ordered by (key32, a, b).  An edge that is the smallest LIVE edge (both ends free) at both of its ends belongs to
// the greedy matching of that order: nothing that sequential greedy visits earlier touches either end, because every earlier
// edge at either end already has a matched end.  For a fixed u, comparing (key32, a, b) across its neighbours w equals
// comparing (key32, w), so a vertex's candidate is one u64 = key32 << 32 | w, and ~0 means none.  The arrays, all in the
// context's workspace behind one WsCursor:
//     flags        the counter block (MatchFlags)
//     best[n]      the round's candidate of a live vertex
//     mate[n]      -1 = free
//     list[2][n]   two live lists that the rounds ping-pong
//     chunk[cap]   the hub chunk records {vertex, chunk number} of the live list that is read next
//     k_match_init     per vertex: P.row_ptr, mate = -1
//     k_match_seed     per vertex: degree > 0 appends v to list 0; an isolated vertex is never listed
//     k_match_point<W> W lanes per live vertex u, striding over S's row u, kMatchDeep steps in flight: a neighbour w with
//                      mate[w] < 0 gives a candidate, the lanes keep the minimum, a shuffle reduction joins the W lanes
//                      and the finishing lane stores best[u] plainly -- it is the sole owner of that word.  A row longer
//                      than kMatchChunk is not walked: its group stores ~0 and the row's chunk records do the work
//     k_match_hub      one workgroup per chunk record: a block-wide minimum and ONE device-scope 64-bit atomicMin on
//                      best[u], so a hub costs what its entries cost
//     k_match_pair     one thread per live u.  best[u] == ~0: u retires, unmatched for good.  Otherwise w = low32(best[u]);
//                      low32(best[w]) == u: mate[u] = w (each end writes its own word, the end with u < w counts the
//                      pair); else u is appended to the OTHER list -- with its degree added to `walked` and, for a hub,
//                      its chunk records taken by hub_chunks_emit, so that the round's one read-back (8 bytes: the other
//                      list's size and its chunk cursor) tells the host the next round's two grids.  The seed does the
//                      same for list 0.  Both run in workgroups of 1024 whose appends, degrees and pairs go out by one
//                      atomic per counter and workgroup (match_list)
//     k_match_finish   per vertex: P.col_idx[v] = min(v, mate[v]), v itself when free
// Invariants.  A free vertex with a free neighbour is live: a vertex leaves the lists only matched or with NO free
// neighbour, and the free set only shrinks, so a retired vertex stays without free neighbours and every free neighbour w of
// a live u is in the round's list -- best[w] is this round's.  The smallest live edge of all is dominant at both ends, so
// every round with a live edge matches a pair: the list shrinks every round and at most n / 2 + 1 rounds run.  By induction
// along the edge order the pairs are those of sequential greedy: unique, so every run, lane width and hub split gives the
// same bits.  The ORDER inside a list or among the chunk records depends on scheduling and changes nothing: a launch
// consumes all of them, and a minimum does not depend on the order of its operands.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores.  Every decision
// rests on values stored by an EARLIER launch (mate[] by the pair launch of an earlier round, best[] by the point and hub
// launches of this round, the list, the chunk records and their sizes through the host) or on the return value of a
// device-scope atomic (the appends' cursors).  The hub's atomicMin results are read by the NEXT launch only.  No kernel
// waits for another workgroup: every loop is bounded by the thread's own row or chunk, or by the list size the host passed
// in.
//
// Cost.  Three launches at most and one synchronisation (8 bytes read back) per round.  A row is walked AGAIN in every
// round in which its vertex is still live (info.entries_walked is that sum): NATURAL on a path stored in ascending order
// takes n / 2 rounds, RANDOM 3 to 7 on the test graphs.  The host caps the loop at n rounds and never spins.
#include "internal.hpp"
#include "wave.hpp"
#include "hub_chunks.hpp"

namespace bsp {

constexpr int kMatchThreads = 256;
constexpr int kMatchWaves = kMatchThreads / 64;
constexpr int kMatchListThreads = 1024;  // the seed and the pair launch: one atomic per counter and WORKGROUP
constexpr int kMatchChunk = 4096;       // the longest row left to one group of lanes; entries per chunk of a longer one
constexpr int kMatchDeep = 4;           // steps of a row in flight per trip of the walk, as kColDeep
constexpr u64 kMatchNone = ~0ull;

struct MatchFlags {
    int2 next[2];           // {entries, chunk records} appended for list 0 / list 1 by the launch that writes it
    int pairs;              // matched edges so far
    int pad;
    u64 walked;             // the degrees of every vertex ever appended: the entries the point launches walk
};

// key32 << 32 | w of the edge {u, w}; du = deg_S(u).  order: a bspgemm_match_order.
__device__ __forceinline__ u64 match_candidate(int order, u32 seed, int u, int du, int w, const int *__restrict__ rpS)
{
    u32 key = 0;
    if (order != BSPGEMM_MATCH_NATURAL) {
        const u32 a = (u32)min(u, w), b = (u32)max(u, w);
        const u32 h = mix32(mix32(a ^ seed) ^ b);
        if (order == BSPGEMM_MATCH_RANDOM) {
            key = h;
        } else {
            const u32 sum = (u32)du + (u32)(rpS[w + 1] - rpS[w]);
            key = (min(sum, 0xffffu) << 16) | (h >> 16);
        }
    }
    return ((u64)key << 32) | (u32)w;
}

__global__ __launch_bounds__(kMatchThreads) void k_match_init(int n, int *__restrict__ mate, int *__restrict__ row_ptr)
{
    const long long v = (long long)blockIdx.x * kMatchThreads + threadIdx.x;
    if (v <= n) row_ptr[v] = (int)v;
    if (v < n && mate) mate[v] = -1;
}

// What the seed and the pair launch do for the vertices they list (`take`) and the pairs they count (`pair`), in workgroups
// of kMatchListThreads: block_list_append (hub_chunks.hpp), with the pairs as its third sum.  A vertex is listed once per
// round at most, and a listed vertex has a non-empty row.
typedef ListBlock<kMatchListThreads, true> MatchBlock;

__device__ __forceinline__ void match_list(bool take, bool pair, int u, const int *__restrict__ rpS, int n, int *list, MatchFlags *fl,
                                           int nx, int2 *chunk, int chunk_cap, MatchBlock &sh)
{
    block_list_append<kMatchListThreads, kMatchChunk, true>(take, pair, u, rpS, n, list, &fl->next[nx], &fl->walked, &fl->pairs, chunk,
                                                            chunk_cap, sh);
}

__global__ __launch_bounds__(kMatchListThreads) void k_match_seed(int n, const int *__restrict__ rpS, int *__restrict__ list,
                                                                 MatchFlags *fl, int2 *__restrict__ chunk, int chunk_cap)
{
    __shared__ MatchBlock sh;
    const long long v = (long long)blockIdx.x * kMatchListThreads + threadIdx.x;
    const bool take = v < n && rpS[v + 1] > rpS[v];
    match_list(take, false, take ? (int)v : 0, rpS, n, list, fl, 0, chunk, chunk_cap, sh);
}

// W lanes per vertex of `list` (fsize entries, from the host).  mate[] was stored by earlier launches.  `reset`: the size
// pair of the OTHER list, which this round's pair launch appends to; the host has read it already.
template <int W>
__global__ __launch_bounds__(kMatchThreads) void k_match_point(int fsize, const int *__restrict__ list, const int *__restrict__ rpS,
                                                              const int *__restrict__ colS, const int *__restrict__ mate,
                                                              u64 *__restrict__ best, int order, u32 seed, int2 *reset)
{
    // (open code: GroupRow of hub_chunks.hpp tests the row's length in 64 bits, this kernel in 32 -- du is needed as an int
    // anyway -- and the two compile to other code)
    const long long t = (long long)blockIdx.x * kMatchThreads + threadIdx.x;
    const long long f = t / W;
    const int sub = (int)(t % W);
    if (t == 0) *reset = make_int2(0, 0);
    int u = 0, du = 0;
    long long pos = 0, e = 0;
    if (f < fsize) {
        u = list[f];
        const long long b = rpS[u];
        e = rpS[u + 1];
        du = (int)(e - b);
        if (du > kMatchChunk) e = b;                         // (the chunks' row)
        pos = b + sub;
    }
    u64 m = kMatchNone;
    // kMatchDeep steps per trip, stage by stage (columns, then mate[], then the keys), so that a long row pays the two
    // dependent memory latencies once per kMatchDeep * W entries
    for (; pos < e; pos += (long long)W * kMatchDeep) {
        int x[kMatchDeep], mt[kMatchDeep];
        bool in[kMatchDeep];
#pragma unroll
        for (int j = 0; j < kMatchDeep; j++) {
            in[j] = pos + (long long)W * j < e;
            x[j] = in[j] ? colS[pos + (long long)W * j] : 0; // in [0, n): S is symmetrize's output
        }
#pragma unroll
        for (int j = 0; j < kMatchDeep; j++) mt[j] = in[j] ? mate[x[j]] : 0;
#pragma unroll
        for (int j = 0; j < kMatchDeep; j++)
            if (in[j] && mt[j] < 0) m = min(m, match_candidate(order, seed, u, du, x[j], rpS));
    }
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) m = min(m, (u64)__shfl_xor(m, off, 64));
    if (f < fsize && sub == 0) best[u] = m;                  // (a hub: ~0, and its chunks lower it)
}

// one workgroup per chunk record chunk[blockIdx.x]: the chunk's minimum to best[hub] by one atomic
__global__ __launch_bounds__(kMatchThreads) void k_match_hub(const int2 *__restrict__ chunk, const int *__restrict__ rpS,
                                                            const int *__restrict__ colS, const int *__restrict__ mate, u64 *best,
                                                            int order, u32 seed)
{
    __shared__ u64 part[kMatchWaves];
    const int2 rec = chunk[blockIdx.x];
    long long b, e;
    hub_chunk_range<kMatchChunk>(rpS, rec, b, e);
    const int u = rec.x, du = rpS[u + 1] - rpS[u];
    u64 m = kMatchNone;
    for (long long pos = b + threadIdx.x; pos < e; pos += kMatchThreads) {
        const int w = colS[pos];
        if (mate[w] < 0) m = min(m, match_candidate(order, seed, u, du, w, rpS));
    }
    m = block_min<kMatchThreads>(m, part);
    if (threadIdx.x == 0 && m != kMatchNone) atomicMin(&best[u], m);
}

// one thread per vertex of `list`.  best[] is complete: the point and the hub launch were earlier ones.  mate[] is only
// stored here (the thread's own word) and never loaded.  nx: the list that is appended to.
__global__ __launch_bounds__(kMatchListThreads) void k_match_pair(int n, int fsize, const int *__restrict__ list,
                                                             const int *__restrict__ rpS, const u64 *__restrict__ best,
                                                             int *__restrict__ mate, int *__restrict__ next, MatchFlags *fl, int nx,
                                                             int2 *__restrict__ chunk, int chunk_cap)
{
    __shared__ MatchBlock sh;
    const long long t = (long long)blockIdx.x * kMatchListThreads + threadIdx.x;
    const bool live = t < fsize;
    const int u = live ? list[t] : 0;
    const u64 bu = live ? best[u] : kMatchNone;
    bool keep = false, pair = false;
    if (bu != kMatchNone) {
        const int w = (int)(u32)bu;
        if ((unsigned)w < (unsigned)n && (int)(u32)best[w] == u) {   // (best[w] == ~0: its low word is no vertex)
            mate[u] = w;
            pair = u < w;
        } else {
            keep = true;
        }
    }
    match_list(keep, pair, u, rpS, n, next, fl, nx, chunk, chunk_cap, sh);
}

// mate NULL (S has no entries): every vertex is free
__global__ __launch_bounds__(kMatchThreads) void k_match_finish(int n, const int *__restrict__ mate, int *__restrict__ label)
{
    const long long v = (long long)blockIdx.x * kMatchThreads + threadIdx.x;
    if (v >= n) return;
    const int w = mate ? mate[v] : -1;
    label[v] = w >= 0 && w < v ? w : (int)v;
}

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_maximal_matching(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_match_order order,
                                                   unsigned seed, bspgemm_matrix **P, int *mate_host, bspgemm_match_info *info)
{
    static const char who[] = "bspgemm_maximal_matching";
    if (P) *P = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!ctx || !A || !P) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_maximal_matching: NULL argument");
    if (order != BSPGEMM_MATCH_NATURAL && order != BSPGEMM_MATCH_RANDOM && order != BSPGEMM_MATCH_LIGHT_FIRST)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_maximal_matching: unknown order");
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_SQUARE)) return st;
    // BSPGEMM_MATCH_TIMING: host clocks around the stages; every launch is then synchronised, so that the three launches of a
    // round and its read-back are told apart
    StageClock clk(ctx->match_timing, ctx->stream);
    double ms_sym = 0, ms_seed = 0, ms_point = 0, ms_hub = 0, ms_pair = 0, ms_back = 0;
    if (bspgemm_status st = use_device(ctx)) return st;
    const int forced_w = ctx->match_lanes;
    // The workspace grows ONCE per call: to what the symmetrize takes at most over its stages or, if that is more, to the
    // call's own state.  S has at most 2 nnz(A) entries, and a row longer than the chunk size has fewer than 2 len / chunk
    // chunks, so all hubs together have fewer than 4 nnz(A) / chunk records; the capacity is set again from nnz(S) below.
    const size_t n4 = ws_pad4((size_t)A->rows);
    MatchFlags *d_flags = nullptr;
    u64 *best = nullptr;
    int *mate = nullptr, *list[2] = {nullptr, nullptr};
    int2 *chunk = nullptr;
    auto chunk_cap_of = [](long long E) { return (size_t)(2 * E / kMatchChunk + 1); };
    auto carve = [&](int *tmp, size_t chunk_cap) {
        return WsCursor(tmp).take(d_flags, 1).take(best, n4).take(mate, n4).take(list[0], n4).take(list[1], n4).take(chunk, chunk_cap).ints();
    };
    const size_t upper_ints = carve(nullptr, chunk_cap_of(2 * (long long)A->nnz));
    bspgemm_matrix *S = nullptr;
    if (bspgemm_status st = symmetrized_operand(ctx, A, upper_ints, A->nnz > 0, clk, ms_sym, &S)) return st;
    hipStream_t s = ctx->stream;
    const int n = S->rows;
    const long long E = S->nnz;                             // <= INT_MAX: symmetrize refuses more
    const bool edges = E > 0;
    bspgemm_matrix *m = nullptr;                            // the assignment operand
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_matrix_free(m);
        bspgemm_matrix_free(S);
        return st;
    };
    const size_t chunk_cap = chunk_cap_of(E);
    if (edges) {
        if (bspgemm_status st = ensure_tmp(ctx, carve(nullptr, chunk_cap))) return bail(st);   // (there already, see above)
        carve(ctx->tmp, chunk_cap);
    }
    if (bspgemm_status st = assignment_operand(ctx, n, &m)) return bail(st);
    const dim3 vgrid = vertex_grid(n, kMatchThreads), block(kMatchThreads);
    clk.start();
    hipLaunchKernelGGL(k_match_init, vgrid, block, 0, s, n, mate, m->d_row_ptr);
    HIPCHK_B(hipGetLastError());
    int rounds = 0, W = 0;
    long long hub_chunks = 0;
    MatchFlags h_flags;
    memset(&h_flags, 0, sizeof h_flags);
    if (edges) {
        HIPCHK_B(round_reset(d_flags, sizeof(MatchFlags), s));
        hipLaunchKernelGGL(k_match_seed, grid_for(n, kMatchListThreads), dim3(kMatchListThreads), 0, s, n, S->d_row_ptr, list[0], d_flags, chunk, (int)chunk_cap);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(clk.lap(ms_seed, true));
        int2 head = make_int2(0, 0);                        // {entries, chunk records} of the list that is read next
        int cur = 0;
        HIPCHK_B(hipMemcpyAsync(&head, &d_flags->next[0], sizeof head, hipMemcpyDeviceToHost, s));
        HIPCHK_B(hipStreamSynchronize(s));
        HIPCHK_B(clk.lap(ms_back));
        if (!frontier_head_ok(head, 2, n, chunk_cap)) return bail(fail_stuck(who));   // an edge has two ends
        // the lanes per live vertex of the call: a QUARTER of the mean degree of the listed vertices, the rule of
        // betweenness.hip -- no group walks more than kMatchChunk entries, so a hub is no serial tail
        W = forced_w ? forced_w : lanes_for_mean(E, head.x, 4);
        while (head.x > 0) {
            if (rounds >= n) return bail(fail_stuck(who));
            rounds++;
            hub_chunks += head.y;
            const int fsize = head.x;
            double ms_round = 0;
            clk.start();
            dispatch_lanes(W, [&](auto w) {
                hipLaunchKernelGGL(k_match_point<decltype(w)::value>, grid_for((long long)fsize * W, kMatchThreads), block, 0, s, fsize, list[cur],
                                   S->d_row_ptr, S->d_col_idx, mate, best, (int)order, (u32)seed, &d_flags->next[cur ^ 1]);
            });
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_point, true));
            ms_round += clk.last;
            if (head.y > 0) {
                hipLaunchKernelGGL(k_match_hub, dim3((unsigned)head.y), block, 0, s, chunk, S->d_row_ptr, S->d_col_idx, mate, best,
                                   (int)order, (u32)seed);
                HIPCHK_B(hipGetLastError());
                HIPCHK_B(clk.lap(ms_hub, true));
                ms_round += clk.last;
            }
            hipLaunchKernelGGL(k_match_pair, grid_for(fsize, kMatchListThreads), dim3(kMatchListThreads), 0, s, n, fsize, list[cur], S->d_row_ptr, best, mate,
                               list[cur ^ 1], d_flags, cur ^ 1, chunk, (int)chunk_cap);
            HIPCHK_B(hipGetLastError());
            HIPCHK_B(clk.lap(ms_pair, true));
            clk.longest(ms_round + clk.last, rounds, fsize);
            HIPCHK_B(hipMemcpyAsync(&head, &d_flags->next[cur ^ 1], sizeof head, hipMemcpyDeviceToHost, s));
            HIPCHK_B(hipStreamSynchronize(s));              // the round's one synchronisation
            HIPCHK_B(clk.lap(ms_back));
            // the smallest live edge of the round was matched, or nobody had a candidate: the list shrinks
            if (!frontier_head_ok(head, 0, fsize - 1, chunk_cap)) return bail(fail_stuck(who));
            cur ^= 1;
        }
        HIPCHK_B(hipMemcpyAsync(&h_flags, d_flags, sizeof h_flags, hipMemcpyDeviceToHost, s));
    }
    hipLaunchKernelGGL(k_match_finish, vgrid, block, 0, s, n, mate, m->d_col_idx);
    HIPCHK_B(hipGetLastError());
    if (mate_host && n > 0) {
        if (edges) HIPCHK_B(hipMemcpyAsync(mate_host, mate, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        else std::fill(mate_host, mate_host + n, -1);
    }
    if (bspgemm_status st = operand_finish(m, n)) return bail(st);   // one label per vertex
    HIPCHK_B(hipStreamSynchronize(s));
    if (h_flags.pairs < 0 || 2ll * h_flags.pairs > n || (edges && h_flags.pairs == 0)) return bail(fail_stuck(who));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: n %d nnz(S) %lld order %d pairs %d entries walked %llu hub chunks %lld (%d lanes) | total %.3f ms "
                        "= symmetrize %.3f + seed %.3f + %d point launches %.3f + hub launches %.3f + pair launches %.3f + read-backs "
                        "%.3f + rest | longest round %.3f ms (round %d, %d live vertices)\n",
                who, n, E, (int)order, h_flags.pairs, h_flags.walked, hub_chunks, W, clk.total(), ms_sym, ms_seed, rounds, ms_point,
                ms_hub, ms_pair, ms_back, clk.max_ms, clk.max_tag[0], clk.max_tag[1]);
    bspgemm_matrix_free(S);
    if (info) {
        info->pairs = h_flags.pairs;
        info->entries_walked = (int64_t)h_flags.walked;
        info->hub_chunks = hub_chunks;
        info->rounds = rounds;
        info->lanes = W;
    }
    *P = m;
    return BSPGEMM_OK;
}
