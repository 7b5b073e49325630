// lp.hip -- community detection by synchronous label propagation (CDLP as LDBC Graphalytics defines it), everything
// device-resident: bspgemm_label_propagation (include/bspgemm.h).  No product.  On the simple undirected graph S =
// bspgemm_matrix_symmetrize(A, DROP_DIAGONAL) (sorted duplicate-free rows, no diagonal, every column in [0, n): the
// transpose inside symmetrize tests them) every iteration gives every vertex v with a non-empty row the MODE of the multiset
// { label(w) : w in S_v } of the labels of the iteration before: the most frequent one, ties to the smallest.  The arrays:
//     label[2][n]  the labels the iteration reads and the ones it writes; [0] is the col_idx of the assignment operand P
//                  that the call returns, [1] is in the workspace; the iterations ping-pong
//     list[4][n]   the vertices of each degree class, built once per call (S does not change)          (workspace)
//     tab_of[n]    64-bit: where a hub's table starts in `tabs`, counted in slots; -1 for everybody else (workspace)
//     tabs         per hub an open-addressing table of 2 d slots {label + 1, count}, 0 = empty    (the values workspace)
// and a block of eight counters and the kLpShards words of the `changed` counter.
//     k_lp_init      per vertex: P.row_ptr, label[1] = label[0] (= v, or the caller's labels, copied in before)
//     k_lp_classify  per vertex of degree d >= 1: class = max(own, BSPGEMM_OPT_LP_MIN_CLASS), own = 0 for d <= kLpLaneCap,
//                    1 for d <= kLpWaveCap, 2 for d <= kLpGroupCap, else 3; appended to its class list (ballot, one atomicAdd
//                    per wave and class, lane rank by mbcnt); a hub takes its 2 d slots from a 64-bit cursor by atomicAdd
//     k_lp_lane      one lane per vertex of list 0: the row's labels in registers, d * d compares
//     k_lp_wave      one wave per vertex of list 1: the labels gathered into the wave's LDS segment, sorted there (bitonic
//                    over the next power of two, padded with INT_MAX, which is no label), every element that ends a run of
//                    equal labels finds the run's start by a binary search, (count, label) reduced across the wave
//     k_lp_group     one workgroup per vertex of list 2: the same at workgroup scope
//     k_lp_hub_walk  per stored entry (v, w) of S, in select's geometry (sel_rows.hpp: a workgroup owns kSelTile consecutive
//                    entries whatever rows they belong to -- a hub row costs what its entries cost): for a hub v the label
//                    of w is inserted into v's table: the slot is claimed by a device-scope atomicCAS on its key word (0 ->
//                    label + 1) and counted by an atomicAdd on its count word; a lane joins consecutive entries of one
//                    row with one label into one insert
//     k_lp_hub_mode  a SECOND launch, one workgroup per hub: the argmax over its table
//     k_lp_mark      at the end, per vertex: the first atomicExch on mark[label(v)] counts one community
// All four classes compute the same function and write label_out[v]; a vertex whose label differs from label_in[v] adds
// to the `changed` counter (ballot, one atomic per wave, on the word the workgroup's number picks: lp_shard).  One read-back
// of that counter per iteration, which the host sums, is the loop's only
// synchronisation; an iteration that changes nothing is a fixpoint and ends the loop.
//
// Invariants.  label_in is only read in a launch and was written by an EARLIER launch (the init, or the iteration before:
// launches of one stream run in order); label_out is another array, and label_out[v] is written by v's owner only: the
// lane, wave or workgroup that the class list gives v to, once per list, and a vertex is in exactly one list.  A vertex
// of degree 0 is in no list: both arrays hold its first label from the init on.  So every vertex reads the labels of the
// iteration before and nothing else: the propagation is synchronous, counts are integers, the argmax with the smallest-
// label tie is unique, and every run gives the same bits whatever the scheduling.  The ORDER inside a list, and where in
// `tabs` a hub's table lies, depend on scheduling and change nothing.
//
// The hub tables.  Touched by atomics only while the walk runs, cleared by a memset on the stream before it, and read
// plainly only by k_lp_hub_mode, a later launch.  The key word holds label + 1 (at most INT_MAX, n being an int), so the
// empty slot 0 cannot collide with label 0.  A table has 2 d slots and receives at most d inserts of at most d distinct labels:
// it never fills, a probe sequence meets an empty slot or its own key after fewer than 2 d steps, it starts at
// (mix32(label) * size) >> 32 < size, wraps to slot 0 of ITS OWN table at `size` and is bounded by `size` steps all the
// same.  The return value of the atomicCAS decides: 0 (claimed now) or label + 1 (claimed by somebody else for the same
// label) counts here, anything else moves on; a key never changes once it is set.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores.  Nothing here reads
// plainly what the same launch writes: labels and tables cross launches only, and within a launch only return values of
// device-scope atomics are used (the list cursors, the table keys).  No kernel waits for another workgroup: every loop is
// bounded by the thread's own row, by its table's size or by the list size the host passed in.
//
// Cost (DESIGN.md 4.19 has the figures).  An iteration reads every entry of S once through its row's owner (col_idx, then
// the gathered label) and, when there is a hub, once more in the walk, which streams ALL of S.col_idx to reach the hubs'
// entries.  The lane class is bound by its gather; the wave and workgroup classes by the sort (log2(N)^2 / 2 passes over
// LDS, with a barrier each in the workgroup); the hubs by their atomics: where the labels have settled, most of a hub's
// inserts meet in one or two slots, and atomics on one address run one after the other -- the lane's runs take a factor
// of up to 16 off that, a join across the wave's lanes would take more and is not done.  k_lp_hub_mode gives one workgroup
// to a table: a hub of degree d is a serial tail of 2 d / 256 steps there.  Synchronous propagation oscillates with period
// 2 on bipartite components: max_iter is what ends it, nothing here detects the cycle.
#include "internal.hpp"
#include "sel_rows.hpp"

namespace bsp {

constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / 64;
constexpr int kLpLaneCap = 8;           // the longest row one lane takes (registers, d * d compares)
constexpr int kLpWaveCap = 256;         // the longest row one wave sorts in its LDS segment: four labels per lane
constexpr int kLpGroupCap = 4096;       // the longest row one workgroup sorts: 16 KiB of LDS, so that occupancy stays with the
                                        // 32-waves-per-CU cap and not with LDS
constexpr int kLpClasses = 4;
constexpr int kLpShards = 64;           // words of the `changed` counter, each on a line of its own
constexpr int kLpShardStride = 32;
constexpr int kLpPad = INT_MAX;         // pads a sort buffer; a label is below n <= INT_MAX

struct LpFlags {
    int size[kLpClasses];   // vertices of the class lists
    int pad;
    int communities;        // distinct labels (k_lp_mark)
    u64 slots;              // table slots handed out to the hubs
};

// (count, label) as one word that orders by the larger count, then by the SMALLER label
__device__ __forceinline__ u64 lp_pack(int count, int label) { return ((u64)(u32)count << 32) | (u32)~(u32)label; }
__device__ __forceinline__ int lp_label(u64 best) { return (int)~(u32)best; }

// The `changed` counter is kLpShards words, kLpShardStride ints apart (a 128-byte line each); a workgroup adds to the one
// its number picks and the host sums them.  On a graph whose labels all move, one word would take an atomic from every
// wave of k_lp_wave, and atomics on one address run one after the other (10 ns each, 6.8 ms an iteration).
__device__ __forceinline__ int *lp_shard(int *changed) { return changed + kLpShardStride * (blockIdx.x & (kLpShards - 1)); }

// label0 holds the first labels already when `given`
__global__ __launch_bounds__(kLpThreads) void k_lp_init(int n, bool given, int *__restrict__ label0, int *__restrict__ label1,
                                                       int *__restrict__ row_ptr)
{
    const long long v = (long long)blockIdx.x * kLpThreads + threadIdx.x;
    if (v <= n) row_ptr[v] = (int)v;
    if (v < n) {
        const int l = given ? label0[v] : (int)v;
        if (!given) label0[v] = l;
        if (label1) label1[v] = l;
    }
}

__device__ __forceinline__ int lp_class_of(int d)
{
    return d <= kLpLaneCap ? 0 : d <= kLpWaveCap ? 1 : d <= kLpGroupCap ? 2 : 3;
}

// list: kLpClasses lists, `stride` ints apart
__global__ __launch_bounds__(kLpThreads) void k_lp_classify(int n, int min_class, const int *__restrict__ rpS,
                                                           int *__restrict__ list, size_t stride,
                                                           long long *__restrict__ tab_of, LpFlags *flags)
{
    const int lane = lane_id();
    const long long v = (long long)blockIdx.x * kLpThreads + threadIdx.x;
    int cls = -1;
    if (v < n) {
        const int d = rpS[v + 1] - rpS[v];
        if (d > 0) cls = max(lp_class_of(d), min_class);
        tab_of[v] = cls == 3 ? (long long)atomicAdd(&flags->slots, 2ull * (u64)d) : -1;
    }
#pragma unroll
    for (int c = 0; c < kLpClasses; c++) wave_append(cls == c, (int)v, list + c * stride, &flags->size[c], n, lane);
}

// ---------------------------------------------------------------- class 0: one lane per vertex -------------------------
__global__ __launch_bounds__(kLpThreads) void k_lp_lane(int count, const int *__restrict__ list, const int *__restrict__ rpS,
                                                       const int *__restrict__ colS, const int *__restrict__ label_in,
                                                       int *__restrict__ label_out, int *changed)
{
    const long long i = (long long)blockIdx.x * kLpThreads + threadIdx.x;
    bool moved = false;
    if (i < count) {
        const int v = list[i];
        const long long b = rpS[v];
        const int d = min(rpS[v + 1] - (int)b, kLpLaneCap);  // (the list holds rows of at most kLpLaneCap entries)
        int x[kLpLaneCap];
#pragma unroll
        for (int j = 0; j < kLpLaneCap; j++) x[j] = j < d ? colS[b + j] : 0;   // in [0, n): S is symmetrize's output
#pragma unroll
        for (int j = 0; j < kLpLaneCap; j++) x[j] = j < d ? label_in[x[j]] : -1 - j;   // (pads equal nothing)
        u64 best = 0;
#pragma unroll
        for (int j = 0; j < kLpLaneCap; j++) {
            int c = 0;
#pragma unroll
            for (int k = 0; k < kLpLaneCap; k++) c += x[k] == x[j] ? 1 : 0;
            const u64 key = lp_pack(c, x[j]);
            if (j < d && key > best) best = key;
        }
        if (d > 0) {
            const int l = lp_label(best);
            moved = l != label_in[v];
            label_out[v] = l;
        }
    }
    wave_count(moved, lp_shard(changed), lane_id());
}

// ---------------------------------------------------------------- classes 1 and 2: sort in LDS -------------------------
// The mode of buf[0 .. d) by THREADS threads (t: this thread's index among them) that share buf and nothing else: a wave
// (THREADS == 64, ordered by wave_lds_fence) or the whole workgroup (ordered by the barrier).  buf holds N >= d ints, N a
// power of two >= 2, buf[d .. N) = kLpPad.  Returns this thread's best (count, label); the caller joins the threads.
template <int THREADS>
__device__ __forceinline__ void lp_sync()
{
    if (THREADS == 64) wave_lds_fence();
    else __syncthreads();
}

template <int THREADS>
__device__ __forceinline__ u64 lp_sorted_mode(int *buf, int d, int N, int t)
{
    lp_sync<THREADS>();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < (N >> 1); p += THREADS) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));   // < N - j
                const int hi = lo | j;                                  // < N
                const int a = buf[lo], b = buf[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    buf[lo] = b;
                    buf[hi] = a;
                }
            }
            lp_sync<THREADS>();
        }
    }
    // ascending now, the pads last.  The element that ends a run knows the run's length once it has the run's start
    u64 best = 0;
    for (int i = t; i < d; i += THREADS) {
        const int x = buf[i];
        if (i + 1 < d && buf[i + 1] == x) continue;
        const int first = sel_lower_bound(buf, 0, i, x);
        const u64 key = lp_pack(i - first + 1, x);
        if (key > best) best = key;
    }
    return best;
}

__device__ __forceinline__ int lp_pow2_at_least(int d)      // 2 <= result, d <= result, d >= 1
{
    return d <= 2 ? 2 : 1 << (32 - __clz(d - 1));
}

__global__ __launch_bounds__(kLpThreads) void k_lp_wave(int count, const int *__restrict__ list, const int *__restrict__ rpS,
                                                       const int *__restrict__ colS, const int *__restrict__ label_in,
                                                       int *__restrict__ label_out, int *changed)
{
    __shared__ int seg[kLpWaves][kLpWaveCap];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kLpWaves + w;
    if (i >= count) return;                                  // (wave-uniform)
    const int v = list[i];
    const long long b = rpS[v];
    const int d = min(rpS[v + 1] - (int)b, kLpWaveCap);      // (the list holds rows of 1 .. kLpWaveCap entries)
    const int N = lp_pow2_at_least(d);                       // <= kLpWaveCap, a power of two itself
    int *buf = seg[w];
    // stage by stage (columns, then labels), so that the row pays the two dependent memory latencies once
    int x[kLpWaveCap / 64];
#pragma unroll
    for (int j = 0; j < kLpWaveCap / 64; j++) x[j] = 64 * j + lane < d ? colS[b + 64 * j + lane] : 0;   // in [0, n)
#pragma unroll
    for (int j = 0; j < kLpWaveCap / 64; j++) x[j] = 64 * j + lane < d ? label_in[x[j]] : kLpPad;
#pragma unroll
    for (int j = 0; j < kLpWaveCap / 64; j++)
        if (64 * j + lane < N) buf[64 * j + lane] = x[j];
    const u64 best = wave_max(lp_sorted_mode<64>(buf, d, N, lane));
    const int l = lp_label(best);
    const bool moved = lane == 0 && l != label_in[v];
    if (lane == 0) label_out[v] = l;
    wave_count(moved, lp_shard(changed), lane);
}

__global__ __launch_bounds__(kLpThreads) void k_lp_group(int count, const int *__restrict__ list, const int *__restrict__ rpS,
                                                        const int *__restrict__ colS, const int *__restrict__ label_in,
                                                        int *__restrict__ label_out, int *changed)
{
    __shared__ int buf[kLpGroupCap];
    __shared__ u64 wbest[kLpWaves];
    const int t = threadIdx.x;
    const int v = list[blockIdx.x];                          // the grid is `count` workgroups
    const long long b = rpS[v];
    const int d = min(rpS[v + 1] - (int)b, kLpGroupCap);     // (the list holds rows of 1 .. kLpGroupCap entries)
    const int N = lp_pow2_at_least(d);
#pragma unroll 4
    for (int q = t; q < N; q += kLpThreads) buf[q] = q < d ? label_in[colS[b + q]] : kLpPad;
    const u64 best = wave_max(lp_sorted_mode<kLpThreads>(buf, d, N, t));
    if (lane_id() == 0) wbest[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        u64 top = wbest[0];
#pragma unroll
        for (int q = 1; q < kLpWaves; q++) top = wbest[q] > top ? wbest[q] : top;
        const int l = lp_label(top);
        if (l != label_in[v]) atomicAdd(lp_shard(changed), 1);
        label_out[v] = l;
    }
}

// ---------------------------------------------------------------- class 3: the hubs ------------------------------------
// The insert as an op of sel_walk_entries.  tabs: 2 ints per slot, {label + 1 or 0, count}.  A lane joins the entries it
// walks one after the other that carry the same label into the same table and inserts the run by one pair of atomics when the
// label or the row changes (and at the end: flush()): where the labels have settled, a hub's neighbours mostly agree, and
// its one counter would otherwise take an atomic per entry, one after the other.
struct LpHubInsert {
    const int *__restrict__ rpS;
    const long long *__restrict__ tab_of;
    const int *__restrict__ label_in;
    int *tabs;
    int *tab;               // the table of the lane's row; NULL: not a hub
    u32 size;
    int cur;                // the lane's row (-1: none yet)
    int key, run;           // the pending run: label + 1 and its length (0: none)
    __device__ __forceinline__ void flush()
    {
        if (run == 0) return;
        u32 at = (u32)(((u64)mix32((u32)(key - 1)) * size) >> 32);   // < size
        for (u32 probe = 0; probe < size; probe++) {
            const int old = atomicCAS(&tab[2 * (size_t)at], 0, key);
            if (old == 0 || old == key) {
                atomicAdd(&tab[2 * (size_t)at + 1], run);
                break;
            }
            if (++at == size) at = 0;                        // wraps inside its own table
        }
        run = 0;
    }
    __device__ __forceinline__ void load(int, long long) {}
    __device__ __forceinline__ void row(int r)
    {
        if (r == cur) return;                                // (the walk enters the row again at every step)
        flush();                                             // (into the table of the row it was walked in)
        cur = r;
        const long long off = tab_of[r];
        tab = off >= 0 ? tabs + 2 * off : nullptr;
        size = 2u * (u32)(rpS[r + 1] - rpS[r]);
    }
    __device__ __forceinline__ void entry(int, long long, int w, int)
    {
        if (!tab) return;
        const int k = label_in[w] + 1;                       // w in [0, n): S is symmetrize's output
        if (run && k != key) flush();
        key = k;
        run++;
    }
};

__global__ __launch_bounds__(kSelThreads) void k_lp_hub_walk(const int *__restrict__ rpS, const int *__restrict__ colS, int n,
                                                            long long E, bool vec, const int *__restrict__ tile_row,
                                                            const long long *__restrict__ tab_of,
                                                            const int *__restrict__ label_in, int *tabs)
{
    LpHubInsert op = {rpS, tab_of, label_in, tabs, nullptr, 0u, -1, 0, 0};
    sel_walk_entries<false>(rpS, colS, n, E, vec, tile_row, op);
    op.flush();
}

// one workgroup per hub of `list` (the grid is its size); the tables are complete: the walk was an earlier launch
__global__ __launch_bounds__(kLpThreads) void k_lp_hub_mode(const int *__restrict__ list, const int *__restrict__ rpS,
                                                           const long long *__restrict__ tab_of, const int *__restrict__ tabs,
                                                           const int *__restrict__ label_in, int *__restrict__ label_out,
                                                           int *changed)
{
    __shared__ u64 wbest[kLpWaves];
    const int t = threadIdx.x;
    const int v = list[blockIdx.x];
    const long long off = tab_of[v];
    const u32 size = off >= 0 ? 2u * (u32)(rpS[v + 1] - rpS[v]) : 0u;   // (off < 0 cannot be: the list holds hubs)
    const int2 *tab = reinterpret_cast<const int2 *>(tabs) + (off >= 0 ? off : 0);
    u64 best = 0;
    for (u32 q = t; q < size; q += kLpThreads) {
        const int2 slot = tab[q];
        if (slot.x) {
            const u64 key = lp_pack(slot.y, slot.x - 1);
            if (key > best) best = key;
        }
    }
    best = wave_max(best);
    if (lane_id() == 0) wbest[t >> 6] = best;
    __syncthreads();
    if (t == 0 && size) {
        u64 top = wbest[0];
#pragma unroll
        for (int q = 1; q < kLpWaves; q++) top = wbest[q] > top ? wbest[q] : top;
        const int l = lp_label(top);
        if (l != label_in[v]) atomicAdd(lp_shard(changed), 1);
        label_out[v] = l;
    }
}

// mark: n zeroed ints.  The plain load only spares atomics: the return value of the exchange decides who counts a label.
__global__ __launch_bounds__(kLpThreads) void k_lp_mark(int n, const int *__restrict__ label, int *mark, int *communities)
{
    const long long v = (long long)blockIdx.x * kLpThreads + threadIdx.x;
    bool first = false;
    if (v < n) {
        const unsigned l = (unsigned)label[v];
        if (l < (unsigned)n && mark[l] == 0) first = atomicExch(&mark[l], 1) == 0;
    }
    wave_count(first, communities, lane_id());
}

}  // namespace bsp

using namespace bsp;

extern "C" bspgemm_status bspgemm_label_propagation(bspgemm_context *ctx, const bspgemm_matrix *A, const int *initial_labels,
                                                    int max_iter, bspgemm_matrix **P, bspgemm_lp_info *info)
{
    static const char who[] = "bspgemm_label_propagation";
    if (P) *P = nullptr;
    if (info) *info = bspgemm_lp_info{};
    if (!ctx || !A || !P) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_label_propagation: NULL argument");
    if (max_iter < 0) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_label_propagation: max_iter < 0");
    if (bspgemm_status st = check_operand(ctx, A, who, NEED_SQUARE)) return st;
    const int n = A->rows;
    if (initial_labels)                                     // on the host, before anything is launched
        for (int v = 0; v < n; v++)
            if ((unsigned)initial_labels[v] >= (unsigned)n) {
                snprintf(g_err, sizeof g_err, "%s: initial_labels[%d] = %d is outside [0, %d)", who, v, initial_labels[v], n);
                return BSPGEMM_ERR_INVALID;
            }
    // BSPGEMM_LP_TIMING: host clocks around the stages; every class's launch is then synchronised, and so the iteration
    // before its read-back is issued, so that they are told apart
    StageClock clk(ctx->lp_timing, ctx->stream);
    double ms_sym = 0, ms_lists = 0, ms_launch = 0, ms_back = 0, ms_class[kLpClasses] = {};
    if (bspgemm_status st = use_device(ctx)) return st;
    // The workspace grows ONCE here: to what the symmetrize takes at most over its stages or, if that is more, to the
    // call's own state (the counters, tab_of, the second label array, the four lists and the words of `changed`).  The hubs' tables live in the
    // values workspace, whose size is known only after the lists are: growing it leaves this one where it is.
    const size_t n4 = ws_pad4((size_t)n);
    const size_t shard_ints = (size_t)kLpShards * kLpShardStride;
    LpFlags *d_flags = nullptr;
    long long *tab_of = nullptr;
    int *label[2] = {nullptr, nullptr}, *list = nullptr, *d_changed = nullptr;
    auto carve = [&](int *tmp) {
        return WsCursor(tmp).take(d_flags, 1).take(tab_of, n4).take(label[1], n4).take(list, kLpClasses * n4).take(d_changed, shard_ints).ints();
    };
    const size_t own_ints = n > 0 ? carve(nullptr) : 0;
    bspgemm_matrix *S = nullptr;
    if (bspgemm_status st = symmetrized_operand(ctx, A, own_ints, true, clk, ms_sym, &S)) return st;   // (own_ints whatever nnz(A) is)
    hipStream_t s = ctx->stream;
    const long long E = S->nnz;                             // <= INT_MAX: symmetrize refuses more
    const bool edges = E > 0;
    bspgemm_matrix *m = nullptr;                            // the assignment operand: its col_idx is label[0]
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_matrix_free(m);
        bspgemm_matrix_free(S);
        return st;
    };
    if (edges)
        if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)E)) return bail(st);
    if (bspgemm_status st = ensure_tmp(ctx, own_ints)) return bail(st);   // (there already, see above)
    if (bspgemm_status st = assignment_operand(ctx, n, &m)) return bail(st);
    label[0] = m->d_col_idx;
    if (n > 0) carve(ctx->tmp);
    const dim3 vgrid = vertex_grid(n, kLpThreads), block(kLpThreads);
    LpFlags h = {};
    if (n > 0) HIPCHK_B(round_reset(d_flags, sizeof(LpFlags), s));
    if (initial_labels && n > 0)
        HIPCHK_B(hipMemcpyAsync(label[0], initial_labels, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lp_init, vgrid, block, 0, s, n, initial_labels != nullptr, label[0], edges ? label[1] : nullptr,
                       m->d_row_ptr);
    HIPCHK_B(hipGetLastError());
    int iterations = 0, converged = edges ? 0 : 1, changed = 0;
    size_t tab_ints = 0;
    if (edges) {
        clk.start();
        hipLaunchKernelGGL(k_lp_classify, vgrid, block, 0, s, n, ctx->lp_min_class, S->d_row_ptr, list, n4, tab_of, d_flags);
        HIPCHK_B(round_fetch(&h, d_flags, sizeof h, s));
        long long listed = 0;
        for (int c = 0; c < kLpClasses; c++) {
            if (h.size[c] < 0 || h.size[c] > n) return bail(fail_stuck(who));
            listed += h.size[c];
        }
        // a hub's table has 2 d slots and the hubs' rows are disjoint parts of S
        if (listed > n || h.slots > 2ull * (u64)E || (h.slots == 0) != (h.size[3] == 0)) return bail(fail_stuck(who));
        tab_ints = 2 * (size_t)h.slots;
        if (bspgemm_status st = ensure_tmpv(ctx, tab_ints)) return bail(st);   // sized and carved before any iteration
        if (h.size[3]) launch_select_tile_rows(S->d_row_ptr, n, ctx->tile_row, s);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(clk.lap(ms_lists, true));
        int h_changed[kLpShards * kLpShardStride];          // 8 KiB: the counter's words and the gaps between them
        while (iterations < max_iter) {
            const int *in = label[iterations & 1];
            int *out = label[(iterations & 1) ^ 1];
            iterations++;
            // under BSPGEMM_LP_TIMING: a synchronisation behind every class, so that their times are told apart
            StageClock cls(clk.on, s);
            clk.start();
            HIPCHK_B(hipMemsetAsync(d_changed, 0, shard_ints * sizeof(int), s));
            if (h.size[0]) {
                hipLaunchKernelGGL(k_lp_lane, dim3((unsigned)(((long long)h.size[0] + kLpThreads - 1) / kLpThreads)), block, 0, s,
                                   h.size[0], list, S->d_row_ptr, S->d_col_idx, in, out, d_changed);
                HIPCHK_B(cls.lap(ms_class[0], true));
            }
            if (h.size[1]) {
                hipLaunchKernelGGL(k_lp_wave, dim3((unsigned)(((long long)h.size[1] + kLpWaves - 1) / kLpWaves)), block, 0, s,
                                   h.size[1], list + n4, S->d_row_ptr, S->d_col_idx, in, out, d_changed);
                HIPCHK_B(cls.lap(ms_class[1], true));
            }
            if (h.size[2]) {
                hipLaunchKernelGGL(k_lp_group, dim3((unsigned)h.size[2]), block, 0, s, h.size[2], list + 2 * n4, S->d_row_ptr,
                                   S->d_col_idx, in, out, d_changed);
                HIPCHK_B(cls.lap(ms_class[2], true));
            }
            if (h.size[3]) {
                HIPCHK_B(hipMemsetAsync(ctx->tmpv, 0, tab_ints * sizeof(int), s));
                hipLaunchKernelGGL(k_lp_hub_walk, dim3(select_tiles(E)), dim3(kSelThreads), 0, s, S->d_row_ptr, S->d_col_idx, n, E,
                                   aligned16(S->d_col_idx), ctx->tile_row, tab_of, in, ctx->tmpv);
                hipLaunchKernelGGL(k_lp_hub_mode, dim3((unsigned)h.size[3]), block, 0, s, list + 3 * n4, S->d_row_ptr, tab_of,
                                   ctx->tmpv, in, out, d_changed);
                HIPCHK_B(cls.lap(ms_class[3], true));
            }
            HIPCHK_B(hipGetLastError());
            (void)clk.lap(ms_launch);
            clk.longest(clk.last, iterations);
            HIPCHK_B(hipMemcpyAsync(h_changed, d_changed, sizeof h_changed, hipMemcpyDeviceToHost, s));
            HIPCHK_B(hipStreamSynchronize(s));              // the iteration's one synchronisation
            HIPCHK_B(clk.lap(ms_back));
            long long moved = 0;
            for (int q = 0; q < kLpShards; q++) moved += h_changed[q * kLpShardStride];
            if (moved < 0 || moved > n) return bail(fail_stuck(who));
            changed = (int)moved;
            if (changed == 0) {                             // a fixpoint: both arrays hold it
                converged = 1;
                break;
            }
        }
        // the last iteration wrote label[iterations & 1]; one that changed nothing wrote what label[0] holds already
        if (!converged && (iterations & 1))
            HIPCHK_B(hipMemcpyAsync(label[0], label[1], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    if (n > 0) {                                            // the lists are done with: list 0 is the mark array
        HIPCHK_B(hipMemsetAsync(list, 0, (size_t)n * sizeof(int), s));
        hipLaunchKernelGGL(k_lp_mark, vgrid, block, 0, s, n, label[0], list, &d_flags->communities);
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(hipMemcpyAsync(&h.communities, &d_flags->communities, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    if (bspgemm_status st = operand_finish(m, n)) return bail(st);   // one label per vertex
    HIPCHK_B(hipStreamSynchronize(s));
    if (h.communities < (n > 0 ? 1 : 0) || h.communities > n) return bail(fail_stuck(who));
    if (clk.on)
        fprintf(stderr, "[bspgemm] %s: n %d nnz(S) %lld classes %d/%d/%d/%d table slots %llu communities %d | total %.3f ms = "
                        "symmetrize %.3f + class lists %.3f + %d iterations %.3f (lane %.3f, wave %.3f, workgroup %.3f, hub %.3f) + "
                        "read-backs %.3f + rest | longest iteration %.3f ms (iteration %d)\n",
                who, n, E, h.size[0], h.size[1], h.size[2], h.size[3], (unsigned long long)h.slots, h.communities,
                clk.total(), ms_sym, ms_lists, iterations, ms_launch, ms_class[0], ms_class[1], ms_class[2], ms_class[3], ms_back,
                clk.max_ms, clk.max_tag[0]);
    bspgemm_matrix_free(S);
    if (info) {
        info->iterations = iterations;
        info->converged = converged;
        info->communities = h.communities;
        info->changed = changed;
        for (int c = 0; c < kLpClasses; c++) info->class_vertices[c] = h.size[c];
    }
    *P = m;
    return BSPGEMM_OK;
}
