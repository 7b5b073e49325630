// bfs_tree.hip -- single-source direction-optimising breadth-first search that returns the BFS tree, everything
// device-resident: bspgemm_bfs_tree (include/bspgemm.h).  No product: level-synchronous steps on four arrays of the
// context's workspace
//     level[n]    -1 = unreached                       parent[n]   INT_MAX = none yet
//     list[2][n]  two frontier lists that the launches ping-pong
// and a block of counters {next frontier size, error bits, the next frontier's out-degree sum} per list.  Level d = 1, 2, ...
// is produced from the frontier, the vertices of level d - 1, by ONE launch of either kind and one read-back of the block:
//     k_bfs_push<W>   W lanes per frontier vertex u, striding over A's row u.  A neighbour v outside [0, n) sets an error
//                     bit.  level[v] in [0, d) (plain load): v belongs to an earlier launch, skip.  parent[v] <= u (plain
//                     load): skip.  Else old = atomicMin(&parent[v], u) at device scope; old == INT_MAX is the first touch
//                     and it alone stores level[v] = d, appends v to the OTHER list and adds v's out-degree to the sum.
//     k_bfs_pull      one thread per vertex.  A v with level[v] == -1 scans AT's row v, ascending, for the first w with
//                     level[w] == d - 1: a lane walks kBfsPullLight entries of its own row with early exit; the lanes
//                     that exhaust them without a hit hand the rest of their rows to the whole wave one after another, 64
//                     entries per step, the first step with a hit ends the row and the lowest hit lane is the parent.  A
//                     found v stores parent[v] and level[v] = d, is appended and adds its out-degree (A.row_ptr).
// Both kinds keep level[], parent[] and the next list, so a change of direction costs no conversion pass.
//
// Why the result is unique.  The vertices of level d are those unreached vertices with an in-neighbour of level d - 1:
// push touches exactly them (every edge out of the frontier is walked), pull finds exactly them (every in-row of an
// unreached vertex is scanned to its first frontier member or to its end).  parent(v) = the smallest such in-neighbour:
// in push the minimum of the atomicMin operands over all frontier u with (u, v) stored, in pull the first hit of an
// ascending row.  So levels are shortest-path distances, parents are the smallest vertex one level up, and the bits are
// the same on every run, for every direction and every knob.  The ORDER inside a list depends on scheduling and changes
// nothing: a launch consumes the whole list.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores.  Every decision
// rests on the return value of a device-scope atomic or on a value from before the launch (the list and its size, A, AT,
// level[] values below d).  The plain loads of words that the same launch changes:
//   push, level[v]:   the launch stores only d there, over -1.  The filter asks for a value in [0, d): neither -1 nor d
//                     passes it, stale or not.
//   push, parent[v]:  only ever lowered.  A stale value is an older one, so only ever HIGHER than the true one: a vertex
//                     the load lets pass merely runs its atomic, whose return value decides; one it skips has
//                     parent[v] <= u in truth, and the atomic would have changed nothing and returned no INT_MAX.
//   pull, level[w]:   the test is == d - 1, a value from before the launch; a concurrent store writes d, which never
//                     reads as d - 1.  Only thread v writes level[v] and parent[v]: pull needs no atomic but the append.
// The stores to level[], parent[] and the lists are otherwise read by the next launch only.  No kernel waits for another
// workgroup: every loop is bounded by a row's length or by the list size the host passed in.
//
// Cost.  One synchronisation per level, one before the first (the source's out-degree and the operand checks), and one
// more where the call transposes or canonicalises.  A frontier vertex's row is walked by ONE group of W lanes: a hub in
// the frontier is a serial tail of degree / W steps, as in kcore.hip.  DESIGN.md 4.18.
#include "internal.hpp"
#include "wave.hpp"

#include <algorithm>

namespace bsp {

constexpr int kBtThreads = 256;
constexpr int kBfsPullLight = 32;       // entries of its own in-row that a lane of k_bfs_pull walks before the wave takes over
                                        // (unmeasured starting value: BSPGEMM_OPT_DOT_LIGHT's outcome; tests/bfs_tree_ref.py mirrors it)
constexpr unsigned kBtErrRange = 1u;    // a column outside [0, n) met by a launch

struct BtLevel {
    int size;                           // entries appended to the list this block belongs to
    unsigned err;                       // kBtErrRange
    unsigned long long deg;             // the sum of their out-degrees
};
struct BtCounters {
    BtLevel lvl[2];
    unsigned canon;                     // the canonical checks: two bits per operand (kSetErrRange, kSetErrOrder), A / AT
    int pad[3];
};

// The frontier lists are appended to by wave_append (wave.hpp).  A vertex is appended once in its life, so a list never
// passes n entries; the store is bounded all the same.

// the end of a launch: the wave's out-degree sum and error bit, one atomic each per wave.  Whole wave.
__device__ __forceinline__ void bt_finish(long long dsum, bool bad, BtLevel *out, int lane)
{
    dsum = wave_sum(dsum);
    const u64 b = __ballot(bad);
    if (lane == 0) {
        if (dsum) atomicAdd(&out->deg, (unsigned long long)dsum);
        if (b) atomicOr(&out->err, kBtErrRange);
    }
}

// level = -1, parent = INT_MAX; the source: level 0, its own parent, the one entry of list 0.  cnt was zeroed by the host.
__global__ __launch_bounds__(kBtThreads) void k_bfs_tree_init(int n, int source, const int *__restrict__ rpA,
                                                             int *__restrict__ level, int *__restrict__ parent,
                                                             int *__restrict__ list, BtCounters *cnt)
{
    const long long v = (long long)blockIdx.x * kBtThreads + threadIdx.x;
    if (v >= n) return;
    const bool src = v == source;
    level[v] = src ? 0 : -1;
    parent[v] = src ? source : INT_MAX;
    if (src) {
        list[0] = source;
        cnt->lvl[0].size = 1;
        cnt->lvl[0].deg = (unsigned long long)(rpA[source + 1] - rpA[source]);
    }
}

// W lanes per vertex of `list` (fsize entries, from the host).  level and parent are loaded plainly and changed in the
// same launch: neither const nor __restrict__.  `reset` is the block of the list being read: the host has it already, and
// the next launch appends to that list.
template <int W>
__global__ __launch_bounds__(kBtThreads) void k_bfs_push(int n, int d, int fsize, const int *__restrict__ list,
                                                        const int *__restrict__ rpA, const int *__restrict__ colA, int *level,
                                                        int *parent, int *__restrict__ next, BtLevel *out, BtLevel *reset)
{
    const int lane = lane_id();
    if (blockIdx.x == 0 && threadIdx.x == 0) *reset = BtLevel{0, 0u, 0ull};
    // (open code: GroupRow of hub_chunks.hpp loads the row's end before it forms pos, and compiles to other code here)
    const long long t = (long long)blockIdx.x * kBtThreads + threadIdx.x;
    const long long f = t / W;
    const int sub = (int)(t % W);
    int u = 0;
    long long pos = 0, e = 0;                                // (64-bit: e may be INT_MAX)
    if (f < fsize) {
        u = list[f];
        pos = (long long)rpA[u] + sub;
        e = rpA[u + 1];
    }
    long long dsum = 0;
    bool bad = false;
    // the groups of a wave have different trip counts: the loop runs to the wave's longest with the other lanes
    // predicated off, because the append needs the whole wave
    while (__ballot(pos < e) != 0) {                         // (wave-uniform)
        bool take = false;
        int v = 0;
        if (pos < e) {
            v = colA[pos];
            if ((unsigned)v >= (unsigned)n) {                // before v indexes anything
                bad = true;
            } else {
                const int lv = level[v];
                if (!(lv >= 0 && lv < d) && parent[v] > u && atomicMin(&parent[v], u) == INT_MAX) {
                    level[v] = d;
                    dsum += rpA[v + 1] - rpA[v];
                    take = true;
                }
            }
        }
        wave_append(take, v, next, &out->size, n, lane);
        pos += W;
    }
    bt_finish(dsum, bad, out, lane);
}

// one thread per vertex.  level is loaded plainly (other vertices') and stored (the thread's own) in the same launch:
// neither const nor __restrict__.
__global__ __launch_bounds__(kBtThreads) void k_bfs_pull(int n, int d, const int *__restrict__ rpT, const int *__restrict__ colT,
                                                        const int *__restrict__ rpA, int *level, int *__restrict__ parent,
                                                        int *__restrict__ next, BtLevel *out, BtLevel *reset)
{
    const int lane = lane_id();
    if (blockIdx.x == 0 && threadIdx.x == 0) *reset = BtLevel{0, 0u, 0ull};
    const long long v = (long long)blockIdx.x * kBtThreads + threadIdx.x;
    const bool mine = v < n && level[v] == -1;
    if (__ballot(mine) == 0) return;                         // (wave-uniform)
    const int want = d - 1;
    long long b = 0, e = 0;
    bool found = false, bad = false;
    int p = 0;
    if (mine) {
        b = rpT[v];
        e = rpT[v + 1];
        const long long stop = e - b > kBfsPullLight ? b + kBfsPullLight : e;
        for (; b < stop; b++) {
            const int w = colT[b];
            if ((unsigned)w >= (unsigned)n) {                // before w indexes anything
                bad = true;
                continue;
            }
            if (level[w] == want) {
                found = true;
                p = w;
                break;
            }
        }
    }
    // the rows that are not exhausted, one after another by the whole wave (b: the first entry not yet looked at)
    for (u64 m = __ballot(mine && !found && b < e); m != 0; m &= m - 1) {   // (wave-uniform)
        const int src = __ffsll((long long)m) - 1;
        const long long rb = __shfl(b, src, 64), re = __shfl(e, src, 64);
        for (long long at = rb; at < re; at += 64) {
            int w = -1;
            if (at + lane < re) w = colT[at + lane];
            const bool in = (unsigned)w < (unsigned)n;
            if (at + lane < re && !in) bad = true;
            const bool hit = in && level[w] == want;
            const u64 hb = __ballot(hit);
            if (hb != 0) {                                   // (wave-uniform)
                const int pw = __shfl(w, __ffsll((long long)hb) - 1, 64);
                if (lane == src) {
                    found = true;
                    p = pw;
                }
                break;
            }
        }
    }
    long long dsum = 0;
    if (found) {
        parent[v] = p;
        level[v] = d;
        dsum = rpA[v + 1] - rpA[v];
    }
    wave_append(found, (int)v, next, &out->size, n, lane);
    bt_finish(dsum, bad, out, lane);
}

// the result's int64 row_ptr: the reached vertices before v (k_dot_row_ptr of dot.hip with the identity for a row_ptr)
__global__ __launch_bounds__(256) void k_bfs_tree_row_ptr(int n, long long words, const u64 *__restrict__ flags,
                                                         const long long *__restrict__ pre, long long *__restrict__ out)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > n) return;
    out[v] = v >= n ? pre[words] : pre[v >> 6] + __popcll(flags[v >> 6] & mask_lt((int)(v & 63)));
}

template <int W>
static void launch_push(int n, int d, int fsize, const int *list, const bspgemm_matrix *A, int *level, int *parent, int *next,
                        BtLevel *out, BtLevel *reset, hipStream_t s)
{
    hipLaunchKernelGGL(k_bfs_push<W>, grid_for((long long)fsize * W, kBtThreads), dim3(kBtThreads), 0, s, n, d, fsize, list,
                       A->d_row_ptr, A->d_col_idx, level, parent, next, out, reset);
}

}  // namespace bsp

using namespace bsp;

static const char kBtWho[] = "bspgemm_bfs_tree";

// A buffer of the result: from the context's cache of freed results, else ONE request.  result_alloc would drop the cache
// and ask again after an out-of-memory answer; here the workspace request at the head of the call, many times these
// 16 n bytes, has done that already where it was needed, so a failure of these is reported as one.
static hipError_t tree_buffer(bspgemm_context *ctx, void **out, size_t bytes)
{
    if (result_cached(ctx, bytes)) return result_alloc(ctx, out, bytes);
    return dev_alloc_bytes(out, bytes);
}

extern "C" bspgemm_status bspgemm_bfs_tree(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT, int source,
                                           bspgemm_bfs_direction direction, int max_depth, bspgemm_result **tree,
                                           bspgemm_bfs_tree_info *info)
{
    if (tree) *tree = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!ctx || !A || !tree) return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_bfs_tree: NULL argument");
    if (direction != BSPGEMM_BFS_AUTO && direction != BSPGEMM_BFS_PUSH && direction != BSPGEMM_BFS_PULL)
        return FAIL(BSPGEMM_ERR_INVALID, "bspgemm_bfs_tree: unknown direction");
    if (bspgemm_status st = check_graph_operand(ctx, A, kBtWho, NEED_SQUARE)) return st;
    const int n = A->rows;
    if (source < 0 || source >= n) {
        snprintf(g_err, sizeof g_err, "%s: source %d outside [0, %d)", kBtWho, source, n);
        return BSPGEMM_ERR_INVALID;
    }
    if (direction == BSPGEMM_BFS_PUSH) AT = nullptr;         // ignored
    if (bspgemm_status st = check_transposed_operand(ctx, A, AT, kBtWho)) return st;
    if (bspgemm_status st = check_operand(ctx, A, kBtWho, NEED_ENTRIES_CONSISTENT)) return st;
    // BSPGEMM_BFS_TREE_TIMING: host clocks around the stages; a launch is then synchronised before its read-back is issued,
    // so that the two are told apart
    StageClock clk(ctx->bfs_tree_timing, ctx->stream);
    double ms_tr = 0, ms_push = 0, ms_pull = 0, ms_back = 0, ms_out = 0;
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const long long alpha = ctx->bfs_alpha, beta = ctx->bfs_beta;
    const int forced_w = ctx->bfs_push_lanes;
    const bool own_at = !AT && direction != BSPGEMM_BFS_PUSH;   // the call transposes A itself before the first pull launch

    // The workspace, grown ONCE, before anything is launched (growing it synchronises and moves it): the transpose that
    // the call may run works in the leading part, so the state of the search starts behind it; then the counters, level,
    // parent, the two lists and the flag scratch of the read-out.
    const size_t n4 = ws_pad4((size_t)n);
    const size_t o_cnt = own_at ? transpose_workspace_ints(A->nnz, n) : 0;
    BtCounters *d_cnt = nullptr;
    int *level = nullptr, *parent = nullptr, *list[2] = {nullptr, nullptr};
    FlagScratch sc;
    auto carve = [&](int *tmp) {                             // (again after anything that may have moved the workspace)
        WsCursor c(tmp, o_cnt);
        c.take(d_cnt, 1).take(level, n4).take(parent, n4).take(list[0], n4).take(list[1], n4);
        return flag_scratch_carve(tmp, c.aligned(), n, false, tmp ? &sc : nullptr);
    };
    const size_t total = carve(nullptr);
    if (!total) return FAIL(BSPGEMM_ERR_OVERFLOW, "bspgemm_bfs_tree: too many vertices for the word scan");
    if (bspgemm_status st = ensure_tmp(ctx, total)) return st;
    if (bspgemm_status st = ensure_tile_rows(ctx, (size_t)std::max(A->nnz, AT ? AT->nnz : 0))) return st;
    carve(ctx->tmp);

    bspgemm_matrix *mine = nullptr;                          // the transpose or the canonical AT that the call owns
    bspgemm_result *R = nullptr;
    auto bail = [&](bspgemm_status st) {
        hipStreamSynchronize(s);
        bspgemm_result_free(R);
        bspgemm_matrix_free(mine);
        return st;
    };
    const dim3 vgrid = vertex_grid(n, kBtThreads), block(kBtThreads);
    auto start = [&]() {
        hipError_t e = hipMemsetAsync(d_cnt, 0, sizeof(BtCounters), s);
        hipLaunchKernelGGL(k_bfs_tree_init, vgrid, block, 0, s, n, source, A->d_row_ptr, level, parent, list[0], d_cnt);
        return e;
    };
    // the first read-back: the source's out-degree, and the check of every distinct handle (A: its columns' range alone,
    // its rows may be in any order; AT: range and ascending order).  The checks write d_cnt->canon after the memset.
    HIPCHK_B(start());
    launch_graph_canonical_checks(ctx, A, AT, &d_cnt->canon, s);
    BtCounters h = {};
    clk.start();
    HIPCHK_B(round_fetch(&h, d_cnt, sizeof h, s));
    (void)clk.lap(ms_back);
    if (h.canon & (kSetErrRange | (kSetErrRange << 2))) return bail(fail_bad_column_in(kBtWho, n, h.canon));
    int canonicalised = 0;
    if (AT && (h.canon & (AT == A ? kSetErrOrder : kSetErrOrder << 2))) {
        // transposed twice, in the leading part of the workspace, which may grow for it: the state is set up again
        clk.start();
        if (bspgemm_status st = operand_canonical(ctx, AT, &mine)) return bail(st);
        if (bspgemm_status st = ensure_tmp(ctx, total)) return bail(st);
        AT = mine;
        canonicalised = 1;
        carve(ctx->tmp);
        HIPCHK_B(start());
        HIPCHK_B(clk.lap(ms_tr, true));
    }

    long long n_f = h.lvl[0].size, m_f = (long long)h.lvl[0].deg, prev_nf = 0;
    if (n_f != 1 || m_f < 0 || m_f > A->nnz) return bail(fail_stuck(kBtWho));
    long long reached = 1, m_u = A->nnz - m_f, edges_pushed = 0;
    uint64_t pull_mask = 0;
    int d = 0, cur = 0, pushes = 0, pulls = 0, transposed = 0;
    bool pulling = direction == BSPGEMM_BFS_PULL;
    while (n_f > 0 && (max_depth <= 0 || d < max_depth)) {
        if (pushes + pulls >= n) return bail(fail_stuck(kBtWho));   // defensive: a level holds at least one new vertex
        d++;
        if (direction == BSPGEMM_BFS_AUTO) {                 // (the rule is part of the header's contract)
            if (!pulling) pulling = m_f * alpha > m_u && n_f > prev_nf;
            else pulling = !(n_f * beta < n);
        }
        if (pulling && !AT) {
            clk.start();
            if (bspgemm_status st = bspgemm_matrix_transpose(ctx, A, &mine)) return bail(st);   // (works in front of o_cnt)
            AT = mine;
            transposed = 1;
            (void)clk.lap(ms_tr);
        }
        BtLevel *out = &d_cnt->lvl[cur ^ 1], *reset = &d_cnt->lvl[cur];
        clk.start();
        if (pulling) {
            hipLaunchKernelGGL(k_bfs_pull, vgrid, block, 0, s, n, d, AT->d_row_ptr, AT->d_col_idx, A->d_row_ptr, level, parent,
                               list[cur ^ 1], out, reset);
            pulls++;
            if (d <= 64) pull_mask |= (uint64_t)1 << (d - 1);
        } else {
            // the lanes per frontier vertex: the smallest W at or above the frontier's MEAN out-degree -- no chunk records
            // here, so a frontier hub is a serial tail of degree / W steps
            const int W = forced_w ? forced_w : lanes_for_mean(m_f, n_f, 1);
            dispatch_lanes(W, [&](auto w) {
                launch_push<decltype(w)::value>(n, d, (int)n_f, list[cur], A, level, parent, list[cur ^ 1], out, reset, s);
            });
            pushes++;
            edges_pushed += m_f;
        }
        HIPCHK_B(hipGetLastError());
        HIPCHK_B(clk.lap(pulling ? ms_pull : ms_push, true));
        clk.longest(clk.last, d, (int)n_f);
        BtLevel hl = {};
        HIPCHK_B(hipMemcpyAsync(&hl, out, sizeof hl, hipMemcpyDeviceToHost, s));
        HIPCHK_B(hipStreamSynchronize(s));                   // the launch's one synchronisation
        (void)clk.lap(ms_back);
        if (hl.err) return bail(fail_bad_column(kBtWho, n));
        prev_nf = n_f;
        n_f = hl.size;
        m_f = (long long)hl.deg;
        if (n_f < 0 || n_f > n - reached || m_f < 0 || m_f > m_u) return bail(fail_stuck(kBtWho));
        reached += n_f;
        m_u -= m_f;
        cur ^= 1;
    }
    const int depth = n_f > 0 ? d : (d > 0 ? d - 1 : 0);     // the last launch of a complete search found nobody

    // the read-out: an ordinary counted result, released the way a product's is; its size is the sum of the frontier
    // sizes, which the host knows, so nothing is read back for it
    clk.start();
    R = new (std::nothrow) bspgemm_result{ctx, n, reached, nullptr, nullptr, 0};
    if (!R) return bail(FAIL(BSPGEMM_ERR_ALLOC, "result"));
    HIPCHK_B(tree_buffer(ctx, reinterpret_cast<void **>(&R->d_row_ptr), result_bytes_rowptr(n)));
    HIPCHK_B(tree_buffer(ctx, reinterpret_cast<void **>(&R->d_col_idx), result_bytes_colidx(reached)));
    R->col_cap = reached;
    HIPCHK_B(tree_buffer(ctx, reinterpret_cast<void **>(&R->d_values), result_bytes_colidx(reached)));
    launch_select_flags_value(level, n, BSPGEMM_CMP_GE, 0, sc.flags, sc.cnt, s);
    launch_scan_counts(sc.cnt, sc.words, sc.pre, sc.part, nullptr, s);
    launch_select_scatter(parent, n, sc.flags, sc.pre, R->d_col_idx, s);
    launch_select_scatter(level, n, sc.flags, sc.pre, R->d_values, s);
    hipLaunchKernelGGL(k_bfs_tree_row_ptr, row_pass_grid(n), dim3(256), 0, s, n, (long long)sc.words, sc.flags, sc.pre,
                       R->d_row_ptr);
    HIPCHK_B(hipGetLastError());
    HIPCHK_B(hipStreamSynchronize(s));
    if (clk.on) {
        (void)clk.lap(ms_out);
        fprintf(stderr, "[bspgemm] %s: n %d nnz %lld source %d reached %lld depth %d | total %.3f ms = transpose %.3f + %d push "
                        "launches %.3f + %d pull launches %.3f + read-backs %.3f + read-out %.3f + rest | longest launch %.3f ms "
                        "(level %d, %d frontier vertices)\n",
                kBtWho, n, (long long)A->nnz, source, reached, depth, clk.total(), ms_tr, pushes, ms_push, pulls, ms_pull,
                ms_back, ms_out, clk.max_ms, clk.max_tag[0], clk.max_tag[1]);
    }
    bspgemm_matrix_free(mine);
    if (info) {
        info->reached = reached;
        info->edges_pushed = edges_pushed;
        info->pull_mask = pull_mask;
        info->depth = depth;
        info->complete = n_f == 0;
        info->push_levels = pushes;
        info->pull_levels = pulls;
        info->transposed = transposed;
        info->canonicalised = canonicalised;
    }
    *tree = R;
    return BSPGEMM_OK;
}
