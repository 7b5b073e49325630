"""The reference of the shortest-path tests (bspgemm_weights_*, bspgemm_sssp): the weight hash of include/bspgemm.h, a heap
Dijkstra in Python integers (the definition; also right above 2^53, where a float Dijkstra is not), the tight-predecessor
parents, a numpy model of the synchronous near-far rounds as the library runs them that returns the distances and every
field of bspgemm_sssp_info for a given delta and lanes (the default delta formula included) and asserts the 2 n + 2 bound
on the rounds, and the graphs the tests use.  Nothing here touches the GPU.
"""
import collections
import heapq

import numpy as np

import cc_ref
import gen
from color_ref import mix32

INF = 2 ** 64 - 1
NONE = np.uint64(INF)
LANES = (0, 4, 16, 64)   # bspgemm_sssp_params.lanes
CHUNK = 4096             # csrc/sssp.hip kSsspChunk: the longest row left to one group of lanes, and the entries of a chunk
DEEP = 4                 # csrc/sssp.hip kSsspDeep: steps of a row in flight per trip
DELTA_C = 32             # BSPGEMM_SSSP_DELTA_C
SETTLE_STRIDE = 256 * 1024   # csrc/sssp.hip kSsspSettleBlocks * kSsspListThreads: candidates one stride of the settle covers
INFO = ("delta", "dist_max", "reached", "entries_walked", "improved", "hub_chunks", "rounds", "buckets", "lanes", "reserved")

Sssp = collections.namedtuple("Sssp", "dist " + " ".join(INFO))
Graph = collections.namedtuple("Graph", "rp ci n w source")


def weight_hash(rp, ci, n, seed, wmin, wmax, symmetric=False):
    """uint32[nnz]: w = wmin + mix32(mix32(a ^ seed) ^ b) % (wmax - wmin + 1), (a, b) = (row, col) or (min, max)"""
    assert 0 <= wmin <= wmax < 2 ** 32
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci, np.int64)
    a, b = (np.minimum(rows, cols), np.maximum(rows, cols)) if symmetric else (rows, cols)
    h = mix32(mix32(a.astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)) ^ b.astype(np.uint32))
    return (np.uint64(wmin) + h.astype(np.uint64) % np.uint64(wmax - wmin + 1)).astype(np.uint32)


def dijkstra(rp, ci, w, n, source):
    """uint64[n]: the definition, by a heap over Python integers; INF = unreached"""
    rp, ci, w = np.asarray(rp).tolist(), np.asarray(ci).tolist(), np.asarray(w).tolist()
    dist = [INF] * n
    if n == 0:
        return np.zeros(0, np.uint64)
    dist[source] = 0
    heap = [(0, source)]
    while heap:
        d, u = heapq.heappop(heap)
        if d != dist[u]:
            continue
        for k in range(rp[u], rp[u + 1]):
            nd = d + w[k]
            if nd < dist[ci[k]]:
                dist[ci[k]] = nd
                heapq.heappush(heap, (nd, ci[k]))
    assert all(d == INF or d < 2 ** 63 for d in dist)
    return np.array(dist, dtype=np.uint64)


def parents(rp, ci, w, n, source, dist):
    """int32[n]: the source itself, -1 for an unreached vertex, else the smallest u with a stored entry k = (u, v) and
    dist(u) + w[k] == dist(v)"""
    dist = np.asarray(dist, np.uint64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci, np.int64)
    ok = dist[rows] != NONE
    tight = np.zeros(rows.size, bool)
    tight[ok] = dist[rows[ok]] + np.asarray(w, np.uint64)[ok] == dist[cols[ok]]
    par = np.full(n, n, np.int64)
    np.minimum.at(par, cols[tight], rows[tight])
    par[par == n] = -1
    par[dist == NONE] = -1
    if n:
        par[source] = source
    return par.astype(np.int32)


def default_delta(wsum, nnz, n, c=DELTA_C):
    """max(1, c * (sum / nnz) / max(1, nnz / n)), integer divisions in exactly this order; 1 without entries"""
    if nnz <= 0:
        return 1
    return max(1, c * (int(wsum) // nnz) // max(1, nnz // n))


def chunks_of(deg, chunk=CHUNK):
    deg = np.asarray(deg, np.int64)
    return np.where(deg > chunk, (deg + chunk - 1) // chunk, 0)


def lanes_for(nnz, n, forced=0):
    """the lanes per near-list vertex: forced, or the smallest of 4, 16, 64 at or above a quarter of the mean stored degree"""
    if forced:
        return forced
    if nnz <= 16 * n:
        return 4
    return 16 if nnz <= 64 * n else 64


def _entries_of(rp, deg, rows):
    """(owner index into rows, entry position) of every stored entry of the rows"""
    lens = deg[rows]
    total = int(lens.sum())
    owner = np.repeat(np.arange(rows.size), lens)
    first = np.cumsum(lens) - lens
    pos = np.repeat(np.asarray(rp, np.int64)[rows], lens) + (np.arange(total) - np.repeat(first, lens))
    return owner, pos


def model(rp, ci, w, n, source, delta=0, lanes=0, chunk=CHUNK):
    """the rounds as the library runs them: an Sssp.  A vertex is dirty from the moment it is lowered until its row is
    walked; a round walks the dirty vertices below T from their distances BEFORE the round"""
    if n == 0:
        return Sssp(np.zeros(0, np.uint64), *([0] * len(INFO)))
    ci, w = np.asarray(ci, np.int64), np.asarray(w, np.uint64)
    deg = np.diff(rp).astype(np.int64)
    delta = int(delta) or default_delta(int(w.sum(dtype=np.uint64)) if w.size else 0, int(ci.size), n)
    assert 1 <= delta <= INF
    dist = np.full(n, NONE, np.uint64)
    dist[source] = 0
    dirty = np.zeros(n, bool)
    near = np.array([source], np.int64)
    T, buckets, rounds, walked, improved, hubs = delta, 1, 0, 0, 0, 0
    while True:
        if near.size == 0:                                   # ADVANCE
            pend = np.flatnonzero(dirty)
            if pend.size == 0:
                break
            m = int(dist[pend].min())
            T = (m // delta + 1) * delta
            assert m < T <= INF
            buckets += 1
            near = pend[dist[pend] < np.uint64(T)]
            assert near.size                                 # every opened bucket is non-empty
        rounds += 1
        assert rounds <= 2 * n + 2, "the round bound"
        walked += int(deg[near].sum())
        hubs += int(chunks_of(deg[near], chunk).sum())
        dirty[near] = False
        owner, pos = _entries_of(rp, deg, near)
        new = dist.copy()
        np.minimum.at(new, ci[pos], dist[near[owner]] + w[pos])
        lowered = np.flatnonzero(new < dist)
        improved += int(lowered.size)
        dist = new
        dirty[lowered] = True
        near = lowered[dist[lowered] < np.uint64(T)]
    fin = dist[dist != NONE]
    return Sssp(dist, delta, int(fin.max()), int(fin.size), walked, improved, hubs, rounds, buckets, lanes_for(int(ci.size), n, lanes), 0)


def model_of(g, delta=0, lanes=0):
    """model() of a Graph"""
    return model(g.rp, g.ci, g.w, g.n, g.source, delta, lanes)


def reference_of(g):
    """(dist, parent) of a Graph by the definition"""
    dist = dijkstra(g.rp, g.ci, g.w, g.n, g.source)
    return dist, parents(g.rp, g.ci, g.w, g.n, g.source, dist)


# ---------------------------------------------------------------- graphs ---------------------------------------------
def _graph(rows, cols, n, w=None, source=0, hashed=(7, 1, 255)):
    rp, ci, n = cc_ref.csr(rows, cols, n)
    if w is None:
        w = weight_hash(rp, ci, n, *hashed)
    else:                                                    # (cc_ref.csr groups the pairs by row, stably)
        w = np.asarray(w, np.uint64)[np.argsort(np.asarray(rows, np.int64), kind="stable")].astype(np.uint32)
    return Graph(rp, ci, n, w, source)


# rows of these stored lengths: the lane-stride and tail edges, W x (steps in flight) +- 1 for W = 4, 16, 64 among them
ROW_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def row_lengths():
    """vertex i < len(ROW_LENGTHS) has a row of ROW_LENGTHS[i] random columns (unsorted, repeats), the source n - 1 reaches
    each of them and the rest have rows of 2: every listed length is walked"""
    rng = np.random.default_rng(5)
    n, k = 331, len(ROW_LENGTHS)
    lens = list(ROW_LENGTHS) + [2] * (n - 1 - k) + [k]
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n - 1, rows.size)
    cols[rows == n - 1] = np.arange(k)
    return _graph(rows, cols, n, source=n - 1)


def star(leaves, late=False):
    """the hub with a row of `leaves` entries; late: behind a path of three edges from the source"""
    if not late:
        return _graph(np.full(leaves, leaves), np.arange(leaves), leaves + 1, source=leaves)
    hub, n = leaves, leaves + 4
    rows = np.concatenate([[n - 1, n - 2, n - 3], np.full(leaves, hub)])
    cols = np.concatenate([[n - 2, n - 3, hub], np.arange(leaves)])
    return _graph(rows, cols, n, source=n - 1)


def near_star(leaves):
    """the star's hub as the source, and every leaf with an entry back to the hub and one to the next leaf"""
    hub, i = leaves, np.arange(leaves)
    rows = np.concatenate([np.full(leaves, hub), i, i])
    cols = np.concatenate([i, np.full(leaves, hub), (i + 1) % leaves])
    return _graph(rows, cols, leaves + 1, source=hub)


def hub_twice(leaves):
    """s -> hub (10), s -> a (1), a -> hub (1), hub -> leaves (3 each): in one bucket the hub is lowered in round 1 and again
    in round 2, so its row is walked in rounds 2 and 3 and its chunk records are emitted twice"""
    hub, a, s, n = leaves, leaves + 1, leaves + 2, leaves + 3
    rows = np.concatenate([[s, s, a], np.full(leaves, hub)])
    cols = np.concatenate([[hub, a, hub], np.arange(leaves)])
    w = np.concatenate([[10, 1, 1], np.full(leaves, 3)])
    return _graph(rows, cols, n, w, source=s)


def snap_rule():
    """s -> a (1), s -> b (5), a -> b (1), b -> c (1): in one bucket round 2 walks a and b; a lowers b to 2 while b is walked
    from its settled 5, so c gets 6 in round 2 and 3 in round 3 -- three rounds with 2 + 2 + 1 vertices lowered, and a fourth
    that walks c's empty row"""
    s, a, b, c = 0, 1, 2, 3
    return _graph([s, s, a, b], [a, b, b, c], 5, [1, 5, 1, 1], source=s)


def untidy():
    """unsorted rows, repeated entries with different weights, self-loops (one of length 0), zero-length edges and a
    zero-length 2-cycle 4 <-> 5, and the unreachable 7 and 8 (8 -> 0)"""
    rows = [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 8]
    cols = [3, 1, 1, 0, 2, 1, 2, 6, 3, 3, 4, 5, 4, 4, 6, 2, 0]
    w = [9, 4, 2, 5, 7, 0, 3, 0, 0, 1, 0, 0, 8, 0, 2, 0, 1]
    return _graph(rows, cols, 9, w, source=0)


def heavy_path():
    """a path of 6 vertices with edges of 2^32 - 1: the distances pass 2^32"""
    return _graph(np.arange(5), np.arange(1, 6), 6, np.full(5, 2 ** 32 - 1), source=0)


def unit_path(n=300):
    return _graph(np.arange(n - 1), np.arange(1, n), n, np.ones(n - 1), source=0)


def single():
    return _graph([], [], 1, [], source=0)


def no_entries():
    return _graph([], [], 5, [], source=3)


def rmat(scale, symmetric):
    """R-MAT, edge factor 5, lengths hashed in [1, 255]; symmetric: both directions stored, with the same length"""
    rp, ci, n = gen.rmat(scale, 5, (0.57, 0.19, 0.19, 0.05), 1200 + scale)
    if symmetric:
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        rp, ci = gen._csr_from_pairs(np.concatenate([rows, ci]), np.concatenate([ci, rows]), n)
    w = weight_hash(rp, ci, n, 7, 1, 255, symmetric)
    return Graph(rp, ci, n, w, int(np.argmax(np.diff(rp))))      # a hub source


def dense(n, d, seed):
    """rows of about d distinct columns: the automatic lanes are 16 at a mean degree above 16, 64 above 64"""
    rp, ci, n = gen.uniform(n, d, seed)
    return Graph(rp, ci, n, weight_hash(rp, ci, n, 3, 0, 1000), 1)


def settle_stride():
    """a star whose round 1 lowers more vertices than the settle grid covers in one stride"""
    return star(SETTLE_STRIDE + 5)


SMALL = {
    "row_lengths": row_lengths,
    "snap_rule": snap_rule,
    "untidy": untidy,
    "heavy_path": heavy_path,
    "single": single,
    "no_entries": no_entries,
    "dense16": lambda: dense(200, 40, 21),
    "dense64": lambda: dense(300, 100, 22),
}
HUB_GRAPHS = dict([("star_%d" % d, (lambda d=d: star(d))) for d in (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)]
                  + [("late_star_%d" % d, (lambda d=d: star(d, late=True))) for d in (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)]
                  + [("near_star_%d" % d, (lambda d=d: near_star(d))) for d in (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)]
                  + [("hub_twice_%d" % d, (lambda d=d: hub_twice(d))) for d in (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)])
RMAT_GRAPHS = {
    "rmat10": lambda: rmat(10, False),
    "rmat10_sym": lambda: rmat(10, True),
    "rmat12": lambda: rmat(12, False),
    "rmat12_sym": lambda: rmat(12, True),
}
GRAPHS = dict(SMALL, **HUB_GRAPHS, **RMAT_GRAPHS, unit_path300=unit_path, settle_stride=settle_stride)
DELTAS = (1, 16, 0, INF)     # 0: the default
