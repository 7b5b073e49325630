"""The reference of the PageRank tests (bspgemm_pagerank): the numpy model of the header's definition in unsigned 64-bit fixed
point (uint64 throughout, np.add.at over the canonical entries), a naive model in Python integers to check it with, a
float64 power iteration with the same quantised damping D / 2^32, the in-degree classes of csrc/pagerank.hip, and the graphs
the tests use.  Nothing here touches the GPU.
"""
import math

import numpy as np
from scipy.sparse import csr_matrix

import cc_ref
import gen
from bspgemm import PR_AUTO, PR_PULL, PR_PUSH  # noqa: F401  (bspgemm_pr_method, as the Python view names it)
import kcore_ref
import lcc_ref

LANE_CAP = 8             # csrc/pagerank.hip kPrLaneCap: the longest row of AT one lane sums (0 included)
WAVE_CAP = 256           # csrc/pagerank.hip kPrWaveCap: the longest row one wave sums
GROUP_CAP = 4096         # csrc/pagerank.hip kPrGroupCap: the longest row one workgroup sums; longer rows are hubs
HUB_CHUNK = 4096         # csrc/pagerank.hip kPrHubChunk: entries of a hub's row per workgroup
CAPS = (LANE_CAP, WAVE_CAP, GROUP_CAP)
ONE = 1 << 62
U = np.uint64


def edges(rp, ci, n):
    """(src, dst) int64 of the distinct stored entries, sorted by (src, dst): the canonical A"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    if n == 0 or ci.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    key = np.unique(np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + ci)
    return key // n, key % n


def canonical(rp, ci, n):
    src, dst = edges(rp, ci, n)
    return cc_ref.csr(src, dst, n)


def is_canonical(rp, ci, n):
    """every row strictly ascending: what the library's canonical check asks"""
    crp, cci, _ = canonical(rp, ci, n)
    return np.array_equal(crp, rp) and np.array_equal(cci, ci)


def transposed(rp, ci, n):
    src, dst = edges(rp, ci, n)
    o = np.lexsort((src, dst))
    return cc_ref.csr(dst[o], src[o], n)


def constants(n, damping):
    """(q, D, B) as Python integers"""
    q = ONE // n if n else 0
    D = int(math.floor(damping * 4294967296.0 + 0.5))
    return q, D, ((4294967296 - D) * q) >> 32


def threshold(tolerance):
    return int(math.floor(tolerance * 2.0 ** 62))


def trajectory(rp, ci, n, damping, max_iter, tolerance=0.0):
    """([r_0, r_1, ...] uint64 arrays, [delta_1, ...] Python ints, converged) of the definition: max_iter iterations, or
    (tolerance > 0) up to the first one with delta <= floor(tolerance * 2^62)"""
    src, dst = edges(rp, ci, n)
    q, D, B = constants(n, damping)
    outdeg = np.bincount(src, minlength=n).astype(U)
    dangling = outdeg == 0
    safe = np.where(dangling, U(1), outdeg)
    D64, B64, lo32, s32 = U(D), U(B), U(0xFFFFFFFF), U(32)
    rs, deltas = [np.full(n, q, U)], []
    while len(deltas) < max_iter:
        r = rs[-1]
        c = np.where(dangling, U(0), r // safe)
        share = int(r[dangling].sum(dtype=U)) // n if n else 0
        s = np.full(n, share, U)
        np.add.at(s, dst, c[src])
        rn = B64 + D64 * (s >> s32) + ((D64 * (s & lo32)) >> s32)
        rs.append(rn)
        deltas.append(int(np.where(rn > r, rn - r, r - rn).sum(dtype=U)))
        if tolerance > 0 and deltas[-1] <= threshold(tolerance):
            return rs, deltas, True
    return rs, deltas, False


def to_double(r):
    return np.asarray(r, U).astype(np.float64) * 2.0 ** -62


def result(rs, deltas, converged, rp, ci, n, at=None):
    """what the call returns after `at` iterations (default: all of the trajectory)"""
    at = len(deltas) if at is None else at
    src, _ = edges(rp, ci, n)
    r = rs[at]
    return {"fixed": r, "rank": to_double(r), "mass": int(r.sum(dtype=U)), "delta": deltas[at - 1] if at else 0,
            "dangling": int((np.bincount(src, minlength=n) == 0).sum()) if n else 0, "iterations": at,
            "converged": int(converged and at == len(deltas))}


def pagerank(rp, ci, n, damping=0.85, max_iter=20, tolerance=0.0):
    return result(*trajectory(rp, ci, n, damping, max_iter, tolerance), rp, ci, n)


def naive(rp, ci, n, damping, max_iter, tolerance=0.0):
    """(r as a list of Python ints, deltas, converged) from the definition, vertex by vertex"""
    rp, ci = np.asarray(rp).tolist(), np.asarray(ci).tolist()
    out = [sorted(set(ci[rp[u]:rp[u + 1]])) for u in range(n)]
    q, D, B = constants(n, damping)
    r, deltas = [q] * n, []
    while len(deltas) < max_iter:
        c = [r[u] // len(out[u]) if out[u] else 0 for u in range(n)]
        share = sum(r[u] for u in range(n) if not out[u]) // n if n else 0
        s = [share] * n
        for u in range(n):
            for v in out[u]:
                s[v] += c[u]
        assert all(x < 1 << 63 for x in s)
        rn = [B + D * (x >> 32) + ((D * (x & 0xFFFFFFFF)) >> 32) for x in s]
        assert all(y == B + (D * x >> 32) for x, y in zip(s, rn))        # the split product is the exact one
        deltas.append(sum(abs(a - b) for a, b in zip(rn, r)))
        r = rn
        if tolerance > 0 and deltas[-1] <= threshold(tolerance):
            return r, deltas, True
    return r, deltas, False


def float_iteration(rp, ci, n, damping, iterations):
    """a plain float64 power iteration with the damping the fixed-point form uses, D / 2^32"""
    src, dst = edges(rp, ci, n)
    d = constants(n, damping)[1] / 4294967296.0
    outdeg = np.bincount(src, minlength=n).astype(np.float64)
    dangling = outdeg == 0
    M = csr_matrix((np.ones(src.size), (dst, src)), shape=(n, n))
    r = np.full(n, 1.0 / n)
    for _ in range(iterations):
        c = np.where(dangling, 0.0, r / np.where(dangling, 1.0, outdeg))
        r = (1.0 - d) / n + d * (M @ c + r[dangling].sum() / n)
    return r


# ---------------------------------------------------------------- the in-degree classes of csrc/pagerank.hip ---------
def indegree(rp, ci, n):
    return np.bincount(edges(rp, ci, n)[1], minlength=n)


def class_vertices(rp, ci, n, min_class=0):
    """bspgemm_pr_info.class_vertices under PULL: every vertex, in-degree 0 included, in class max(own, min_class)"""
    own = np.searchsorted(np.array(CAPS), indegree(rp, ci, n), side="left")     # d <= cap: that class
    return np.bincount(np.maximum(own, min_class), minlength=4).tolist()


def hub_chunks(rp, ci, n, min_class=0):
    d = indegree(rp, ci, n)
    hubs = d > GROUP_CAP if min_class < 3 else d >= 0
    return int(((d[hubs] + HUB_CHUNK - 1) // HUB_CHUNK).sum())


# ---------------------------------------------------------------- graphs ---------------------------------------------
def _pairs(pairs, n):
    return cc_ref.csr([p[0] for p in pairs], [p[1] for p in pairs], n)


def _empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), n


def sink_star(K):
    """three sinks of in-degree K - 1, K and K + 1 (vertices K + 1, K + 2, K + 3) fed by the sources 0 .. K, which also
    point at each other: source i at i + 1, every third one at i + 2 and at i + 5 too (out-degrees 1 .. 6, in-degrees <= 3).
    The sinks are dangling."""
    m = K + 1
    i = np.arange(m)
    rows = [i[:K - 1], i[:K], i, i, i[::3], i[::3]]
    cols = [np.full(K - 1, m), np.full(K, m + 1), np.full(m, m + 2), (i + 1) % m, (i[::3] + 2) % m, (i[::3] + 5) % m]
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), m + 3)


def hub_chunks_graph():
    """vertex 0 with in-degree 3 * HUB_CHUNK + 1 (four chunks, the last of one entry); every other source also points on"""
    m = 3 * HUB_CHUNK + 1
    i = np.arange(1, m + 1)
    odd = i[i % 2 == 1]
    return cc_ref.csr(np.concatenate([i, odd, [0]]), np.concatenate([np.zeros(m, np.int64), 1 + (odd * 7) % m, [5]]), m + 1)


def source_star():
    """vertex 0 with out-degree 5000: PUSH's contended row and a small c(u); every second leaf points back"""
    i = np.arange(1, 5001)
    return cc_ref.csr(np.concatenate([np.zeros(5000, np.int64), i[::2]]), np.concatenate([i, np.zeros(2500, np.int64)]), 5001)


def self_loops_graph():
    """a self-loop on every vertex of 37, a vertex with nothing else, and i -> i + 1 from the even ones"""
    i = np.arange(37)
    return cc_ref.csr(np.concatenate([i, i[:-1:2]]), np.concatenate([i, i[:-1:2] + 1]), 37)


def rmat11_cut():
    """directed R-MAT scale 11 cut to its first 2011 vertices: neither n nor nnz is a multiple of 64"""
    rp, ci, n = gen.rmat(11, 8, kcore_ref.SKEW, 5601)
    src, dst = edges(rp, ci, n)
    keep = (src < 2011) & (dst < 2011)
    return cc_ref.csr(src[keep], dst[keep], 2011)


def symmetric_rmat9():
    rp, ci, n = gen.rmat(9, 6, kcore_ref.SKEW, 5602)
    src, dst = edges(rp, ci, n)
    both = np.unique(np.concatenate([src * n + dst, dst * n + src]))
    return cc_ref.csr(both // n, both % n, n)


def n_4097():
    """vertices beyond one tile of 4096, entries under one; the last vertex has edges both ways"""
    rng = np.random.default_rng(5603)
    r, c = rng.integers(0, 4097, size=(2, 2990))
    return cc_ref.csr(np.concatenate([r, [4096, 4096, 17]]), np.concatenate([c, [3, 4000, 4096]]), 4097)


GRAPHS = {
    "empty0": lambda: _empty(0),
    "empty1": lambda: _empty(1),
    "loop1": lambda: _pairs([(0, 0)], 1),
    "all_dangling": lambda: _empty(300),
    "two_cycle": lambda: _pairs([(0, 1), (1, 0)], 2),
    "dir_cycle257": lambda: cc_ref.csr(np.arange(257), (np.arange(257) + 1) % 257, 257),
    "path_dangling_end": lambda: cc_ref.path(50),
    "sink_star_8": lambda: sink_star(LANE_CAP),
    "sink_star_256": lambda: sink_star(WAVE_CAP),
    "sink_star_4096": lambda: sink_star(GROUP_CAP),
    "hub_chunks": hub_chunks_graph,
    "source_star": source_star,
    "self_loops": self_loops_graph,
    "dups_unsorted": lambda: gen.dups_unsorted(300, 6, 5604),
    "untidy": lambda: lcc_ref.untidy(150, 2200, 5605),
    "rmat11": rmat11_cut,
    "symmetric_rmat9": symmetric_rmat9,
    "n_4097": n_4097,
}
SMALL = ("empty0", "empty1", "loop1", "two_cycle", "path_dangling_end", "self_loops", "sink_star_8", "untidy")
DAMPINGS = (0.85, 0.0, 1.0, 0.5000001)
ITERATIONS = (0, 1, 2, 20)

_cache = {}


def graph(name):
    """the named graph, built once"""
    if name not in _cache:
        rp, ci, n = GRAPHS[name]()
        rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        rp.setflags(write=False)
        ci.setflags(write=False)
        _cache[name] = (rp, ci, n)
    return _cache[name]


def cached_trajectory(name, damping, max_iter=max(ITERATIONS)):
    """the trajectory of a named graph under tolerance 0, computed once and shared (read-only)"""
    key = (name, damping, max_iter)
    if key not in _cache:
        rs, deltas, conv = trajectory(*graph(name), damping, max_iter)
        for r in rs:
            r.setflags(write=False)
        _cache[key] = (rs, deltas, conv)
    return _cache[key]
