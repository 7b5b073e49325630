"""The reference of the PageRank tests (bspgemm_pagerank): the numpy model of the header's definition in unsigned 64-bit fixed
point (uint64 throughout, np.add.at over the canonical entries), a naive model in Python integers to check it with, a
float64 power iteration with the same quantised damping D / 2^32, the in-degree classes of csrc/pagerank.hip, a host model of
the kernel edges an input reaches (cells), and the graphs the tests use.  Nothing here touches the GPU.
"""
import math
import os
import re

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


# ---------------------------------------------------------------- the kernel edges ("cells") an input reaches ---------
THREADS = 256            # csrc/pagerank.hip kPrThreads
WAVES = THREADS // 64    # csrc/pagerank.hip kPrWaves
MAX_BLOCKS = 2048        # csrc/pagerank.hip kPrMaxBlocks: the workgroups of a grid-stride launch at the most
LANES_MEAN = 32          # csrc/pagerank.hip, bspgemm_pagerank: wave_entries <= 32 * size gives 16 lanes per row, else 64


def _classes(rp, ci, n, min_class):
    """(in-degrees, the class of every vertex under PULL)"""
    d = indegree(rp, ci, n)
    return d, np.maximum(np.searchsorted(np.array(CAPS), d, side="left"), min_class)


def wave_lanes(rp, ci, n, min_class=0):
    """the lanes per row of the wave class: 16 where its rows hold LANES_MEAN entries or fewer in the mean, else 64 (also
    for an empty class, where nothing is launched)"""
    d, cls = _classes(rp, ci, n, min_class)
    size = int((cls == 1).sum())
    return 16 if size and int(d[cls == 1].sum()) <= LANES_MEAN * size else 64


def grid(items, per_block):
    """csrc/pagerank.hip pr_grid: the workgroups of a launch over `items`"""
    return max(1, min((items + per_block - 1) // per_block, MAX_BLOCKS))


def _trips(kernel, items, per_block):
    """the grid-stride loop of `kernel` goes round once, or some workgroup goes round again"""
    return "%s: %s" % (kernel, "second trip" if items > grid(items, per_block) * per_block else "one trip")


CELLS = frozenset(
    ["%s: %s" % (k, t) for k in ("init", "lane", "wave16", "wave64", "group", "hub_chunk", "finish", "finish_push", "mass")
     for t in ("one trip", "second trip")] +
    ["wave16: last wave partly idle", "wave64: last workgroup partly idle",
     "hub: in-degree chunk + 1", "hub: in-degree an exact multiple of the chunk", "hub: in-degree of several chunks otherwise",
     "hub: in-degree within one chunk", "hub: in-degree 0", "hubs: two of several chunks", "hub: dangling", "hub: self-loop",
     "lanes: 16", "lanes: 64", "lanes: mean exactly 32", "lanes: mean just above 32",
     "push: aligned col_idx", "push: unaligned col_idx"])


def cells(rp, ci, n, min_class, method, col_shift=0):
    """the kernel edges of csrc/pagerank.hip that one iteration on this input reaches, as a subset of CELLS.  col_shift: the
    ints by which A's col_idx is off 16-byte alignment (PUSH reads it four entries at a time where it is aligned)"""
    if n == 0:
        return set()
    out = {_trips("init", n, THREADS), _trips("mass", n, THREADS)}
    if method == PR_PUSH:
        out.add(_trips("finish_push", n, THREADS))
        if edges(rp, ci, n)[0].size:
            out.add("push: unaligned col_idx" if col_shift % 4 else "push: aligned col_idx")
        return out
    src, dst = edges(rp, ci, n)
    d, cls = _classes(rp, ci, n, min_class)
    size = np.bincount(cls, minlength=4).tolist()
    if size[0]:
        out.add(_trips("lane", size[0], THREADS))
    if size[1]:
        entries, lanes = int(d[cls == 1].sum()), wave_lanes(rp, ci, n, min_class)
        out.add("lanes: %d" % lanes)
        if entries == LANES_MEAN * size[1]:
            out.add("lanes: mean exactly 32")
        if entries == LANES_MEAN * size[1] + 1:
            out.add("lanes: mean just above 32")
        if lanes == 16:                                      # four rows per wave, sixteen per workgroup
            out.add(_trips("wave16", size[1], WAVES * 4))
            if size[1] % 4:
                out.add("wave16: last wave partly idle")
        else:                                                # a row per wave, four per workgroup
            out.add(_trips("wave64", size[1], WAVES))
            if size[1] % WAVES:
                out.add("wave64: last workgroup partly idle")
    if size[2]:
        out.add(_trips("group", size[2], 1))
    if size[3]:
        hubs = np.flatnonzero(cls == 3)
        chunks = hub_chunks(rp, ci, n, min_class)
        assert chunks == int(((d[hubs] + HUB_CHUNK - 1) // HUB_CHUNK).sum())
        if chunks:
            out.add(_trips("hub_chunk", chunks, 1))
        out.add(_trips("finish", size[3], THREADS))
        dh = d[hubs]
        several = dh > HUB_CHUNK
        for cell, hit in (("hub: in-degree 0", dh == 0), ("hub: in-degree within one chunk", (dh > 0) & ~several),
                          ("hub: in-degree chunk + 1", dh == HUB_CHUNK + 1),
                          ("hub: in-degree an exact multiple of the chunk", several & (dh % HUB_CHUNK == 0)),
                          ("hub: in-degree of several chunks otherwise", several & (dh != HUB_CHUNK + 1) & (dh % HUB_CHUNK != 0))):
            if hit.any():
                out.add(cell)
        if several.sum() >= 2:
            out.add("hubs: two of several chunks")
        big = hubs[several]
        if (np.bincount(src, minlength=n)[big] == 0).any():
            out.add("hub: dangling")
        if np.isin(src[src == dst], big).any():
            out.add("hub: self-loop")
    assert out <= CELLS
    return out


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


# ---------------------------------------------------------------- the edge graphs (tests/test_gpu_pagerank_edges.py) --
# Kept out of GRAPHS: the parametrised tests and the naive models that go over GRAPHS would become slow.  The builders take
# the sizes that the kernels' constants set as parameters, so that a scaled-down twin has the same structure.
def hubs_graph(chunk=HUB_CHUNK):
    """four hubs, the vertices 0 .. 3, with in-degrees chunk + 1, 2 * chunk, 2 * chunk + 1 and 3 * chunk, fed by overlapping
    ranges of the feeders 4 .. n - 2.  Hub 0 is dangling, hub 3 has a self-loop (one of its 3 * chunk entries), hubs 1 and 2
    point at a few feeders; the last vertex, fed by every sixth feeder, is one for a whole workgroup.  A feeder also points
    at 0 .. 2 other feeders, every sixteenth at up to 400 of them, so the feeders' out-degrees run from 1 to over 400 and
    the c(u) that one chunk sums differ by two orders of magnitude."""
    S = 3 * chunk + chunk // 4
    i = np.arange(S)
    member = [(0, chunk + 1), (chunk // 2, chunk // 2 + 2 * chunk), (chunk, 3 * chunk + 1), (S - (3 * chunk - 1), S)]
    sixth = 4 + i[::6]
    rows = [4 + i[a:b] for a, b in member] + [[3], [1, 1, 2], sixth, [S + 4]]
    cols = [np.full(b - a, h) for h, (a, b) in enumerate(member)] + [[3], [4, 4 + S - 1, 4 + S // 2], np.full(sixth.size, S + 4), [11]]
    extra = np.where(i % 16 == 0, 1 + (i * 37) % 400, i % 3)
    extra = np.minimum(extra, S - 1)
    at = np.arange(int(extra.sum())) - np.repeat(np.cumsum(extra) - extra, extra)
    rows.append(4 + np.repeat(i, extra))
    cols.append(4 + (np.repeat(i * 7 + 1, extra) + at) % S)
    return canonical(*cc_ref.csr(np.concatenate(rows), np.concatenate(cols), S + 5))


def wide_graph(lane=THREADS * MAX_BLOCKS + 300, wave=16 * MAX_BLOCKS + 17):
    """`lane` vertices of in-degree 0 .. 2 and behind them `wave` vertices of in-degree 9 or 10: with the defaults more
    lane-class vertices than one trip of k_pr_lane (and of init, finish and mass) covers, more wave-class vertices than
    one trip of k_pr_wave<16> covers, at a mean in-degree under 32, and a wave-class size that is no multiple of four.  The
    lane vertices that feed nothing and are no multiple of eight are dangling, and so is every fifth wave-class vertex: a
    vertex that a kernel finished twice would count twice in the next dangling sum."""
    k = np.arange(wave)
    deg = 9 + k % 2
    at = np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
    i8 = np.arange(0, lane, 8)
    k5 = k[k % 5 != 0]                                       # (every fifth wave-class vertex is dangling too)
    rows = [(np.repeat(k * 11, deg) + 3 * at) % lane, np.repeat(lane + k5, 3), i8]
    cols = [lane + np.repeat(k, deg), (np.repeat(k5 * 16, 3) + np.tile(np.arange(3), k5.size)) % lane, (i8 * 5 + 1) % lane]
    return canonical(*cc_ref.csr(np.concatenate(rows), np.concatenate(cols), lane + wave))


def wave64_graph(wave=WAVES * MAX_BLOCKS + 5, feeders=3001, deg=40):
    """`wave` vertices of in-degree `deg` behind `feeders` vertices of in-degree 2 .. 3: with the defaults more wave-class
    vertices than one trip of k_pr_wave<64> covers, at a mean in-degree over 32, their number no multiple of four"""
    k = np.arange(wave)
    rows = [(np.repeat(k * 7, deg) + 13 * np.tile(np.arange(deg), wave)) % feeders, feeders + k]
    cols = [feeders + np.repeat(k, deg), k % feeders]
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), feeders + wave)


def lanes_graph(extra, mean=LANES_MEAN, size=5):
    """`size` wave-class vertices behind 40 + extra feeders: in-degree `mean` each, the last one `mean + extra`: the wave
    class holds exactly mean * size + extra entries"""
    m = 40 + extra
    rows = [(k + np.arange(mean + (extra if k == size - 1 else 0))) % m for k in range(size)] + [m + np.arange(size)]
    cols = [np.full(r.size, m + k) for k, r in enumerate(rows[:-1])] + [np.arange(size)]
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), m + size)


EDGE_GRAPHS = {
    "hubs": hubs_graph,
    "wide": wide_graph,
    "wave64": wave64_graph,
    "lanes_at_32": lambda: lanes_graph(0),
    "lanes_above_32": lambda: lanes_graph(1),
}
EDGE_ITERATIONS = {"hubs": 20, "wide": 3, "wave64": 3, "lanes_at_32": 20, "lanes_above_32": 20}   # what the model runs
EDGE_MIN_CLASSES = {"hubs": (0, 1, 2, 3), "wide": (0, 1, 2, 3), "wave64": (0, 1, 2, 3), "lanes_at_32": (0,), "lanes_above_32": (0,)}


def source_constants():
    """the constants above read from csrc/pagerank.hip, under the names above (a CPU test compares the two)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "binary-spgemm_amd", "csrc", "pagerank.hip")) as f:
        src = f.read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert "constexpr int kPrWaves = kPrThreads / 64;" in src
    assert "std::max(1ll, std::min(blocks, (long long)kPrMaxBlocks))" in src and "(items + per_block - 1) / per_block" in src
    for launch in ("k_pr_init, pr_grid(n, kPrThreads)", "k_pr_lane, pr_grid(h.size[0], kPrThreads)",
                   "k_pr_wave<16>, pr_grid(h.size[1], kPrWaves * 4)", "k_pr_wave<64>, pr_grid(h.size[1], kPrWaves)",
                   "k_pr_group, pr_grid(h.size[2], 1)", "k_pr_hub_chunk, pr_grid(h.chunks, 1)",
                   "k_pr_finish, pr_grid(h.size[3], kPrThreads)", "k_pr_finish, pr_grid(n, kPrThreads)",
                   "k_pr_mass, pr_grid(n, kPrThreads)"):
        assert launch in src, launch
    return {"LANE_CAP": const("kPrLaneCap"), "WAVE_CAP": const("kPrWaveCap"), "GROUP_CAP": const("kPrGroupCap"),
            "HUB_CHUNK": const("kPrHubChunk"), "THREADS": const("kPrThreads"), "MAX_BLOCKS": const("kPrMaxBlocks"),
            "LANES_MEAN": int(re.search(r"h\.wave_entries <= (\d+)ull \* \(u64\)h\.size\[1\]\) wave_lanes = 16;", src).group(1))}

_cache = {}


def graph(name):
    """the named graph, built once"""
    if name not in _cache:
        rp, ci, n = (EDGE_GRAPHS[name] if name in EDGE_GRAPHS else GRAPHS[name])()
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
