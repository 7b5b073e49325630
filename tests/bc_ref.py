"""The reference of the betweenness tests (bspgemm_betweenness): the numpy model of the header's definition (exact uint64 path
counts, 2^32-scaled integer dependencies, the two double operations as numpy does them), which also predicts every field of
bspgemm_bc_info; a naive model in Python integers and floats to check it with; networkx's Brandes in float64 to measure the
deviation against; a host model of the edges of the hub code that a call reaches (cells); and the graphs the tests use.
Nothing here touches the GPU.
"""
import math
import zlib

import numpy as np

import cc_ref
import gen
import pagerank_ref as P

HUB_CHUNK = 4096         # csrc/betweenness.hip kBcHubChunk: the longest row left to one group of lanes, and the chunk size
ONE = 1 << 32
U = np.uint64
M32 = U(0xFFFFFFFF)
S32 = U(32)
LANES = (0, 4, 16, 64)   # BSPGEMM_OPT_BC_LANES

edges, canonical, is_canonical = P.edges, P.canonical, P.is_canonical


class Overflow(Exception):
    """a path count of 2^63 or more: what BSPGEMM_ERR_OVERFLOW reports"""

    def __init__(self, index, level):
        Exception.__init__(self, "sources[%d], level %d" % (index, level))
        self.index, self.level = index, level


def _rows(crp, cci, F):
    """(src, dst) int64 of the entries of the rows F of a canonical CSR, row after row"""
    lens = (crp[F + 1] - crp[F]).astype(np.int64)
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.cumsum(lens) - lens
    idx = np.arange(total) - np.repeat(first, lens) + np.repeat(crp[F].astype(np.int64), lens)
    return np.repeat(np.asarray(F, np.int64), lens), cci[idx].astype(np.int64)


def model(rp, ci, n, sources, trace=None):
    """{"fixed", "bc", and every field of bspgemm_bc_info} of the definition; raises Overflow.  trace: a list that takes,
    per source, {"fronts", "level", "sigma", "delta"} as the sweep left them (cells() reads them)"""
    crp, cci, _ = canonical(rp, ci, n)
    crp = np.asarray(crp, np.int64)
    outdeg = np.diff(crp)
    chunks_of = np.where(outdeg > HUB_CHUNK, (outdeg + HUB_CHUNK - 1) // HUB_CHUNK, 0)
    bc = np.zeros(n, U)
    info = {"sigma_max": 0, "reached": 0, "edges_forward": 0, "hub_chunks": 0, "sources": len(sources), "depth_max": 0,
            "levels": 0, "canonicalised": 0 if is_canonical(rp, ci, n) else 1}
    if n == 0:
        info["canonicalised"] = 0
    for index, s in enumerate(int(x) for x in sources):
        level = np.full(n, -1, np.int64)
        sigma = np.zeros(n, U)
        level[s], sigma[s] = 0, 1
        fronts = [np.array([s], np.int64)]
        while True:                                          # a forward launch per level that has entries to walk
            F, d = fronts[-1], len(fronts)
            es, ed = _rows(crp, cci, F)
            if es.size == 0:
                break
            info["levels"] += 1
            info["edges_forward"] += int(es.size)
            info["hub_chunks"] += int(chunks_of[F].sum())
            new = np.unique(ed[level[ed] == -1])
            if new.size == 0:
                break
            level[new] = d
            into = level[ed] == d
            su = sigma[es[into]]
            hi, lo = np.zeros(n, U), np.zeros(n, U)           # the sums in two halves: no wrap, whatever they come to
            np.add.at(hi, ed[into], su >> S32)
            np.add.at(lo, ed[into], su & M32)
            top = hi + (lo >> S32)
            if int(top.max()) >= 1 << 31:                    # sigma >= 2^63
                raise Overflow(index, d)
            sigma[new] = (top[new] << S32) | (lo[new] & M32)
            fronts.append(new)
        depth = len(fronts) - 1
        delta, c = np.zeros(n, U), np.zeros(n, np.float64)
        for d in range(depth, -1, -1):
            F = fronts[d]
            if d < depth:
                es, ed = _rows(crp, cci, F)
                down = level[ed] == d + 1
                summand = np.floor(c[ed[down]] * sigma[es[down]].astype(np.float64)).astype(U)
                np.add.at(delta, es[down], summand)
                info["hub_chunks"] += int(chunks_of[F].sum())
            c[F] = (U(ONE) + delta[F]).astype(np.float64) / sigma[F].astype(np.float64)
        if trace is not None:
            trace.append({"fronts": fronts, "level": level, "sigma": sigma, "delta": delta.copy()})
        delta[s] = 0
        bc += delta
        info["sigma_max"] = max(info["sigma_max"], int(sigma.max()))
        info["reached"] += int(sum(F.size for F in fronts))
        info["depth_max"] = max(info["depth_max"], depth)
    info["fixed"], info["bc"] = bc, to_double(bc)
    return info


def to_double(bc):
    return np.asarray(bc, U).astype(np.float64) * 2.0 ** -32


def naive(rp, ci, n, sources):
    """bc as a list of Python ints from the definition, vertex by vertex; raises Overflow"""
    rp, ci = np.asarray(rp).tolist(), np.asarray(ci).tolist()
    out = [sorted(set(ci[rp[u]:rp[u + 1]])) for u in range(n)]
    bc = [0] * n
    for index, s in enumerate(int(x) for x in sources):
        level, sigma, order = {s: 0}, {s: 1}, [[s]]
        while True:
            nxt, d = [], len(order)
            for u in order[-1]:
                for w in out[u]:
                    if w not in level:
                        level[w], sigma[w] = d, 0
                        nxt.append(w)
                    if level[w] == d:
                        sigma[w] += sigma[u]
            if not nxt:
                break
            if any(sigma[w] >= 1 << 63 for w in nxt):
                raise Overflow(index, d)
            order.append(nxt)
        delta, c = {}, {}
        for vs in reversed(order):
            for v in vs:
                total = 0
                for w in out[v]:
                    if level[w] == level[v] + 1:
                        total += int(math.floor(c[w] * float(sigma[v])))
                delta[v] = total
                c[v] = float(ONE + total) / float(sigma[v])
        for v in level:
            if v != s:
                bc[v] += delta[v]
    return bc


# ---------------------------------------------------------------- the kernel edges ("cells") an input reaches ---------
THREADS = 256            # csrc/betweenness.hip kBcThreads: k_bc_source writes that many chunk records per trip

CELLS = frozenset([
    "source is a hub", "source hub of more than 256 records", "two hubs in one level", "hub level with a non-zero chunk offset",
    "hub length chunk + 1", "hub length an exact multiple of the chunk", "hub length otherwise", "hub in the last level",
    "hub with a self-loop", "hub entry to the source", "hub entry to an earlier level", "hub entry to the same level",
    "hub with backward sum 0", "hub reached from two sources in a row", "stored row over the chunk, distinct row not",
    "stored and distinct row over the chunk", "hub successor with sigma > 1 fed from two chunks"])


def cells(rp, ci, n, sources, chunk=HUB_CHUNK):
    """the edges of csrc/betweenness.hip's hub code that the sweeps from `sources` reach, as a subset of CELLS: read off the
    model's own fronts.  A hub is a reached vertex whose canonical row is longer than `chunk`; its records lie in chunk[]
    behind those of the levels before it (BcLevelRec::coff)."""
    rp = np.asarray(rp, np.int64)
    crp, cci, _ = canonical(rp, ci, n)
    crp = np.asarray(crp, np.int64)
    stored, outdeg = np.diff(rp), np.diff(crp)
    hub = outdeg > chunk
    records = np.where(hub, (outdeg + chunk - 1) // chunk, 0)
    trace, out, before = [], set(), None
    model(rp, ci, n, sources, trace)
    for s, t in zip((int(x) for x in sources), trace):
        fronts, level, sigma, delta = t["fronts"], t["level"], t["sigma"], t["delta"]
        depth, coff, mine = len(fronts) - 1, 0, set()
        if hub[s]:
            out.add("source is a hub")
            if records[s] > THREADS:
                out.add("source hub of more than 256 records")
        for d, F in enumerate(fronts):
            H = F[hub[F]]
            if ((stored[F] > chunk) & ~hub[F]).any():
                out.add("stored row over the chunk, distinct row not")
            if (stored[H] != outdeg[H]).any():
                out.add("stored and distinct row over the chunk")
            if H.size == 0:
                continue
            if H.size >= 2:
                out.add("two hubs in one level")
            if coff > 0:
                out.add("hub level with a non-zero chunk offset")
            coff += int(records[H].sum())
            mine.update(H.tolist())
            for cell, hit in (("hub length chunk + 1", outdeg[H] == chunk + 1),
                              ("hub length an exact multiple of the chunk", outdeg[H] % chunk == 0),
                              ("hub length otherwise", (outdeg[H] != chunk + 1) & (outdeg[H] % chunk != 0))):
                if hit.any():
                    out.add(cell)
            if d == depth:
                out.add("hub in the last level")
            elif (delta[H] == 0).any():
                out.add("hub with backward sum 0")
            es, ed = _rows(crp, cci, H)
            lw = level[ed]
            for cell, hit in (("hub with a self-loop", ed == es), ("hub entry to the source", (ed == s) & (es != s)),
                              ("hub entry to an earlier level", (lw >= 0) & (lw < d) & (ed != s)),
                              ("hub entry to the same level", (lw == d) & (ed != es))):
                if hit.any():
                    out.add(cell)
            # the successors one level down that two different chunks add to (of one hub or of two)
            lens = outdeg[H]
            record = (np.arange(es.size) - np.repeat(np.cumsum(lens) - lens, lens)) // chunk + \
                np.repeat(np.cumsum(records[H]) - records[H], lens)
            down = lw == d + 1
            fed = np.unique(ed[down] * int(records[H].sum()) + record[down]) // int(records[H].sum())
            w, times = np.unique(fed, return_counts=True)
            if (sigma[w[times >= 2]] > U(1)).any():
                out.add("hub successor with sigma > 1 fed from two chunks")
        if before is not None and before & mine:
            out.add("hub reached from two sources in a row")
        before = mine
    assert out <= CELLS
    return out


def symmetric(rp, ci, n):
    src, dst = edges(rp, ci, n)
    return np.array_equal(np.sort(src * n + dst), np.sort(dst * n + src))


def networkx_bc(rp, ci, n, sources):
    """networkx's unnormalised Brandes (float64) restricted to the distinct `sources`: on the directed graph, or, for a
    symmetric pattern, on the undirected graph times two"""
    import networkx as nx
    src, dst = edges(rp, ci, n)
    und = symmetric(rp, ci, n)
    G = nx.Graph() if und else nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(src.tolist(), dst.tolist()))
    sources = sorted(set(int(x) for x in sources))
    if len(sources) == n:
        got = nx.betweenness_centrality(G, normalized=False, endpoints=False)
    else:
        got = nx.betweenness_centrality_subset(G, sources, list(range(n)), normalized=False)
    return np.array([got[v] for v in range(n)], np.float64) * (2.0 if und else 1.0)


# ---------------------------------------------------------------- graphs ---------------------------------------------
def _pairs(pairs, n):
    return cc_ref.csr([p[0] for p in pairs], [p[1] for p in pairs], n)


def _empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), n


def _both(rows, cols, n):
    """every pair in both directions, in canonical form"""
    rows, cols = np.asarray(rows), np.asarray(cols)
    return canonical(*cc_ref.csr(np.concatenate([rows, cols]), np.concatenate([cols, rows]), n))


def star_in(n=50):
    """leaves 1 .. n - 2 -> hub 0 -> tail n - 1: the hub lies on every leaf's path to the tail"""
    leaves = np.arange(1, n - 1)
    return cc_ref.csr(np.concatenate([leaves, [0]]), np.concatenate([np.zeros(n - 2, np.int64), [n - 1]]), n)


def disconnected():
    """a directed triangle, a path of four, an edge, and 11 isolated vertices: most sources reach little"""
    return _pairs([(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 6), (7, 8)], 20)


def diamond_ladder(rungs=12):
    """0 -> {1, 2} -> 3 -> {4, 5} -> 6 ...: sigma doubles per rung, every ratio is dyadic"""
    pairs = []
    for r in range(rungs):
        a = 3 * r
        pairs += [(a, a + 1), (a, a + 2), (a + 1, a + 3), (a + 2, a + 3)]
    return _pairs(pairs, 3 * rungs + 1)


def layers(widths):
    """source 0 -> complete bipartite layers of the given widths -> one sink: sigma(sink) = the product of the widths, at
    level len(widths) + 1"""
    rows, cols, prev, at = [], [], np.array([0]), 1
    for w in list(widths) + [1]:
        cur = np.arange(at, at + w)
        rows.append(np.repeat(prev, w))
        cols.append(np.tile(cur, prev.size))
        prev, at = cur, at + w
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), at)


def hub(K):
    """root 0 -> {hub 1, side 2}; the hub's row has exactly K entries, the leaves 3 .. K + 2; the side vertex points at
    every fifth leaf (sigma 2 there); every leaf -> K + 3 -> K + 4 -> root: the hub is in a frontier from every source, with
    successors beyond it"""
    leaves = np.arange(3, K + 3)
    rows = [[0, 0], np.full(K, 1), np.full(leaves[::5].size, 2), leaves, [K + 3, K + 4]]
    cols = [[1, 2], leaves, leaves[::5], np.full(K, K + 3), [K + 4, 0]]
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), K + 5)


def grid(k):
    i = np.arange(k * k).reshape(k, k)
    return _both(np.concatenate([i[:, :-1].ravel(), i[:-1, :].ravel()]), np.concatenate([i[:, 1:].ravel(), i[1:, :].ravel()]), k * k)


def from_networkx(G, directed):
    n = G.number_of_nodes()
    e = np.array(list(G.edges()), np.int64).reshape(-1, 2)
    return cc_ref.csr(e[:, 0], e[:, 1], n) if directed else _both(e[:, 0], e[:, 1], n)


GRAPHS = {
    "empty0": lambda: _empty(0),
    "empty1": lambda: _empty(1),
    "loop1": lambda: _pairs([(0, 0)], 1),
    "two_cycle": lambda: _pairs([(0, 1), (1, 0)], 2),
    "path5": lambda: _both(np.arange(4), np.arange(1, 5), 5),
    "dipath6": lambda: cc_ref.path(6),
    "star_in": star_in,
    "star_out": lambda: cc_ref.star(50, 0),
    "self_loops": P.self_loops_graph,
    "dups_unsorted": lambda: gen.dups_unsorted(300, 6, 5904),
    "untidy": lambda: P.lcc_ref.untidy(150, 2200, 5905),
    "disconnected": disconnected,
    "diamond_ladder": diamond_ladder,
    "layers_2p62": lambda: layers([8] * 20 + [4]),
    "layers_3p39": lambda: layers([3] * 39),
    "hub_4095": lambda: hub(HUB_CHUNK - 1),
    "hub_4096": lambda: hub(HUB_CHUNK),
    "hub_4097": lambda: hub(HUB_CHUNK + 1),
    "hub_chunks": lambda: hub(3 * HUB_CHUNK + 1),
    "n_4097": P.n_4097,
    "rmat11": P.rmat11_cut,
    "symmetric_rmat9": P.symmetric_rmat9,
}
# sigma reaches 2^63: (widths, the level at which the call refuses)
REFUSED = {
    "layers_2p63": ([8] * 21, 22),
    "layers_meet": ([8] * 20 + [4, 2, 1], 23),
    "layers_2p64": ([8] * 21 + [2], 22),
}
SMALL = ("empty0", "empty1", "loop1", "two_cycle", "path5", "dipath6", "star_in", "star_out", "self_loops", "disconnected",
         "diamond_ladder", "untidy", "layers_2p62", "layers_3p39")
ALL_SOURCES_UP_TO = 600


# ---------------------------------------------------------------- the edge graphs (tests/test_gpu_bc_edges.py) -------
# Kept out of GRAPHS: the parametrised tests and the naive model that go over GRAPHS would become slow.  The builders take
# the chunk as a parameter, so that a twin with a chunk of 16 has the same structure at a size the naive model walks.
def hub_levels(chunk=HUB_CHUNK):
    """Hubs in four levels of the sweep from vertex 0, in canonical form:
        0 -> 1, 2, 3        rows of chunk + 1, 2 * chunk (two full chunks) and chunk entries (no hub) over 5 * chunk / 2
                            leaves (the vertices 4 ...): the ranges overlap, so leaves have sigma 2 and 3, also where two
                            chunks of different hubs add to them
        three leaves -> g   the second-generation hub, 2 * chunk + 1 entries: itself, the source, vertex 2 (level 1), p (its
                            own level; a fourth leaf -> p), and 2 * chunk - 3 fresh vertices.  Its records lie behind the
                            four of vertices 1 and 2.
        fresh: X, Y         X: chunk + 1 entries, all leaves (two levels up): a hub whose sum is 0, not in the last level,
        Y -> Z              Z: chunk + 1 entries, all leaves: a hub in the last level whose forward chunks find nothing
    (g, p, X, Y, Z are what hub_levels_names returns.)  From vertex 2 the source is a hub; from the first leaf, g is alone in
    level 1 and vertices 2 and X share level 2."""
    C = chunk
    leaves = 4 + np.arange(5 * C // 2)
    g, p, fresh, X, Y, Z = hub_levels_names(C)
    pairs = [([0, 0, 0], [1, 2, 3]), (np.full(C + 1, 1), leaves[:C + 1]), (np.full(2 * C, 2), leaves[C // 2:C // 2 + 2 * C]),
             (np.full(C, 3), leaves[C:2 * C]), (leaves[[0, C, -1]], [g, g, g]), ([leaves[1]], [p]),
             (np.full(4 + fresh.size, g), np.concatenate([[g, 0, 2, p], fresh])), ([p], [fresh[0]]),
             (np.full(C + 1, X), leaves[:C + 1]), ([Y], [Z]), (np.full(C + 1, Z), leaves[C - 1:2 * C])]
    return canonical(*cc_ref.csr(np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs]), Z + 1))


def hub_levels_names(chunk=HUB_CHUNK):
    """(g, p, the fresh vertices, X, Y, Z) of hub_levels"""
    g = 4 + 5 * chunk // 2
    fresh = g + 2 + np.arange(2 * chunk - 3)
    return g, g + 1, fresh, int(fresh[1]), int(fresh[2]), int(fresh[-1]) + 1


def hub_levels_sources(chunk=HUB_CHUNK):
    """vertex 0, a first-generation hub, a leaf, and the same hub again"""
    return np.array([0, 2, 4, 2], np.int32)


def hub_stored(stored, distinct):
    """hub(distinct) with the hub's row stored `stored` entries long: its entries in descending order, again and again"""
    rp, ci, n = hub(distinct)
    row = np.resize(ci[rp[1]:rp[2]][::-1], stored)
    rp = rp.copy()
    rp[2:] += stored - distinct
    return rp, np.concatenate([ci[:rp[1]], row, ci[rp[1] + distinct:]]).astype(np.int32), n


EDGE_GRAPHS = {
    "hub_levels": hub_levels,
    "hub_258_records": lambda: hub((THREADS + 1) * HUB_CHUNK + 1),
    "stored_5000_of_4000": lambda: hub_stored(5000, 4000),
    "stored_9000_of_4097": lambda: hub_stored(9000, 4097),
}
EDGE_SOURCES = {
    "hub_levels": hub_levels_sources(),
    "hub_258_records": np.array([1, 0], np.int32),
    "stored_5000_of_4000": np.array([0, 1, 3], np.int32),
    "stored_9000_of_4097": np.array([0, 1, 3], np.int32),
}

_cache = {}


def graph(name):
    """the named graph, built once"""
    if name not in _cache:
        rp, ci, n = layers(REFUSED[name][0]) if name in REFUSED else (EDGE_GRAPHS[name] if name in EDGE_GRAPHS else GRAPHS[name])()
        rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        rp.setflags(write=False)
        ci.setflags(write=False)
        _cache[name] = (rp, ci, n)
    return _cache[name]


def sources_of(name):
    """every vertex where n <= 600, else 8 seeded sources and the first of them once more"""
    n = graph(name)[2]
    if n <= ALL_SOURCES_UP_TO:
        return np.arange(n, dtype=np.int32)
    s = np.random.default_rng(zlib.crc32(name.encode())).integers(0, n, 8)
    return np.concatenate([s, s[:1]]).astype(np.int32)


def expected(name):
    """the model on the named graph from sources_of(name), computed once and shared (read-only)"""
    key = ("model", name)
    if key not in _cache:
        res = model(*graph(name), sources_of(name))
        res["fixed"].setflags(write=False)
        res["bc"].setflags(write=False)
        _cache[key] = res
    return _cache[key]


def edge_expected(name, backwards=False):
    """(sources, the model) of an edge graph from EDGE_SOURCES[name], in the given or the opposite order, computed once
    and shared (read-only)"""
    key = ("edge", name, backwards)
    if key not in _cache:
        sources = np.ascontiguousarray(EDGE_SOURCES[name][::-1] if backwards else EDGE_SOURCES[name])
        res = model(*graph(name), sources)
        res["fixed"].setflags(write=False)
        res["bc"].setflags(write=False)
        _cache[key] = (sources, res)
    return _cache[key]


def edge_cells(name):
    """cells() of an edge graph from EDGE_SOURCES[name], computed once"""
    key = ("cells", name)
    if key not in _cache:
        _cache[key] = frozenset(cells(*graph(name), EDGE_SOURCES[name]))
    return _cache[key]


def cli_sources(n, k, seed):
    """SpGEMM_hip_bc --sources k --seed seed"""
    x, out = seed, []
    for _ in range(k):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out.append((x >> 33) % n)
    return np.array(out, np.int32)
