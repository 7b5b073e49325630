"""The reference of the BFS-tree tests (bspgemm_bfs_tree): a level-synchronous numpy search with the smallest-parent rule,
a host model of the direction rule of include/bspgemm.h, the tree check, and the small graphs the tests walk.  Nothing here
touches the GPU.
"""
import functools

import numpy as np

import bfs_ref
import cc_ref
import gen
import kcore_ref

K_PULL_LIGHT = 32        # csrc/bfs_tree.hip kBfsPullLight: entries of its own in-row that a lane of k_bfs_pull walks
INT_MAX = 2**31 - 1


def _rows_of(rp, ci, f):
    """(u, v) of every stored entry in the rows of the vertices f, as two arrays"""
    rp = np.asarray(rp, np.int64)
    lens = rp[f + 1] - rp[f]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    starts = np.repeat(rp[f] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return np.repeat(f, lens), np.asarray(ci)[starts + np.arange(total)].astype(np.int64)


def search(rp, ci, n, source, max_depth=0):
    """(level int32[n], parent int32[n], frontiers): level -1 and parent -1 where unreached; parent(v) = the smallest u one
    level up with (u, v) stored; the source is its own parent.  frontiers[k] = (n_f, m_f) of the frontier that level k + 1
    was produced from -- its size and its stored out-degree sum -- for every level that was attempted, the last, empty one
    included when the search ended by itself."""
    deg = np.diff(np.asarray(rp, np.int64))
    level = np.full(n, -1, np.int32)
    parent = np.full(n, -1, np.int32)
    level[source] = 0
    parent[source] = source
    f = np.array([source], np.int64)
    frontiers = []
    d = 0
    while f.size and (max_depth <= 0 or d < max_depth):
        d += 1
        frontiers.append((int(f.size), int(deg[f].sum())))
        u, v = _rows_of(rp, ci, f)
        new = level[v] < 0
        u, v = u[new], v[new]
        best = np.full(n, INT_MAX, np.int64)
        np.minimum.at(best, v, u)
        f = np.flatnonzero(best != INT_MAX)
        level[f] = d
        parent[f] = best[f]
    return level, parent, frontiers, int(f.size)


def tree_csr(level, parent):
    """(row_ptr int64, col_idx int32, values int32) of the result object: one entry (v, parent(v)) = level(v) per reached v"""
    reached = level >= 0
    rp = np.concatenate([[0], np.cumsum(reached)]).astype(np.int64)
    return rp, parent[reached].astype(np.int32), level[reached].astype(np.int32)


def bfs_tree(rp, ci, n, source, max_depth=0):
    """(row_ptr int64, parents, levels) of what bspgemm_bfs_tree returns"""
    level, parent, _, _ = search(rp, ci, n, source, max_depth)
    return tree_csr(level, parent)


def model(rp, ci, n, source, direction="auto", alpha=15, beta=18, max_depth=0):
    """what bspgemm_bfs_tree_info holds, from the rule of the header: the search starts in PUSH; in PUSH it switches to PULL
    when m_f * alpha > m_u and n_f > the previous level's n_f (0 before level 1); in PULL it switches to PUSH when
    n_f * beta < n.  m_u = nnz(A) - the out-degrees of every vertex reached so far, the frontier included."""
    level, parent, frontiers, left = search(rp, ci, n, source, max_depth)
    nnz = int(np.asarray(rp)[n]) - int(np.asarray(rp)[0])
    pulling = direction == "pull"
    m_u, prev, mask, pushes, pulls, pushed = nnz, 0, 0, 0, 0, 0
    for d, (n_f, m_f) in enumerate(frontiers, start=1):
        m_u -= m_f
        if direction == "auto":
            if not pulling:
                pulling = m_f * alpha > m_u and n_f > prev
            else:
                pulling = not n_f * beta < n
        if pulling:
            pulls += 1
            if d <= 64:
                mask |= 1 << (d - 1)
        else:
            pushes += 1
            pushed += m_f
        prev = n_f
    return {"reached": int((level >= 0).sum()), "edges_pushed": pushed, "pull_mask": mask, "depth": int(level.max()),
            "complete": int(left == 0), "push_levels": pushes, "pull_levels": pulls}


def tree_check(rp, ci, n, source, t_rp, t_parent, t_level):
    """asserts that the downloaded tree is a BFS tree of the graph: one entry per reached row, level(parent(v)) ==
    level(v) - 1 with the edge (parent(v), v) stored, the source its own parent at level 0, and no stored edge out of a
    reached vertex that ends at an unreached one or more than one level further down"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    lens = np.diff(t_rp)
    assert t_rp.size == n + 1 and ((lens == 0) | (lens == 1)).all()
    level = np.full(n, -1, np.int64)
    parent = np.full(n, -1, np.int64)
    reached = np.flatnonzero(lens)
    level[reached] = t_level
    parent[reached] = t_parent
    assert level[source] == 0 and parent[source] == source and int((level == 0).sum()) == 1
    others = reached[reached != source]
    assert (parent[others] >= 0).all() and (parent[others] < n).all()
    assert (level[parent[others]] == level[others] - 1).all()
    rows = np.repeat(np.arange(n), np.diff(rp))
    stored = set(zip(rows.tolist(), ci.tolist()))
    assert all((int(parent[v]), int(v)) in stored for v in others)
    from_reached = level[rows] >= 0
    assert (level[ci[from_reached]] >= 0).all()
    assert (level[ci[from_reached]] <= level[rows[from_reached]] + 1).all()


# ---------------------------------------------------------------- graphs ---------------------------------------------
def star_out(m):
    """the hub 0 -> m leaves: one group walks a row of m entries and appends m vertices"""
    return cc_ref.csr(np.zeros(m, np.int64), 1 + np.arange(m), m + 1) + (0,)


def star_in(m):
    """0 -> m leaves -> the hub m + 1: m frontier vertices with one atomicMin address; parent(hub) = 1, the smallest leaf"""
    leaves = 1 + np.arange(m)
    rows = np.concatenate([np.zeros(m, np.int64), leaves])
    cols = np.concatenate([leaves, np.full(m, m + 1)])
    return cc_ref.csr(rows, cols, m + 2) + (0,)


def rows_around(W, seed):
    """0 -> 12 vertices whose rows hold W - 1, W, W + 1, W - 1, ... entries, drawn from a pool of 3 W shared targets in
    shuffled order: the groups of one wave of k_bfs_push<W> have unequal trip counts, and most targets have several
    candidate parents"""
    rng = np.random.default_rng(seed)
    mids = 1 + np.arange(12)
    pool = 13 + np.arange(3 * W)
    rows, cols = [np.zeros(12, np.int64)], [mids]
    for i, u in enumerate(mids):
        rows.append(np.full(W - 1 + i % 3, u))
        cols.append(rng.choice(pool, size=W - 1 + i % 3, replace=False))
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), 13 + 3 * W) + (0,)


def in_row(L, where):
    """0 -> a, and the vertex t = L + 2 with the in-neighbours 1 .. L, of which only a can be reached: a = 1 ("first"),
    a = L ("last"), or a = L + 1, which is not among them ("absent": t has L in-edges and stays unreached)"""
    a = {"first": 1, "last": L, "absent": L + 1}[where]
    rows = np.concatenate([[0], 1 + np.arange(L)])
    cols = np.concatenate([[a], np.full(L, L + 2)])
    return cc_ref.csr(rows, cols, L + 3) + (0,)


def sparse_random(n, seed):
    """2 n random directed edges and the chain 0 -> 1 -> ... -> 9: from 0 the search reaches a part of the graph whose
    ids are spread over every 64-entry flag word of the read-out"""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, size=(2, 2 * n))
    return cc_ref.csr(np.concatenate([np.arange(9), r]), np.concatenate([1 + np.arange(9), c]), n) + (0,)


def layered(seed):
    rp, ci, n, ids = bfs_ref.layered([1, 6, 40, 300, 700, 150, 20], 60, seed)
    return rp, ci, n, int(ids[0][0])


def symmetrised(builder):
    rp, ci, n = builder()
    srp, sci = kcore_ref.simple(rp, ci, n)
    return srp.astype(np.int32), sci, n, 0


def _empty(n, source=0):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), n, source


GRAPHS = {}
for _m in (63, 64, 65, 5000):
    GRAPHS["star_out%d" % _m] = functools.partial(star_out, _m)
    GRAPHS["star_in%d" % _m] = functools.partial(star_in, _m)
for _w in (4, 16, 64):
    GRAPHS["rows_around%d" % _w] = functools.partial(rows_around, _w, 5500 + _w)
GRAPHS["layered"] = functools.partial(layered, 5510)
for _l in (K_PULL_LIGHT - 1, K_PULL_LIGHT, K_PULL_LIGHT + 1, 5000):
    for _where in ("first", "last", "absent"):
        GRAPHS["in_row%d_%s" % (_l, _where)] = functools.partial(in_row, _l, _where)
for _n in (257, 1023, 4099):
    GRAPHS["sparse%d" % _n] = functools.partial(sparse_random, _n, 5520 + _n)
GRAPHS.update({
    "path300": lambda: bfs_ref.path(300) + (0,),
    "sink_source": lambda: bfs_ref.path(5) + (4,),                       # the source has no out-edges
    "single": lambda: _empty(1),
    "no_edges": lambda: _empty(4, 2),
    "self_loop_alone": lambda: (np.array([0, 1], np.int32), np.zeros(1, np.int32), 1, 0),
    "self_loop_source": lambda: cc_ref.csr([0, 0, 1], [0, 1, 2], 3) + (0,),
    "untidy300": lambda: cc_ref.untidy(300, 5440) + (0,),                # repeats, self-loops, shuffled rows
    "rmat12_directed": lambda: kcore_ref.GRAPHS["rmat12"]() + (0,),
    "rmat12": lambda: symmetrised(kcore_ref.GRAPHS["rmat12"]),
    "powerlaw": lambda: kcore_ref.GRAPHS["powerlaw"]() + (0,),
})


@functools.lru_cache(maxsize=None)
def graph(name):
    """(rp, ci, n, source) of the named graph; computed once and read-only"""
    rp, ci, n, source = GRAPHS[name]()
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci, n, int(source)


@functools.lru_cache(maxsize=None)
def expected(name, max_depth=0):
    """(row_ptr, parents, levels) of the reference for the named graph; computed once and read-only"""
    out = bfs_tree(*graph(name), max_depth=max_depth)
    for a in out:
        a.setflags(write=False)
    return out
