"""The reference of the k-core tests (bspgemm_core_numbers, bspgemm_kcore): a level-synchronous numpy peeling of the
symmetrized diagonal-free graph that also counts the peel sub-rounds as the library defines them, the induced subgraph,
and the small graphs the tests use.  Nothing here touches the GPU.
"""
import numpy as np
from scipy.sparse import csr_matrix

import cc_ref
import gen

SKEW = (0.57, 0.19, 0.19, 0.05)


def simple(rp, ci, n):
    """(row_ptr int64[n + 1], col_idx int32) of A | A^T without its diagonal, rows sorted and duplicate-free"""
    ci = np.asarray(ci)
    if n == 0 or ci.size == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32)
    A = csr_matrix((np.ones(ci.size, np.int8), ci.copy(), np.asarray(rp).copy()), shape=(n, n)).tocoo()
    keep = A.row != A.col
    r, c = np.concatenate([A.row[keep], A.col[keep]]), np.concatenate([A.col[keep], A.row[keep]])
    S = csr_matrix((np.ones(r.size, np.int8), (r, c)), shape=(n, n))       # (repeats sum up: still an edge)
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices.astype(np.int32)


def _rows_of(srp, sci, f):
    """the concatenated rows of the vertices f"""
    lens = srp[f + 1] - srp[f]
    total = int(lens.sum())
    if total == 0:
        return sci[:0]
    starts = np.repeat(srp[f] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return sci[starts + np.arange(total)]


def core_numbers(rp, ci, n):
    """(core int32[n], degeneracy, rounds): core[v] = the largest k such that v lies in a subgraph of simple(A) whose
    vertices all have degree >= k.  Level k takes every unassigned vertex of residual degree <= k as the frontier (an empty
    one moves k up to the smallest residual degree left); a round removes the frontier, lowers its unassigned neighbours'
    degrees and makes those that reach k or less the next frontier.  rounds = rounds with a non-empty frontier over all
    levels; 0 for a graph without edges."""
    srp, sci = simple(rp, ci, n)
    core = np.zeros(n, np.int32)
    if sci.size == 0:
        return core, 0, 0
    deg = np.diff(srp)
    alive = np.ones(n, bool)
    k = rounds = 0
    while alive.any():
        k = max(k, int(deg[alive].min()))
        f = np.flatnonzero(alive & (deg <= k))
        while f.size:
            rounds += 1
            core[f] = k
            alive[f] = False
            nb = _rows_of(srp, sci, f)
            nb = nb[alive[nb]]
            np.subtract.at(deg, nb, 1)
            f = np.unique(nb[deg[nb] <= k])
        k += 1
    return core, int(core.max()), rounds


def kcore(rp, ci, n, k):
    """(row_ptr int32[n + 1], col_idx int32) of the subgraph of simple(A) induced by {v : core(v) >= k}, rows sorted"""
    srp, sci = simple(rp, ci, n)
    inside = core_numbers(rp, ci, n)[0] >= k
    rows = np.repeat(np.arange(n), np.diff(srp))
    keep = inside[rows] & inside[sci] if sci.size else np.zeros(0, bool)
    out_rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]) if n else np.zeros(1)
    return out_rp.astype(np.int32), sci[keep].astype(np.int32)


# ---------------------------------------------------------------- graphs ---------------------------------------------
def spider(m):
    """a root with m children, each with one leaf: n = 2 m + 1, core 1, three rounds with frontiers of m, m and 1"""
    rows = np.concatenate([np.zeros(m, np.int64), 1 + np.arange(m)])
    cols = np.concatenate([1 + np.arange(m), 1 + m + np.arange(m)])
    return cc_ref.csr(rows, cols, 2 * m + 1)


def cliques(sizes):
    """disjoint complete graphs of the given sizes, upper triangles stored: a clique of s vertices has core s - 1"""
    rows, cols, at = [], [], 0
    for s in sizes:
        r, c = np.triu_indices(s, 1)
        rows.append(at + r)
        cols.append(at + c)
        at += s
    return cc_ref.csr(np.concatenate(rows), np.concatenate(cols), at)


def clique_tail(m, tail):
    """K_m with a pendant path of `tail` vertices on its last vertex: the path peels at level 1, then the level jumps"""
    r, c = np.triu_indices(m, 1)
    rows = np.concatenate([r, np.arange(m - 1, m - 1 + tail)])
    cols = np.concatenate([c, np.arange(m, m + tail)])
    return cc_ref.csr(rows, cols, m + tail)


def chains(n):
    """three interleaved chains v -> v + 3"""
    return cc_ref.csr(np.arange(n - 3), np.arange(3, n), n)


def _empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), n


GRAPHS = {
    "path200": lambda: cc_ref.path(200),
    "path200_reversed": lambda: cc_ref.path(200, np.arange(200)[::-1]),
    "path4099_permuted": lambda: cc_ref.path_permuted(4099, 5410),
    "cycle200": lambda: cc_ref.cycle(200),
    "star_hub_last": lambda: cc_ref.star(5001, 5000, "hub"),
    "star_hub_middle": lambda: cc_ref.star(5001, 2500, "hub"),
    "star_leaf_rows": lambda: cc_ref.star(5001, 5000, "leaves"),
    "spider63": lambda: spider(63),
    "spider65": lambda: spider(65),
    "spider257": lambda: spider(257),
    "cliques64_66": lambda: cliques([64, 65, 66]),
    "cliques2_40": lambda: cliques(range(2, 41)),
    "clique70_tail130": lambda: clique_tail(70, 130),
    "rmat12": lambda: gen.rmat(12, 8, SKEW, 5401),
    "rmat10": lambda: gen.rmat(10, 6, SKEW, 5403),
    "powerlaw": lambda: gen.powerlaw(6000, 3, 5402),
    "uniform4096_d8": lambda: gen.uniform(4096, 8, 7),
    "untidy300": lambda: cc_ref.untidy(300, 5440),
    "chains257": lambda: chains(257),
    "chains1023": lambda: chains(1023),
    "chains4099": lambda: chains(4099),
    "empty0": lambda: _empty(0),
    "empty1": lambda: _empty(1),
    "empty4": lambda: _empty(4),
    "empty1000": lambda: _empty(1000),
    "self_loop": lambda: (np.array([0, 1], np.int32), np.zeros(1, np.int32), 1),
}
