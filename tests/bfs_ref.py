"""The reference of the BFS tests (bspgemm_bfs): levels from scipy's unweighted shortest paths, as the CSR with values
that the library's result object holds, and the small graphs the tests walk.  Nothing here touches the GPU.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import shortest_path

K_SEL_TILE = 4096        # csrc/kernels.hpp kSelTile: entries of one workgroup of the merge


def distances(rp, ci, n, sources):
    """S x n int64: the BFS level of every vertex from every source along the edges row -> column, -1 where unreachable"""
    ci = np.asarray(ci)
    G = csr_matrix((np.ones(ci.size), ci.copy(), np.asarray(rp).copy()), shape=(n, n))   # (repeats sum up: still an edge)
    dist = shortest_path(G, directed=True, unweighted=True, indices=np.asarray(sources, np.int64))
    return np.where(np.isinf(dist), -1, dist).astype(np.int64).reshape(len(sources), n)


def levels_csr(dist, max_depth=0):
    """(row_ptr int64, col_idx int32, values int32) of the reached entries of `dist`, cut at max_depth when it is > 0"""
    keep = dist >= 0
    if max_depth > 0:
        keep &= dist <= max_depth
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(keep)                     # row-major: rows ascending, columns ascending inside a row
    return rp, cols.astype(np.int32), dist[rows, cols].astype(np.int32)


def bfs_ref(rp, ci, n, sources, max_depth=0):
    """what bspgemm_bfs returns: ((row_ptr, col_idx, values), depth, complete)"""
    dist = distances(rp, ci, n, sources)
    full_depth = int(dist.max())
    csr = levels_csr(dist, max_depth)
    depth = int(csr[2].max())
    if max_depth <= 0 or max_depth > full_depth:
        complete = 1                                  # an empty frontier (or the full set) ended the search
    else:
        complete = int(csr[1].size == len(sources) * n)   # the cap ended it, unless everything was reached by then
    return csr, depth, complete


def frontier_sizes(dist):
    """entries per level, over all sources"""
    return np.bincount(dist[dist >= 0]).tolist()


# ---------------------------------------------------------------- graphs ---------------------------------------------
def _csr(rows, cols, n):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    key = np.unique(rows * (1 << 32) + cols)
    rows, cols = key >> 32, key & 0xFFFFFFFF
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return rp.astype(np.int32), cols.astype(np.int32), n


def path(n):
    """0 -> 1 -> ... -> n - 1"""
    return _csr(np.arange(n - 1), np.arange(1, n), n)


def cycle(n):
    return _csr(np.arange(n), (np.arange(n) + 1) % n, n)


def star(n):
    """0 -> every other vertex"""
    return _csr(np.zeros(n - 1, np.int64), np.arange(1, n), n)


def complete(n):
    r, c = np.nonzero(~np.eye(n, dtype=bool))
    return _csr(r, c, n)


def layered(layers, extra, seed):
    """A graph whose BFS from vertex id[0] has exactly `layers[k]` vertices at level k, plus `extra` vertices nobody reaches
    (they point into the layers).  Every vertex of layer k + 1 has two random parents in layer k, and every vertex two edges
    back into its own or an earlier layer, which the mask has to drop.  The vertex ids are shuffled, so the columns of
    the visited set and of each frontier interleave.  Returns (rp, ci, n, id) with id[k] = the vertices of layer k."""
    rng = np.random.default_rng(seed)
    n = int(sum(layers)) + extra
    perm = rng.permutation(n)
    bounds = np.concatenate([[0], np.cumsum(layers)])
    ids = [perm[bounds[k]:bounds[k + 1]] for k in range(len(layers))]
    rows, cols = [], []
    for k in range(1, len(layers)):
        for _ in range(2):
            rows.append(rng.choice(ids[k - 1], size=ids[k].size))
            cols.append(ids[k])
    for k in range(len(layers)):
        back = perm[:bounds[k + 1]]
        for _ in range(2):
            rows.append(ids[k])
            cols.append(rng.choice(back, size=ids[k].size))
    lost = perm[bounds[-1]:]
    rows.append(lost)
    cols.append(rng.choice(perm[:bounds[-1]], size=lost.size))
    rp, ci, _ = _csr(np.concatenate(rows), np.concatenate(cols), n)
    return rp, ci, n, ids
