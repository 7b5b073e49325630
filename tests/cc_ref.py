"""The reference of the connected-components tests (bspgemm_connected_components): scipy's weak components, relabelled to
the smallest vertex id of every component, and the small graphs the tests use.  Nothing here touches the GPU.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

K_SEL_TILE = 4096        # csrc/kernels.hpp kSelTile: entries of one workgroup of the hook
K_SEL_STAGE = 4096       # csrc/sel_rows.hpp kSelStage: rows of a tile's row_ptr window that are staged in LDS


def labels(rp, ci, n):
    """(label int32[n], ncomponents): label[v] = the smallest vertex id of v's weakly connected component"""
    if n == 0:
        return np.zeros(0, np.int32), 0
    ci = np.asarray(ci)
    G = csr_matrix((np.ones(ci.size), ci.copy(), np.asarray(rp).copy()), shape=(n, n))   # (repeats sum up: still an edge)
    ncomp, comp = connected_components(G, directed=True, connection="weak")
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.int32), int(ncomp)


def members(label):
    """(row_ptr, col_idx) of transpose(P): row c lists the vertices with label c, ascending"""
    n = label.size
    rp = np.concatenate([[0], np.cumsum(np.bincount(label, minlength=n))]).astype(np.int32)
    return rp, np.argsort(label, kind="stable").astype(np.int32)


# ---------------------------------------------------------------- graphs ---------------------------------------------
def csr(rows, cols, n):
    """CSR of the pairs as given: rows grouped, the order inside a row and repeats kept"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    o = np.argsort(rows, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return rp.astype(np.int32), cols[o].astype(np.int32), n


def path(n, ids=None):
    """ids[0] -> ids[1] -> ... -> ids[n - 1], one stored entry per edge (ids: 0 .. n - 1 unless given)"""
    ids = np.arange(n) if ids is None else np.asarray(ids)
    return csr(ids[:-1], ids[1:], n)


def path_permuted(n, seed):
    return path(n, np.random.default_rng(seed).permutation(n))


def cycle(n):
    return csr(np.arange(n), (np.arange(n) + 1) % n, n)


def star(n, hub, stored="hub"):
    """the hub joined to every other vertex; stored as the hub's row alone ("hub") or as one entry leaf -> hub per row"""
    leaves = np.setdiff1d(np.arange(n), [hub])
    if stored == "hub":
        return csr(np.full(n - 1, hub), leaves, n)
    return csr(leaves, np.full(n - 1, hub), n)


def short_paths(entries, seed, seg=4):
    """exactly `entries` stored entries as a union of paths of `seg` edges (the last one shorter) over shuffled ids, and
    isolated vertices up to an n that is no multiple of 4: many components"""
    rng = np.random.default_rng(seed)
    full, rest = divmod(entries, seg)
    used = full * (seg + 1) + (rest + 1 if rest else 0)
    n = used + 7
    n += n % 4 == 0
    ids = rng.permutation(n)
    rows, cols, at = [], [], 0
    for edges in [seg] * full + ([rest] if rest else []):
        rows.append(ids[at:at + edges])
        cols.append(ids[at + 1:at + edges + 1])
        at += edges + 1
    return csr(np.concatenate(rows), np.concatenate(cols), n)


def sparse_far_rows(n, per_row, dozen, seed):
    """entries only in the first and the last `dozen` rows, `per_row` random columns each: a tile of the hook spans the
    empty rows between them, and most vertices are isolated"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.arange(dozen), np.arange(n - dozen, n)])
    return csr(np.repeat(rows, per_row), rng.integers(0, n, size=rows.size * per_row), n)


def two_halves(half, seed, joined_from):
    """two directed random paths on `half` vertices each (ids shuffled inside each half), joined by ONE entry (u, v), u in
    the first half and v in the second, and no (v, u): stored as row u's entry ("first") or, the same undirected edge, as
    row v's entry u ("second").  Returns (rp, ci, n, (u, v))."""
    rng = np.random.default_rng(seed)
    a, b = rng.permutation(half), half + rng.permutation(half)
    u, v = int(a[half // 3]), int(b[half // 2])
    rows = np.concatenate([a[:-1], b[:-1], [u if joined_from == "first" else v]])
    cols = np.concatenate([a[1:], b[1:], [v if joined_from == "first" else u]])
    return csr(rows, cols, 2 * half) + ((u, v),)


def untidy(n, seed):
    """about n random edges among n vertices (several components), 30 % of them stored twice, a self-loop on every fifth
    vertex, the entries of every row in shuffled order"""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, size=(2, (3 * n) // 5))
    again = rng.random(r.size) < 0.3
    loops = np.arange(0, n, 5)
    rows, cols = np.concatenate([r, r[again], loops]), np.concatenate([c, c[again], loops])
    o = rng.permutation(rows.size)
    return csr(rows[o], cols[o], n)
