"""The reference of the graph-colouring tests (bspgemm_graph_coloring): the key formula of include/bspgemm.h, a
level-synchronous numpy model of first fit in the order of (key, id) on the symmetrized diagonal-free graph that also
counts the frontier launches as the library defines them, a plain sequential first fit to check the model with, the four
properties of a greedy colouring, and the graphs the tests use.  Nothing here touches the GPU.
"""
import numpy as np

import cc_ref
import kcore_ref
from kcore_ref import simple

ORDERS = ("natural", "random", "largest")
WINDOW = 2048            # csrc/color.hip kColWindow: colours of one bitmap window


def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in uint32, elementwise"""
    x = np.asarray(x).astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x.astype(np.uint64) * np.uint64(0x7feb352d)).astype(np.uint32)
    x = x ^ (x >> np.uint32(15))
    x = (x.astype(np.uint64) * np.uint64(0x846ca68b)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def keys(n, order, seed, deg):
    """key uint64[n] = (hi << 32) | lo.  deg: the degrees in simple(A)"""
    v = np.arange(n, dtype=np.uint32)
    if order == "natural":
        return v.astype(np.uint64)
    lo = mix32(v ^ np.uint32(seed & 0xFFFFFFFF)).astype(np.uint64)
    if order == "random":
        return lo
    assert order == "largest", order
    hi = (0x7fffffff - np.asarray(deg, np.int64)).astype(np.uint64)
    return (hi << np.uint64(32)) | lo


def visit_order(key):
    """the vertices sorted by (key, id): u precedes v when it comes first here"""
    key = np.asarray(key, np.uint64)
    return np.lexsort((np.arange(key.size), key))


def rank_of(key):
    """rank[v] = the position of v in visit_order(key)"""
    order = visit_order(key)
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    return rank


def _rows_with_owner(srp, sci, f):
    """(owner, neighbour): the concatenated rows of the vertices f and, per entry, the index into f of its row"""
    lens = srp[f + 1] - srp[f]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64), sci[:0]
    owner = np.repeat(np.arange(f.size), lens)
    starts = np.repeat(srp[f] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return owner, sci[starts + np.arange(total)]


def coloring_of(srp, sci, n, key):
    """the model on a simple graph and given keys: (colour int32[n], ncolors, rounds)"""
    if n == 0:
        return np.zeros(0, np.int32), 0, 0
    if sci.size == 0:
        return np.zeros(n, np.int32), 1, 0
    rank = rank_of(key)
    rows = np.repeat(np.arange(n), np.diff(srp))
    cnt = np.bincount(rows[rank[sci] < rank[rows]], minlength=n)       # preceding neighbours not coloured yet
    colour = np.full(n, -1, np.int64)
    f = np.flatnonzero(cnt == 0)
    rounds = 0
    while f.size:
        rounds += 1
        owner, nb = _rows_with_owner(srp, sci, f)
        before = rank[nb] < rank[f[owner]]
        # first fit: per frontier vertex the smallest colour that is missing among its preceding neighbours' colours
        taken = np.unique(owner[before] * np.int64(n + 1) + colour[nb[before]])
        assert (colour[nb[before]] >= 0).all()                         # coloured by an earlier round
        t_owner, t_colour = taken // (n + 1), taken % (n + 1)
        mex = np.zeros(f.size, np.int64)
        if taken.size:
            start = np.flatnonzero(np.concatenate([[True], t_owner[1:] != t_owner[:-1]]))
            size = np.diff(np.concatenate([start, [taken.size]]))
            at = np.arange(taken.size) - np.repeat(start, size)            # position inside the owner's sorted colours
            gap = np.where(t_colour != at, at, np.int64(n + 1))
            first = np.minimum.reduceat(gap, start)
            mex[t_owner[start]] = np.where(first == n + 1, size, first)
        colour[f] = mex
        after = nb[~before]
        np.subtract.at(cnt, after, 1)
        f = np.unique(after[cnt[after] == 0])
    assert (colour >= 0).all()
    return colour.astype(np.int32), int(colour.max()) + 1, rounds


def coloring(rp, ci, n, order="random", seed=0):
    """(colour int32[n], ncolors, rounds) as bspgemm_graph_coloring defines them for the graph of A's entries.  A round
    colours every vertex whose preceding neighbours are all coloured; rounds = rounds with a non-empty frontier; 0 for a
    graph without edges"""
    srp, sci = simple(rp, ci, n)
    return coloring_of(srp, sci, n, keys(n, order, seed, np.diff(srp)))


def first_fit(srp, sci, n, visit):
    """plain sequential first fit in the given visiting order: colour int32[n]"""
    colour = np.full(n, -1, np.int64)
    for v in np.asarray(visit).tolist():
        used = set(colour[sci[srp[v]:srp[v + 1]]].tolist())
        c = 0
        while c in used:
            c += 1
        colour[v] = c
    return colour.astype(np.int32)


def check_properties(srp, sci, n, colour, key):
    """proper, greedy (a vertex of colour c has a neighbour of every colour below c), class 0 is the maximal independent
    set that the order picks first, and at most maxdeg + 1 colours"""
    colour = np.asarray(colour, np.int64)
    if n == 0:
        return
    rows = np.repeat(np.arange(n), np.diff(srp))
    assert (colour[rows] != colour[sci]).all(), "two adjacent vertices share a colour"
    below = np.unique(rows * np.int64(n + 1) + colour[sci])
    b_row, b_col = below // (n + 1), below % (n + 1)
    lower = np.bincount(b_row[b_col < colour[b_row]], minlength=n)         # distinct colours below the vertex's own
    assert np.array_equal(lower, colour), "a vertex lacks a neighbour of some lower colour"
    zero = colour == 0
    has_zero_nb = np.bincount(rows[zero[sci]], minlength=n) > 0
    assert (zero | has_zero_nb).all() and not (zero & has_zero_nb).any(), "class 0 is not a maximal independent set"
    mis = np.zeros(n, bool)                                               # the lexicographically first one of the order
    blocked = np.zeros(n, bool)
    for v in visit_order(key).tolist():
        if not blocked[v]:
            mis[v] = True
            blocked[sci[srp[v]:srp[v + 1]]] = True
    assert np.array_equal(mis, zero), "class 0 is not the first maximal independent set of the order"
    assert colour.max() + 1 <= int(np.diff(srp).max(initial=0)) + 1


# ---------------------------------------------------------------- graphs ---------------------------------------------
CLIQUE = 2060            # more than one window of colours


def window_above():
    """K_2060 (under NATURAL clique vertex i gets colour i) and a last vertex adjacent to the clique's 0..9 and 2050..2059:
    it gets colour 10, the marks above the first window are ignored"""
    rp, ci, n = kcore_ref.cliques([CLIQUE])
    r = np.repeat(np.arange(n), np.diff(rp))
    nb = np.concatenate([np.arange(10), np.arange(2050, 2060)])
    return cc_ref.csr(np.concatenate([r, np.full(nb.size, CLIQUE)]), np.concatenate([ci, nb]), CLIQUE + 1)


def window_below():
    """window_above and a second last vertex adjacent to the clique's 0..2047 and 2049: the first window is full, in the
    second pass the marks below its base are ignored and it gets colour 2048; the leaf hanging off it is released once"""
    rp, ci, n = window_above()
    r = np.repeat(np.arange(n), np.diff(rp))
    nb = np.concatenate([np.arange(WINDOW), [WINDOW + 1]])
    rows = np.concatenate([r, np.full(nb.size, CLIQUE + 1), [CLIQUE + 1]])
    cols = np.concatenate([ci, nb, [CLIQUE + 2]])
    return cc_ref.csr(rows, cols, CLIQUE + 3)


# the small named graphs: everything the ABI test checks against networkx and the GPU test against the model
SMALL = ["cliques64_66", "spider63", "spider65", "spider257", "star_hub_last", "star_hub_middle", "star_leaf_rows", "path200",
         "path4099_permuted", "chains257", "chains1023", "chains4099", "rmat12", "rmat10", "powerlaw", "uniform4096_d8",
         "untidy300", "cycle200", "empty0", "empty1", "empty4", "empty1000", "self_loop"]
GRAPHS = {name: kcore_ref.GRAPHS[name] for name in SMALL}
# the graphs with more colours than one window holds: 2060 rounds each, so only under the orders the tests name
WINDOW_GRAPHS = {
    "cliques2048_2060": lambda: kcore_ref.cliques([WINDOW, CLIQUE]),
    "window_above": window_above,
    "window_below": window_below,
}
