"""The reference of the clustering-coefficient tests (bspgemm_local_clustering): a scipy model of the definition in
include/bspgemm.h, a naive set-per-vertex implementation to hold it against, the prediction of info.heavy_entries, and
the graphs the tests use.  Nothing here touches the GPU.

With A'c = the deduplicated off-diagonal A and S = A'c | A'c^T:
    d(v)   = |S_v|
    num(v) = rowsum(S .* (S * B^T))(v),  B = S (undirected) or A'c (directed)
           = #{(u, w) : u, w in S_v, (u, w) in B}                        ((S B^T)[v, u] = #{w in S_v : (u, w) in B})
    lcc(v) = 0.0 where d < 2, else num / (d * (d - 1)) in float64
"""
import numpy as np
from scipy.sparse import csr_matrix

import cc_ref
import gen
import kcore_ref

K_SEL_TILE = cc_ref.K_SEL_TILE          # csrc/kernels.hpp kSelTile
K_SEL_STAGE = cc_ref.K_SEL_STAGE        # csrc/sel_rows.hpp kSelStage
K_DEEP = 4                              # csrc/sel_rows.hpp kIsectDeep: 64-element steps a heavy kernel has in flight
LIGHT_DEFAULT = 32                      # BSPGEMM_OPT_DOT_LIGHT's default
HALF = "tril"                           # the half of S that csrc/lcc.hip walks: info.heavy_entries depends on it, no result does


def offdiag(rp, ci, n):
    """A'c as a scipy CSR of int64 ones: A without its diagonal, repeats once, rows sorted"""
    ci = np.asarray(ci)
    if n == 0 or ci.size == 0:
        return csr_matrix((n, n), dtype=np.int64)
    A = csr_matrix((np.ones(ci.size, np.int64), ci.copy(), np.asarray(rp).copy()), shape=(n, n)).tocoo()
    keep = A.row != A.col
    B = csr_matrix((np.ones(int(keep.sum()), np.int64), (A.row[keep], A.col[keep])), shape=(n, n))
    B.data[:] = 1                                                         # (repeats summed up: one entry)
    B.sort_indices()
    return B


def graph(rp, ci, n):
    """S as a scipy CSR of int64 ones"""
    B = offdiag(rp, ci, n)
    S = (B + B.T).tocsr()
    S.data[:] = 1
    S.sort_indices()
    return S


def coefficient(num, d):
    """the header's formula, element by element"""
    num, d = np.asarray(num), np.asarray(d)
    out = np.zeros(d.size, np.float64)
    big = d >= 2
    out[big] = num[big].astype(np.float64) / (d[big].astype(np.float64) * (d[big] - 1).astype(np.float64))
    return out


def local_clustering(rp, ci, n, directed=False):
    """(num int32[n], degree int32[n], lcc float64[n], triangles, reciprocal)"""
    S = graph(rp, ci, n)
    B = offdiag(rp, ci, n) if directed else S
    d = np.diff(S.indptr).astype(np.int32)
    num = np.asarray(S.multiply(S @ B.T).sum(axis=1)).ravel().astype(np.int64) if n else np.zeros(0, np.int64)
    und = num if not directed else np.asarray(S.multiply(S @ S.T).sum(axis=1)).ravel() if n else num
    assert num.size == 0 or num.max() <= 2**31 - 1
    reciprocal = int(B.multiply(B.T).nnz // 2) if directed else 0
    return num.astype(np.int32), d, coefficient(num, d), int(und.sum()) // 6, reciprocal


def naive(rp, ci, n, directed=False):
    """(num, degree) by a loop over sets; for small graphs"""
    rp, ci = np.asarray(rp), np.asarray(ci)
    stored = set()
    for v in range(n):
        for u in ci[rp[v]:rp[v + 1]].tolist():
            if u != v:
                stored.add((v, u))
    nb = [set() for _ in range(n)]
    for v, u in stored:
        nb[v].add(u)
        nb[u].add(v)
    edges = stored if directed else stored | {(u, v) for v, u in stored}
    num = np.array([sum(1 for u in nb[v] for w in nb[v] if u != w and (u, w) in edges) for v in range(n)], np.int32)
    return num.reshape(n), np.array([len(s) for s in nb], np.int32).reshape(n)


def heavy_entries(rp, ci, n, light, half=HALF):
    """info.heavy_entries: the entries (i, j) of the walked half T of S with min(|T_i|, |T_j|) > light"""
    S = graph(rp, ci, n).tocoo()
    keep = S.col < S.row if half == "tril" else S.col > S.row
    r, c = S.row[keep], S.col[keep]
    tl = np.bincount(r, minlength=n)
    return int((np.minimum(tl[r], tl[c]) > light).sum())


def half_entries(rp, ci, n):
    """info.entries = nnz(S) / 2"""
    return int(graph(rp, ci, n).nnz // 2)


def transposed(rp, ci, n):
    """the CSR of A^T, rows sorted (repeats summed into one entry)"""
    ci = np.asarray(ci)
    if n == 0:
        return np.zeros(1, np.int32), np.zeros(0, np.int32), 0
    T = csr_matrix((np.ones(ci.size, np.int64), ci.copy(), np.asarray(rp).copy()), shape=(n, n)).T.tocsr()
    T.sort_indices()
    return T.indptr.astype(np.int32), T.indices.astype(np.int32), n


# ---------------------------------------------------------------- graphs ---------------------------------------------
def complete(m, extra=()):
    """K_m, upper triangle stored (one direction), and the `extra` pairs; n = 1 + the largest id"""
    r, c = np.triu_indices(m, 1)
    er, ec = (np.array([p[0] for p in extra], np.int64), np.array([p[1] for p in extra], np.int64))
    rows, cols = np.concatenate([r, er]), np.concatenate([c, ec])
    return cc_ref.csr(rows, cols, int(max(rows.max(), cols.max())) + 1)


def complete_oriented(m, seed):
    """K_m with every edge stored forwards, backwards or both ways, a third each: the directed weights 1 and 2"""
    rng = np.random.default_rng(seed)
    r, c = np.triu_indices(m, 1)
    kind = rng.integers(0, 3, size=r.size)
    rows = np.concatenate([r[kind != 1], c[kind != 0]])
    cols = np.concatenate([c[kind != 1], r[kind != 0]])
    o = rng.permutation(rows.size)
    return cc_ref.csr(rows[o], cols[o], m)


def friendship(m, hub):
    """the hub joined to both ends of m disjoint edges (m triangles that share the hub): n = 2 m + 1; hub = 0 (the smallest
    id) or 2 m (the largest).  One direction stored, from the smaller id."""
    n = 2 * m + 1
    assert hub in (0, n - 1)
    others = np.arange(1, n) if hub == 0 else np.arange(n - 1)
    a, b = others[0::2], others[1::2]
    rows = np.concatenate([a, np.minimum(others, hub)])
    cols = np.concatenate([b, np.maximum(others, hub)])
    return cc_ref.csr(rows, cols, n)


def untidy(n, pairs, seed):
    """`pairs` random entries among n vertices in both or one direction, 30 % stored twice, a self-loop on every fifth vertex,
    the entries of every row in shuffled order: dense enough for triangles"""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, size=(2, pairs))
    again = rng.random(pairs) < 0.3
    loops = np.arange(0, n, 5)
    rows, cols = np.concatenate([r, r[again], loops]), np.concatenate([c, c[again], loops])
    o = rng.permutation(rows.size)
    return cc_ref.csr(rows[o], cols[o], n)


def far_triangles():
    """two triangles and a bridge, more than kSelStage empty rows between them: the one tile spans them all, and its rows
    are searched in row_ptr itself"""
    far = K_SEL_STAGE + 900
    pairs = [(0, 1), (1, 2), (2, 0), (far, far + 1), (far + 1, far + 2), (far + 2, far), (far, 1), (far + 1, 1)]
    return cc_ref.csr([p[0] for p in pairs], [p[1] for p in pairs], far + 3)


def self_loops(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n


def _empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), n


GRAPHS = {
    "empty0": lambda: _empty(0),
    "empty1": lambda: _empty(1),
    "empty1000": lambda: _empty(1000),
    "self_loops5": lambda: self_loops(5),
    "untidy150": lambda: untidy(150, 2200, 5501),                       # unsorted rows, repeats, self-loops, both and one direction
    "cliques2_40": lambda: kcore_ref.cliques(range(2, 41)),             # one direction; rows that end inside a lane's four entries
    "k70": lambda: complete(70),                                        # rows of 69 straddle the 64-lane step; heavy at T = 32
    "k70_oriented": lambda: complete_oriented(70, 5502),
    # oriented rows of every length 0 .. 257: T and T + 1 (32, 33), 63, 64, 65, kDeep * 64 - 1, kDeep * 64, kDeep * 64 + 1
    "k258": lambda: complete(K_DEEP * 64 + 2),
    "k258_oriented": lambda: complete_oriented(K_DEEP * 64 + 2, 5503),
    "friendship_hub_first": lambda: friendship(3000, 0),
    "friendship_hub_last": lambda: friendship(3000, 6000),
    "star5000": lambda: cc_ref.star(5001, 0, "hub"),
    "tile_minus_1": lambda: complete(91),                               # 91 * 90 / 2 = kSelTile - 1 entries in T
    "tile_exact": lambda: complete(91, [(91, 0)]),
    "tile_plus_1": lambda: complete(91, [(91, 0), (1, 91)]),
    "far_triangles": far_triangles,
    "rmat11": lambda: gen.rmat(11, 8, kcore_ref.SKEW, 5504),
    "rmat8": lambda: gen.rmat(8, 6, kcore_ref.SKEW, 5505),
    # ids beyond the per-workgroup credit cache of kLccSlots = 1024 slots (csrc/lcc.hip): vertices that share a slot
    "rmat12": lambda: gen.rmat(12, 8, kcore_ref.SKEW, 5506),
}
