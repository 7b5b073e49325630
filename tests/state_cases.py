"""One table of every compute entry point with its operands and its reference (no tests in here).

CASES maps a name to a Case: which prototypes of include/bspgemm.h the call reaches (`entries`), on which operands it runs
(`on`: names of OPERANDS), which options it forces (`options`), run(ctx, g) -> (arrays, info) and check(g, arrays, info)
against the existing tests/*_ref.py model or the oracle.  arrays is a tuple of numpy arrays, info a dict of ints; both are
compared bit for bit between runs by the tests that drive the table (test_gpu_dirty_state.py: poisoned memory;
test_gpu_workspace_layout.py: cold, warm and grown workspaces).  A reference is computed once per (case, operands).

The graphs are stored untidily: every row descending and naming its largest column twice, so every call that wants
canonical rows canonicalises mid-way (two transposes in the workspace), and no transpose is passed in.
  untidy   the n = 70 graph of the layout test: no multiple of 4, two waves, vertex 0 of degree 69
  hub      6000 vertices; vertex 0 is adjacent to 4100 others in both directions (above 4096 = kSelTile, kSsspChunk,
           kLpGroupCap and the hub-chunk sizes of PageRank and betweenness) with R-MAT scale 10 noise around it; the entry
           count is no multiple of 4 or of 4096
  gap      two cliques of six with 4200 empty rows between them (the unstaged tile window of the transpose)
The closure runs on untidy and gap only: on the hub graph it is a dense 6000 x 6000 result.  The products that a statistic
can tell apart (flows, small path, padded rows, blocked table, a row in each heavy class) run on pairs of their own and
assert that statistic, so a case cannot silently change path.
"""
import collections
import functools

import numpy as np

import bspgemm
import bc_ref
import bfs_ref
import bfs_tree_ref
import cc_ref
import cdlp_ref
import color_ref
import dot_ref
import extract_ref
import gen
import kcore_ref
import ktruss_ref
import lcc_ref
import match_ref
import pagerank_ref
import scc_ref
import setop_ref
import sssp_ref

SEED = 6100
WORDS = (0xFFFFFFFF, 0x00000001)

Case = collections.namedtuple("Case", "entries on options run check")


class Ops:
    """the operands of a case: `host` name -> (row_ptr, col_idx, rows, cols), read-only; upload(ctx) gives `dev` name ->
    Matrix.  A graph has the one operand "A" and the shorthands rp, ci, n, A."""

    def __init__(self, key, host):
        self.key, self.host, self.dev = key, host, {}
        for rp, ci, _, _ in host.values():
            rp.setflags(write=False)
            ci.setflags(write=False)

    def upload(self, ctx):
        self.dev = {k: ctx.upload(rp, ci, cols) for k, (rp, ci, _, cols) in self.host.items()}
        return self

    def free(self):
        for m in self.dev.values():
            m.free()
        self.dev = {}

    rp = property(lambda self: self.host["A"][0])
    ci = property(lambda self: self.host["A"][1])
    n = property(lambda self: self.host["A"][2])
    A = property(lambda self: self.dev["A"])


def cached(fn):
    """the reference of (g, further hashable arguments), computed once per operands key"""
    memo = {}

    @functools.wraps(fn)
    def wrapper(g, *args):
        k = (g.key,) + args
        if k not in memo:
            memo[k] = fn(g, *args)
        return memo[k]
    return wrapper


# ---------------------------------------------------------------- operands ------------------------------------------
def untidy_store(r, c, n):
    """(rp, ci) of the distinct pairs: every row descending, its largest column once more at the end"""
    key = np.unique((np.asarray(r, np.int64) << 32) | np.asarray(c, np.int64))
    r, c = key >> 32, key & 0xFFFFFFFF
    first = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]])) if r.size else np.zeros(0, np.int64)
    last = np.concatenate([first[1:], [r.size]]).astype(np.int64) - 1
    rr, cc = np.concatenate([r, r[last]]), np.concatenate([c, c[last]])
    o = np.lexsort((np.concatenate([-c, np.ones(last.size, np.int64)]), rr))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=n))]).astype(np.int32)
    return rp, cc[o].astype(np.int32)


def small_graph(n):
    """the layout test's graph: vertex 0 points at everybody else (degree n - 1), everybody else at three pseudo-random
    vertices and back at 0 from every third; every row is stored descending and names its first column twice"""
    rng = np.random.default_rng(SEED + n)
    rows = []
    for v in range(n):
        cols = np.arange(1, n) if v == 0 else np.unique(np.concatenate([rng.integers(0, n, size=3), [0] if v % 3 == 0 else []]))
        cols = np.asarray(cols, np.int32)[::-1]
        rows.append(np.concatenate([cols, cols[:1]]) if cols.size else np.asarray([v, v], np.int32))
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    assert not pagerank_ref.is_canonical(rp, ci, n)
    return rp, ci, n


def hub_graph():
    n, hub = 6000, 4100
    rng = np.random.default_rng(SEED)
    r_rp, r_ci, rn = gen.rmat(10, 20, (0.45, 0.22, 0.22, 0.11), SEED)
    where = rng.permutation(np.arange(1, n))[:rn]
    rr = where[np.repeat(np.arange(rn), np.diff(r_rp))]
    v = np.arange(1, hub + 1)
    r, c = np.concatenate([np.zeros(hub, np.int64), v, rr]), np.concatenate([v, np.zeros(hub, np.int64), where[r_ci]])
    extra = 0
    while True:                                             # an entry count that is no multiple of 4 (nor, then, of 4096)
        rp, ci = untidy_store(np.concatenate([r, np.full(extra, n - 1)]), np.concatenate([c, n - 2 - np.arange(extra)]), n)
        if ci.size % 4:
            break
        extra += 1
    assert rp[1] - rp[0] == hub + 1 and np.count_nonzero(ci == 0) >= hub and ci.size % 4096 and 20000 < ci.size < 40000
    return rp, ci, n


def gap_graph():
    n, k = 4212, 6
    a, b = np.arange(k), np.arange(n - k, n)
    r = np.concatenate([np.repeat(a, k), np.repeat(b, k)])
    c = np.concatenate([np.tile(a, k), np.tile(b, k)])
    off = r != c
    rp, ci = untidy_store(r[off], c[off], n)
    assert np.all(np.diff(rp)[k:n - k] == 0) and n - 2 * k > 4096
    return rp, ci, n


def graph_ops(key, rp, ci, n):
    return Ops(key, {"A": (rp, ci, n, n)})


def pair_ops(key, a_rp, a_ci, b_rp, b_ci, cols):
    return Ops(key, {"A": (a_rp, a_ci, a_rp.size - 1, b_rp.size - 1), "B": (b_rp, b_ci, b_rp.size - 1, cols)})


def _heavy_pair():
    """gen.rank_rows over 2^24 columns (rank class to 6144 products, dense class above 8192): a row in each heavy class"""
    return gen.rank_rows(1 << 24, [3000, 7000, 9000, 100, 1, 2500, 6144, 8192, 8193], seed=SEED, counts=(600, 200, 100)) + (1 << 24,)


_BUILDERS = {
    "untidy": lambda: graph_ops("untidy", *small_graph(70)),
    "hub": lambda: graph_ops("hub", *hub_graph()),
    "gap": lambda: graph_ops("gap", *gap_graph()),
    "mixed": lambda: pair_ops("mixed", *gen.mixed_class_rows(), 4096),
    "uniform300": lambda: pair_ops("uniform300", *(gen.uniform(300, 4, SEED)[:2] * 2), 300),
    "heavy": lambda: pair_ops("heavy", *_heavy_pair()),
}
GRAPHS = ("untidy", "hub", "gap")


@functools.lru_cache(maxsize=None)
def operands(name):
    """the host side of the named operands, built once (Ops.upload makes the device side per context)"""
    return _BUILDERS[name]()


def fresh(name):
    """a copy of operands(name) that a test may upload and free on its own"""
    g = operands(name)
    return Ops(g.key, g.host)


# ---------------------------------------------------------------- downloads -----------------------------------------
def _matrix(M):
    out = M.download()
    M.free()
    return tuple(out)


def _result(R):
    out = tuple(R.download()) + ((R.download_values(),) if R.values_device else ())
    R.free()
    return out


def _keys(rp, ci):
    rp = np.asarray(rp, np.int64)
    return (np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp)) << 32) | np.asarray(ci, np.int64)


def _same_csr(got, rp, ci, values=None):
    assert np.array_equal(got[0], rp), "row_ptr differs at rows %s" % np.flatnonzero(np.asarray(got[0]) != np.asarray(rp))[:5]
    assert np.array_equal(got[1], ci), "col_idx differs"
    if values is not None:
        assert np.array_equal(got[2], values), "values differ"


# ---------------------------------------------------------------- the products --------------------------------------
STAT_KEYS = ("rows", "nnz_a", "products", "nnz_c", "flow", "prepass_kernel", "small_path", "padded_rows", "rows_per_bin")


def _stats(ctx):
    st = ctx.stats()
    return {k: ([int(x) for x in st[k]] if k == "rows_per_bin" else int(st[k])) for k in STAT_KEYS}


@cached
def _want(g):
    from oracle import oracle as O
    a, b = g.host["A"], g.host.get("B", g.host["A"])
    return O.spgemm(a[0], a[1], b[0], b[1], b[3])


@cached
def _counted(g):
    from test_gpu_masked_count import count_ref
    a = g.host["A"]
    return count_ref(a[0], a[1], a[0], a[1], a[0], a[1], a[3])


def _multiply(flow="auto"):
    def run(ctx, g):
        ctx.set_flow(flow)
        try:
            R = ctx.multiply(g.dev["A"], g.dev.get("B", g.dev["A"]))
        finally:
            ctx.set_flow("auto")
        return _result(R), _stats(ctx)
    return run


def _check_multiply(**expect):
    def check(g, arrays, info):
        _same_csr(arrays, *_want(g))
        a, b = g.host["A"], g.host.get("B", g.host["A"])
        F = gen.row_products(a[0], a[1], b[0], 0, a[2])
        assert info["products"] == int(F.sum()) and info["nnz_c"] == arrays[1].size
        for k, v in expect.items():
            assert info[k] == v, "the case left its path: %s is %s, not %s" % (k, info[k], v)
        if not info["small_path"]:
            assert info["rows_per_bin"] == gen.expected_bins(F, b[3])
    return check


def _check_heavy(g, arrays, info):
    _check_multiply(small_path=0)(g, arrays, info)
    assert all(info["rows_per_bin"][b] >= 1 for b in (gen.RANK_BIN, gen.MID_BIN, gen.DENSE_BIN)), info["rows_per_bin"]


def _masked(ctx, g):
    return _result(ctx.multiply_masked(g.A, g.A, g.A)), {}


def _check_masked(g, arrays, info):
    _same_csr(arrays, *_counted(g)[:2])


def _complement(ctx, g):
    return _result(ctx.multiply_masked(g.A, g.A, g.A, complement=True)), {}


def _check_complement(g, arrays, info):
    from test_gpu_complement import complement_ref
    _same_csr(arrays, *complement_ref(_want(g), g.rp, g.ci))


def _accumulate(ctx, g):
    return _result(ctx.multiply_accumulate(g.A, g.A, g.A)), {}


def _check_accumulate(g, arrays, info):
    keys = np.union1d(_keys(*_want(g)), _keys(g.rp, g.ci))
    _same_csr(arrays, np.concatenate([[0], np.cumsum(np.bincount(keys >> 32, minlength=g.n))]), keys & 0xFFFFFFFF)


def _masked_count(ctx, g):
    R = ctx.multiply_masked_count(g.A, g.A, g.A)
    total = R.values_sum()
    return _result(R), {"values_sum": total}


def _check_masked_count(g, arrays, info):
    rp, ci, v = _counted(g)
    _same_csr(arrays, rp, ci, v)
    assert info["values_sum"] == int(v.sum(dtype=np.int64))


def _dot(ctx, g):
    R, info = ctx.multiply_masked_dot(g.A, g.A, g.A)
    return _result(R), info


def _check_dot(g, arrays, info):
    e = _dot_want(g)
    assert all(np.array_equal(x, y) for x, y in zip(arrays, e))
    assert info["kept"] == e[1].size and info["canonicalised"] == 7


@cached
def _dot_want(g):
    return dot_ref.dot_ref((g.rp, g.ci), (g.rp, g.ci), (g.rp, g.ci), g.n, g.n, g.n, g.n)


# ---------------------------------------------------------------- operands from operands ----------------------------
def _from_result(ctx, g):
    R = ctx.multiply_masked_count(g.A, g.A, g.A)
    M = ctx.matrix_from_result(R, g.n)
    R.free()
    return _matrix(M), {}


def _from_result_where(ctx, g):
    R = ctx.multiply_masked_count(g.A, g.A, g.A)
    M = ctx.matrix_from_result_where(R, g.n, ">=", 2)
    R.free()
    return _matrix(M), {}


def _check_from_result_where(g, arrays, info):
    rp, ci, v = _counted(g)
    _same_csr(arrays, *ktruss_ref.where_ref(rp, ci, v, ">=", 2))


def _select(op):
    return lambda ctx, g: (_matrix(ctx.select(g.A, op)), {})


def _check_select(op):
    return lambda g, arrays, info: _same_csr(arrays, *ktruss_ref.select_ref(g.rp, g.ci, op))


def _reversed_rows(g):
    """B of the set operations: row i is row n - 1 - i of A, as stored"""
    lens = np.diff(g.rp)[::-1]
    starts = g.rp[:-1][::-1].astype(np.int64)
    idx = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), g.ci[idx]


def _setop(op):
    def run(ctx, g):
        B = ctx.upload(*_reversed_rows(g), g.n)
        try:
            return _matrix(ctx.setop(g.A, B, op)), {}
        finally:
            B.free()
    return run


def _check_setop(op):
    return lambda g, arrays, info: _same_csr(arrays, *setop_ref.setop_ref(g.rp, g.ci, *_reversed_rows(g), g.n, g.n, op))


def _equal(ctx, g):
    B = ctx.upload(*_reversed_rows(g), g.n)
    S = ctx.upload(*setop_ref.canonical_ref(g.rp, g.ci, g.n, g.n), g.n)
    try:
        return (), {"equal_to_its_canonical_form": int(ctx.matrix_equal(g.A, S)), "equal_to_another": int(ctx.matrix_equal(g.A, B))}
    finally:
        B.free()
        S.free()


def _check_equal(g, arrays, info):
    other = np.array_equal(np.unique(_keys(g.rp, g.ci)), np.unique(_keys(*_reversed_rows(g))))
    assert info == {"equal_to_its_canonical_form": 1, "equal_to_another": int(other)}


def _symmetrize(ctx, g):
    return _matrix(ctx.symmetrize(g.A, drop_diagonal=True)), {}


def _transpose(ctx, g):
    return _matrix(ctx.transpose(g.A)), {}


def lists(n):
    """the row and column lists of the extraction: rows out of order with a repeat, columns out of order"""
    return np.arange(n)[::-1][: max(1, 2 * n // 3)].tolist() + [0], np.arange(n)[::-2].tolist()


def _extract(ctx, g):
    I, J = lists(g.n)
    M, info = ctx.extract(g.A, rows=I, cols=J)
    return _matrix(M), info


EXTRACT_INFO = ("kept", "scanned", "hub_chunks", "cols_monotone", "sorted_by", "canonicalised")


@cached
def _extract_want(g, by_row):
    I, J = (g.ci[g.rp[0]:g.rp[1]], None) if by_row else lists(g.n)
    return extract_ref.model(g.rp, g.ci, g.n, g.n, I, J)


def _check_extract(by_row):
    def check(g, arrays, info):
        e = _extract_want(g, by_row)
        _same_csr(arrays, e["rp"], e["ci"])
        assert all(info[k] == e[k] for k in EXTRACT_INFO), (info, {k: e[k] for k in EXTRACT_INFO})
    return check


def _extract_rows_of(ctx, g):
    M, info = ctx.extract_rows_of(g.A, MI=g.A, ri=0)        # the rows that row 0 of A lists as stored (one of them twice)
    return _matrix(M), info


@cached
def _closure_want(g, transitive):
    import scipy.sparse as sp
    M = sp.csr_matrix((np.ones(g.ci.size, np.int64), g.ci, g.rp), shape=(g.n, g.n))
    live = np.flatnonzero(np.diff(g.rp) > 0)                # (reachability lives on the rows that have entries and their targets)
    live = np.union1d(live, g.ci)
    D = (M[live][:, live].toarray() > 0)
    if not transitive:                                      # A*: every vertex reaches itself; A+: only along a cycle, a self-loop included
        np.fill_diagonal(D, True)
    while True:
        N = D | ((D.astype(np.float32) @ D.astype(np.float32)) > 0)
        if np.array_equal(N, D):
            break
        D = N
    r, c = np.nonzero(D)
    keys = (live[r].astype(np.int64) << 32) | live[c]
    if not transitive:
        keys = np.union1d(keys, (np.arange(g.n, dtype=np.int64) << 32) | np.arange(g.n))
    return np.concatenate([[0], np.cumsum(np.bincount(keys >> 32, minlength=g.n))]), keys & 0xFFFFFFFF


def _closure(transitive):
    def run(ctx, g):
        R, it = ctx.closure(g.A, transitive=transitive)
        return _result(R), {"iterations": it}
    return run


def _check_closure(transitive):
    return lambda g, arrays, info: _same_csr(arrays, *_closure_want(g, transitive))


# ---------------------------------------------------------------- triangles and trusses -----------------------------
def _triangles(method):
    return lambda ctx, g: ((), {"triangles": ctx.triangle_count(g.A, method)})


@cached
def _triangles_want(g):
    return ktruss_ref.triangles_ref(g.rp, g.ci, g.n)


def _check_triangles(g, arrays, info):
    assert info == {"triangles": _triangles_want(g)}


def _ktruss(method):
    def run(ctx, g):
        T, it, conv = ctx.ktruss(g.A, 3, method=method)
        return _matrix(T), {"iterations": it, "converged": int(conv)}
    return run


@cached
def _ktruss_want(g):
    return ktruss_ref.ktruss_ref(g.rp, g.ci, g.n, 3)


def _check_ktruss(g, arrays, info):
    (rp, ci), it, conv = _ktruss_want(g)
    _same_csr(arrays, rp, ci)
    assert info == {"iterations": it, "converged": int(conv)}


# ---------------------------------------------------------------- the graph algorithms ------------------------------
def _sources(n):
    return (0, n - 1, min(1, n - 1))


def _bfs(ctx, g):
    R, depth, complete = ctx.bfs(g.A, _sources(g.n))
    return _result(R), {"depth": depth, "complete": int(complete)}


@cached
def _bfs_want(g):
    dist = bfs_ref.distances(g.rp, g.ci, g.n, _sources(g.n))
    return bfs_ref.levels_csr(dist, 0)


def _check_bfs(g, arrays, info):
    rp, ci, v = _bfs_want(g)
    _same_csr(arrays, rp, ci, v)
    assert info == {"depth": int(v.max()), "complete": 1}


def _bfs_tree(direction):
    def run(ctx, g):
        R, info = ctx.bfs_tree(g.A, AT=None, source=0, direction=direction)
        return _result(R), info
    return run


@cached
def _bfs_tree_want(g):
    return bfs_tree_ref.bfs_tree(g.rp, g.ci, g.n, 0)


def _check_bfs_tree(direction):
    def check(g, arrays, info):
        e_rp, e_parent, e_level = _bfs_tree_want(g)
        assert all(np.array_equal(a, e) for a, e in zip(arrays, (e_rp, e_parent, e_level)))
        assert info["reached"] == e_parent.size and info["transposed"] == (1 if info["pull_levels"] else 0)
        assert info["complete"] == 1 and info["depth"] == int(e_level.max())
        if direction != "auto":
            assert info["pull_levels" if direction == "push" else "push_levels"] == 0
    return check


def _cc(ctx, g):
    P, count, rounds = ctx.connected_components(g.A)
    return _matrix(P), {"components": count, "rounds": rounds}


@cached
def _cc_want(g):
    return cc_ref.labels(g.rp, g.ci, g.n)


def _check_cc(g, arrays, info):
    label, count = _cc_want(g)
    assert np.array_equal(arrays[1], label) and info["components"] == count


def _scc(ctx, g):
    P, count, rounds, sweeps = ctx.strongly_connected_components(g.A)
    return _matrix(P), {"components": count, "rounds": rounds, "sweeps": sweeps}


@cached
def _scc_want(g):
    return scc_ref.labels(g.rp, g.ci, g.n)


def _check_scc(g, arrays, info):
    label, count = _scc_want(g)
    assert np.array_equal(arrays[1], label) and info["components"] == count


def _core(ctx, g):
    R, top, rounds = ctx.core_numbers(g.A)
    return _result(R), {"degeneracy": top, "rounds": rounds}


@cached
def _core_want(g):
    return kcore_ref.core_numbers(g.rp, g.ci, g.n)


def _check_core(g, arrays, info):
    core, top, rounds = _core_want(g)
    assert np.array_equal(arrays[2], core) and info == {"degeneracy": top, "rounds": rounds}


def _kcore(ctx, g):
    T, top = ctx.kcore(g.A, 2)
    return _matrix(T), {"degeneracy": top}


@cached
def _kcore_want(g):
    return kcore_ref.kcore(g.rp, g.ci, g.n, 2)


def _check_kcore(g, arrays, info):
    _same_csr(arrays, *_kcore_want(g))
    assert info == {"degeneracy": _core_want(g)[1]}


def _color(ctx, g):
    P, colors, rounds = ctx.graph_coloring(g.A, order="largest", seed=SEED)
    return _matrix(P), {"colors": colors, "rounds": rounds}


@cached
def _color_want(g):
    return color_ref.coloring(g.rp, g.ci, g.n, order="largest", seed=SEED)


def _check_color(g, arrays, info):
    colour, colors, rounds = _color_want(g)
    assert np.array_equal(arrays[1], colour) and info == {"colors": colors, "rounds": rounds}


def _lp(ctx, g):
    P, info = ctx.label_propagation(g.A, max_iter=4)
    return _matrix(P), info


@cached
def _lp_want(g):
    return cdlp_ref.label_propagation(g.rp, g.ci, g.n, 4)


def _check_lp(g, arrays, info):
    labels, iterations, converged, changed, communities = _lp_want(g)
    assert np.array_equal(arrays[1], labels)
    assert (info["iterations"], info["converged"], info["changed"], info["communities"]) == (iterations, converged, changed, communities)


def _lcc(ctx, g):
    R, degree, lcc, info = ctx.local_clustering(g.A, directed=True)
    return _result(R) + (degree, lcc.view(np.uint64)), info


@cached
def _lcc_want(g):
    return lcc_ref.local_clustering(g.rp, g.ci, g.n, True)


def _check_lcc(g, arrays, info):
    num, d, lcc, triangles, reciprocal = _lcc_want(g)
    assert np.array_equal(arrays[2], num) and np.array_equal(arrays[3], d) and np.array_equal(arrays[4], lcc.view(np.uint64))
    assert (info["triangles"], info["reciprocal"]) == (triangles, reciprocal)


def _pagerank(method):
    def run(ctx, g):
        fixed, rank, info = ctx.pagerank(g.A, AT=None, method=method, damping=0.85, max_iter=5)
        return (fixed, rank.view(np.uint64)), info
    return run


@cached
def _pagerank_want(g):
    return pagerank_ref.pagerank(g.rp, g.ci, g.n, 0.85, 5)


def _check_pagerank(method):
    def check(g, arrays, info):
        e = _pagerank_want(g)
        assert np.array_equal(arrays[0], e["fixed"]) and np.array_equal(arrays[1], e["rank"].view(np.uint64))
        assert all(info[k] == e[k] for k in ("mass", "delta", "dangling", "iterations", "converged"))
        assert info["method"] == method
        if method == bspgemm.PR_PULL:
            assert info["transposed"] == 1 and info["canonicalised"] == 1
    return check


def _bc_sources(n):
    return np.arange(min(n, 5))


def _bc(ctx, g):
    fixed, bc, info = ctx.betweenness(g.A, _bc_sources(g.n))
    return (fixed, bc.view(np.uint64)), info


@cached
def _bc_want(g):
    return bc_ref.model(g.rp, g.ci, g.n, _bc_sources(g.n))


def _check_bc(g, arrays, info):
    e = _bc_want(g)
    assert np.array_equal(arrays[0], e["fixed"]) and np.array_equal(arrays[1], e["bc"].view(np.uint64))
    assert all(info[k] == e[k] for k in info if k != "canonicalised") and info["canonicalised"] == 1


MATCH_INFO = ("pairs", "entries_walked", "hub_chunks", "rounds", "lanes")


def _match(ctx, g):
    P, mate, info = ctx.maximal_matching(g.A, "random", SEED, mate=True)
    return _matrix(P) + (mate,), info


@cached
def _match_want(g):
    return match_ref.matching(g.rp, g.ci, g.n, order="random", seed=SEED)


def _check_match(lanes=0):
    def check(g, arrays, info):
        e = _match_want(g)
        assert np.array_equal(arrays[1], e.labels) and np.array_equal(arrays[2], e.mate)
        want = e._replace(lanes=lanes if lanes and e.rounds else e.lanes)
        assert all(info[k] == getattr(want, k) for k in MATCH_INFO), (info, want)
    return check


WEIGHTS = (7, 1, 255)             # seed, wmin, wmax of the hashed lengths


def _weights(ctx, g):
    W = ctx.weights_hashed(g.A, *WEIGHTS)
    try:
        w = W.download()
        U = ctx.weights_upload(g.A, w)                       # ... and back through the upload
        try:
            return (w, U.download()), {"nnz": int(W.nnz), "sum": int(W.sum), "uploaded_sum": int(U.sum)}
        finally:
            U.free()
    finally:
        W.free()


@cached
def _weights_want(g):
    return sssp_ref.weight_hash(g.rp, g.ci, g.n, *WEIGHTS)


def _check_weights(g, arrays, info):
    w = _weights_want(g)
    total = int(w.sum(dtype=np.uint64))
    assert np.array_equal(arrays[0], w) and np.array_equal(arrays[1], w)
    assert info == {"nnz": int(w.size), "sum": total, "uploaded_sum": total}


def _sssp(lanes=0):
    def run(ctx, g):
        W = ctx.weights_hashed(g.A, *WEIGHTS)
        try:
            dist, parent, info = ctx.sssp(g.A, W, 0, lanes=lanes, parents=True)
        finally:
            W.free()
        return (dist, parent), info
    return run


@cached
def _sssp_want(g):
    w = _weights_want(g)
    dist = sssp_ref.dijkstra(g.rp, g.ci, w, g.n, 0)
    m = sssp_ref.model(g.rp, g.ci, w, g.n, 0)
    assert np.array_equal(m.dist, dist)
    return dist, sssp_ref.parents(g.rp, g.ci, w, g.n, 0, dist), m


def _check_sssp(lanes=0):
    def check(g, arrays, info):
        dist, parent, m = _sssp_want(g)
        assert np.array_equal(arrays[0], dist) and np.array_equal(arrays[1], parent)
        want = m._replace(lanes=lanes or m.lanes)
        assert all(info[k] == getattr(want, k) for k in sssp_ref.INFO), (info, want)
    return check


# ---------------------------------------------------------------- sharding helpers ----------------------------------
def _row_work_prefix(ctx, g):
    return (ctx.row_work_prefix(g.A, g.A),), {}


def _prefix_want(g):
    return np.concatenate([[0], np.cumsum(gen.row_products(g.rp, g.ci, g.rp, 0, g.n))]).astype(np.int64)


def _check_row_work_prefix(g, arrays, info):
    assert np.array_equal(arrays[0], _prefix_want(g))


def _partition_rows(ctx, g):
    return (ctx.partition_rows(g.A, g.A, 4),), {}


def _check_partition_rows(g, arrays, info):
    from bspgemm import dist as bdist
    assert np.array_equal(arrays[0], bdist.shard_bounds(_prefix_want(g), 4))


def _stitch_inputs(g):
    """a made-up 3-rank gather of the row lengths of A: ragged shards, the middle one empty, its pad slots set"""
    lens = np.diff(g.rp).astype(np.int32)
    bounds = np.array([0, g.n // 3, g.n // 3, g.n], dtype=np.int32)
    width = max(int(np.diff(bounds).max()), 1)
    padded = np.zeros((3, width), dtype=np.int32)
    for r in range(3):
        padded[r, : bounds[r + 1] - bounds[r]] = lens[bounds[r]: bounds[r + 1]]
    padded[1, :] = 7
    return padded, bounds, width


def _lengths_to_row_ptr(ctx, g):
    import torch
    dev = torch.device("cuda", ctx.device)
    padded, bounds, width = _stitch_inputs(g)
    d_len = torch.from_numpy(padded).to(dev)
    out = torch.empty(g.n + 1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    ctx.lengths_to_row_ptr(d_len.data_ptr(), 3, width, bounds, out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return (out.cpu().numpy(),), {}


def _check_lengths_to_row_ptr(g, arrays, info):
    assert np.array_equal(arrays[0], g.rp.astype(np.int64))


# ---------------------------------------------------------------- the table -----------------------------------------
SMALL_GRAPHS = ("untidy", "gap")
CASES = {}


def _add(name, entries, run, check, on=GRAPHS, options=None):
    assert name not in CASES
    CASES[name] = Case(tuple(entries.split()), tuple(on), dict(options or {}), run, check)


_add("multiply", "bspgemm_multiply", _multiply(), _check_multiply())
_add("multiply_upper_bound", "bspgemm_multiply", _multiply("upper-bound"), _check_multiply(flow=1, small_path=0), on=("mixed",),
     options={"small_path": 0})
_add("multiply_exact", "bspgemm_multiply", _multiply("exact"), _check_multiply(flow=2, small_path=0), on=("mixed",),
     options={"small_path": 0})
_add("multiply_small_on", "bspgemm_multiply", _multiply(), _check_multiply(small_path=1), on=("uniform300",), options={"small_path": 1})
_add("multiply_small_off", "bspgemm_multiply", _multiply(), _check_multiply(small_path=0), on=("uniform300",), options={"small_path": 0})
_add("multiply_padded_rows", "bspgemm_multiply", _multiply(), _check_multiply(padded_rows=1, small_path=0), on=("mixed",),
     options={"padded_rows": 1, "small_path": 0})
_add("multiply_blocked_table", "bspgemm_multiply", _multiply(), _check_multiply(prepass_kernel=1, small_path=0), on=("mixed",),
     options={"blocked_extents": 1, "small_path": 0})
_add("multiply_heavy_classes", "bspgemm_multiply", _multiply(), _check_heavy, on=("heavy",))
_add("masked", "bspgemm_multiply_masked", _masked, _check_masked)
_add("complement", "bspgemm_multiply_masked_ex", _complement, _check_complement)
_add("accumulate", "bspgemm_multiply_accumulate", _accumulate, _check_accumulate)
_add("masked_count", "bspgemm_multiply_masked_count bspgemm_result_values_sum", _masked_count, _check_masked_count)
_add("masked_dot", "bspgemm_multiply_masked_dot", _dot, _check_dot)
_add("from_result", "bspgemm_matrix_from_result", _from_result, lambda g, arrays, info: _same_csr(arrays, *_counted(g)[:2]))
_add("from_result_where", "bspgemm_matrix_from_result_where", _from_result_where, _check_from_result_where)
for _op in ("tril", "triu", "offdiag"):
    _add("select_" + _op, "bspgemm_matrix_select", _select(_op), _check_select(_op))
for _op in ("or", "and", "andnot", "xor"):
    _add("setop_" + _op, "bspgemm_matrix_setop", _setop(_op), _check_setop(_op))
_add("matrix_equal", "bspgemm_matrix_equal", _equal, _check_equal)
_add("symmetrize", "bspgemm_matrix_symmetrize", _symmetrize,
     lambda g, arrays, info: _same_csr(arrays, *setop_ref.symmetrize_ref(g.rp, g.ci, g.n, True)))
_add("transpose", "bspgemm_matrix_transpose", _transpose,
     lambda g, arrays, info: _same_csr(arrays, *setop_ref.transpose_ref(g.rp, g.ci, g.n, g.n)))
_add("extract", "bspgemm_matrix_extract", _extract, _check_extract(False))
_add("extract_rows_of", "bspgemm_matrix_extract_rows_of", _extract_rows_of, _check_extract(True))
_add("closure", "bspgemm_closure", _closure(False), _check_closure(False), on=SMALL_GRAPHS)
_add("closure_transitive", "bspgemm_closure_ex", _closure(True), _check_closure(True), on=SMALL_GRAPHS)
_add("triangle_count", "bspgemm_triangle_count", _triangles("product"), _check_triangles)
_add("triangle_count_dot", "bspgemm_triangle_count_ex", _triangles("dot"), _check_triangles)
_add("ktruss", "bspgemm_ktruss", _ktruss("product"), _check_ktruss)
_add("ktruss_dot", "bspgemm_ktruss_ex", _ktruss("dot"), _check_ktruss)
_add("bfs", "bspgemm_bfs", _bfs, _check_bfs)
for _d in ("pull", "push", "auto"):
    _add("bfs_tree" + ("" if _d == "pull" else "_" + _d), "bspgemm_bfs_tree", _bfs_tree(_d), _check_bfs_tree(_d))
_add("cc", "bspgemm_connected_components", _cc, _check_cc)
_add("scc", "bspgemm_strongly_connected_components", _scc, _check_scc)
_add("core_numbers", "bspgemm_core_numbers", _core, _check_core)
_add("kcore", "bspgemm_kcore", _kcore, _check_kcore)
_add("coloring", "bspgemm_graph_coloring", _color, _check_color)
_add("label_propagation", "bspgemm_label_propagation", _lp, _check_lp)
_add("lcc", "bspgemm_local_clustering", _lcc, _check_lcc)
_add("pagerank_pull", "bspgemm_pagerank", _pagerank(bspgemm.PR_PULL), _check_pagerank(bspgemm.PR_PULL))
_add("pagerank_push", "bspgemm_pagerank", _pagerank(bspgemm.PR_PUSH), _check_pagerank(bspgemm.PR_PUSH))
_add("betweenness", "bspgemm_betweenness", _bc, _check_bc)
_add("maximal_matching", "bspgemm_maximal_matching", _match, _check_match())
_add("weights_hashed", "bspgemm_weights_hashed bspgemm_weights_download bspgemm_weights_upload", _weights, _check_weights)
_add("sssp", "bspgemm_weights_hashed bspgemm_sssp", _sssp(), _check_sssp())
_add("row_work_prefix", "bspgemm_row_work_prefix", _row_work_prefix, _check_row_work_prefix)
_add("partition_rows", "bspgemm_partition_rows", _partition_rows, _check_partition_rows)
_add("lengths_to_row_ptr", "bspgemm_lengths_to_row_ptr", _lengths_to_row_ptr, _check_lengths_to_row_ptr)
# the hub graph once more under every forced value of the min-class and lanes options
for _v in (1, 2, 3):
    _add("label_propagation_min_class_%d" % _v, "bspgemm_label_propagation", _lp, _check_lp, on=("hub",), options={"lp_min_class": _v})
    _add("pagerank_pull_min_class_%d" % _v, "bspgemm_pagerank", _pagerank(bspgemm.PR_PULL), _check_pagerank(bspgemm.PR_PULL),
         on=("hub",), options={"pr_min_class": _v})
for _v in (4, 16, 64):
    _add("betweenness_lanes_%d" % _v, "bspgemm_betweenness", _bc, _check_bc, on=("hub",), options={"bc_lanes": _v})
    _add("maximal_matching_lanes_%d" % _v, "bspgemm_maximal_matching", _match, _check_match(_v), on=("hub",), options={"match_lanes": _v})
    _add("extract_lanes_%d" % _v, "bspgemm_matrix_extract", _extract, _check_extract(False), on=("hub",), options={"extract_lanes": _v})
    _add("bfs_tree_push_lanes_%d" % _v, "bspgemm_bfs_tree", _bfs_tree("push"), _check_bfs_tree("push"), on=("hub",),
         options={"bfs_push_lanes": _v})
    _add("sssp_lanes_%d" % _v, "bspgemm_weights_hashed bspgemm_sssp", _sssp(_v), _check_sssp(_v), on=("hub",))

# the cases that take any square graph: what test_gpu_workspace_layout.py runs at its own sizes
GRAPH_CASES = tuple(k for k, c in CASES.items() if c.on == GRAPHS or c.on == SMALL_GRAPHS)
IDS = tuple((name, on) for name, c in CASES.items() for on in c.on)


def covered_entries():
    """every prototype of include/bspgemm.h that a case names"""
    return {e for c in CASES.values() for e in c.entries}


def run_case(ctx, name, g):
    """the case on the uploaded operands g under its options, which go back to what they were: (arrays, info)"""
    case = CASES[name]
    before = {k: ctx.get_option(k) for k in case.options}
    for k, v in case.options.items():
        ctx.set_option(k, v)
    try:
        return case.run(ctx, g)
    finally:
        for k, v in before.items():
            ctx.set_option(k, v)


def check_case(name, g, arrays, info):
    CASES[name].check(g, arrays, info)


def same(x, y):
    """two (arrays, info) agree bit for bit"""
    return x[1] == y[1] and len(x[0]) == len(y[0]) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(x[0], y[0]))
