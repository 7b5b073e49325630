"""The OR-accumulating product C = D | (A*B) (bspgemm_multiply_accumulate, Context.multiply_accumulate) and the transitive
closure built on it (bspgemm_closure_ex with BSPGEMM_CLOSURE_TRANSITIVE), bit for bit against references built from the
CPU oracle's product, scipy and the plain product of stacked operands.

Every shape of the complemented-mask test runs with four Ds: a random one (unsorted rows, repeats, columns beyond B's and
negative ones, rows without products), D = A, an empty D (the plain product) and D = pattern(A*B) (the plain product).
The launch is asserted from the stats: upper-bound flow, no small path, products = F, and the rows per class of
F_i + |D_i| -- so the accumulate twin of every class that a shape populates really ran.  Then rows whose D moves them
across every class boundary, the stacked-operand identity, knobs, row ranges, errors, closures, a visited-set BFS and one
large product.
"""
import ctypes as C
import math

import numpy as np
import pytest

import bspgemm
import gen
import test_gpu_complement as TC
from oracle import oracle as O

pytestmark = pytest.mark.gpu
RANK_BIN, MID_BIN, DENSE_BIN = gen.RANK_BIN, gen.MID_BIN, gen.DENSE_BIN
ERR_INVALID = 1
_keys, _diff, _slice, _csr = TC._keys, TC._diff, TC._slice, TC._csr


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- reference ---------------------------------------
def accumulate_ref(want, d_rp, d_ci, cols, r0=0):
    """keys of the product (rows r0.. of it) and of D's rows r0.. within [0, cols): (row_ptr int64, col_idx)"""
    rp, ci = want
    R = rp.size - 1
    d_rp = np.asarray(d_rp, np.int64)
    d_ci = np.asarray(d_ci, np.int64)
    lo, hi = d_rp[r0], d_rp[r0 + R]
    drows = np.repeat(np.arange(R, dtype=np.int64), np.diff(d_rp[r0:r0 + R + 1]))
    dc = d_ci[lo:hi]
    ok = (dc >= 0) & (dc < cols)
    k = np.union1d(_keys(rp, ci), (drows[ok] << 32) | dc[ok])
    counts = np.bincount((k >> 32).astype(np.int64), minlength=R)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), (k & 0xffffffff).astype(np.int32)


def random_d(rng, R, cols, want, beyond=1000, in_range=False):
    """a third of the product's entries (some twice), three random columns per row -- some beyond B's columns and some
    negative unless in_range -- all in random order within their rows"""
    rp, ci = want
    rows_c = np.repeat(np.arange(R, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    pick = rng.random(ci.size) < 0.33
    r1, c1 = rows_c[pick], np.asarray(ci, np.int64)[pick]
    twice = rng.random(r1.size) < 0.2
    r3 = rng.integers(0, R, size=3 * R)
    c3 = rng.integers(0, cols, size=r3.size) if in_range else rng.integers(-50, cols + beyond, size=r3.size)
    rows = np.concatenate([r1, r1[twice], r3])
    cols_ = np.concatenate([c1, c1[twice], c3])
    perm = rng.permutation(rows.size)
    order = np.argsort(rows[perm], kind="stable")           # rows grouped, columns within a row left unsorted
    rows, cols_ = rows[perm][order], cols_[perm][order]
    d_rp = np.zeros(R + 1, np.int64)
    np.add.at(d_rp, rows + 1, 1)
    return np.cumsum(d_rp).astype(np.int32), cols_.astype(np.int32)


def _dlen(d_rp, r0, r1):
    return np.diff(np.asarray(d_rp, np.int64))[r0:r1]


def _run(ctx, A, B, D, r0=0, r1=None):
    Cr = ctx.multiply_accumulate(A, B, D, r0, r1)
    st = ctx.stats()
    got = Cr.download()
    Cr.free()
    return got, st


def _path(st):
    return dict(flow=st["flow"], small_path=st["small_path"], rows_per_bin=st["rows_per_bin"], bin_cap=st["bin_cap"],
                products=st["products"], nnz_c=st["nnz_c"])


def _stacked(s, d_rp, d_ci):
    """[A | I] and [B ; D] as host CSR (D within B's columns): their plain product is D | (A*B)"""
    R, nb = s["a_rp"].size - 1, s["b_rp"].size - 1
    a_rows = np.repeat(np.arange(R), np.diff(s["a_rp"]))
    rows = np.concatenate([a_rows, np.arange(R)])
    cols = np.concatenate([s["a_ci"].astype(np.int64), nb + np.arange(R)])
    o = np.argsort(rows, kind="stable")
    sa_rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=R))]).astype(np.int32)
    sb_rp = np.concatenate([s["b_rp"].astype(np.int64), s["b_rp"][-1] + np.asarray(d_rp[1:], np.int64)]).astype(np.int32)
    sb_ci = np.concatenate([s["b_ci"], d_ci]).astype(np.int32)
    return sa_rp, cols[o].astype(np.int32), sb_rp, sb_ci, nb + R


# ---------------------------------------------------------------- D moves rows across the classes ------------------
def _d_classes(ncols, seed):
    """B: 4096 rows of one column (j) and 1024 rows of 64 (64k .. 64k + 63), all below 65536.  A's rows hit a product count
    F just below each one-wave capacity, and D adds a few columns of its own beyond 65536: 3 keep the row in its class, 6
    push it into the next (the last one into a heavy class).  Also rows of F = 0 with |D| = 3000, a rank-class row, a
    small-dense row and a hub row whose D columns lie only in the last span / window, which no product reaches."""
    rng = np.random.default_rng(seed)
    b_rp = np.concatenate([np.arange(4097), 4096 + 64 * np.arange(1, 1025)]).astype(np.int32)
    b_ci = np.concatenate([np.arange(4096), np.arange(65536)]).astype(np.int32)
    a_rows, d_rows = [], []

    def row(F, dcols):
        k, one = divmod(F, 64)
        a = list(4096 + rng.choice(1024, size=k, replace=k > 1024)) + list(rng.choice(4096, size=one, replace=False))
        a_rows.append(list(rng.permutation(a)))
        d_rows.append(list(dcols))

    far = lambda n: rng.choice(np.arange(65536, ncols), size=n, replace=False)
    for cap in gen.WAVE_CAPS:
        for extra in (3, 6):
            row(cap - 3, far(extra))
    for _ in range(3):
        row(0, far(3000))
    last = np.arange(ncols - min(ncols // 4, 1 << 19), ncols)              # the last span / window(s)
    mid_cap, rank_cap = gen._mid_rank_caps(ncols)
    for F in ([2500] if rank_cap else []) + [min(rank_cap + 1000, mid_cap - 2000) if rank_cap else 3000, mid_cap + 5000]:
        row(F, rng.choice(last, size=1500, replace=False))
    row(0, [])                                                          # an empty row
    a_rp, a_ci = _csr(a_rows)
    d_rp, d_ci = _csr(d_rows)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols, d=(d_rp, d_ci))


D_CLASS_SHAPES = {"d_classes_200k": lambda: _d_classes(200_000, 61), "d_classes_3M_spans": lambda: _d_classes(3_000_000, 62)}


@pytest.mark.parametrize("name", list(D_CLASS_SHAPES))
def test_accumulate_d_moves_classes(ctx, name):
    s = D_CLASS_SHAPES[name]()
    R, cols = s["a_rp"].size - 1, s["ncols"]
    d_rp, d_ci = s["d"]
    want = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
    F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)
    size = F + _dlen(d_rp, 0, R)
    bins = gen.expected_bins(size, cols)
    assert bins != gen.expected_bins(F, cols)
    assert all(bins[b] > 0 for b in range(1, 17)) and bins[MID_BIN] > 0 and bins[DENSE_BIN] > 0, bins
    if cols > (1 << 18):
        assert bins[RANK_BIN] > 0, bins
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    D = ctx.upload(d_rp, d_ci, cols)
    try:
        got, st = _run(ctx, A, B, D)
    finally:
        for h in (A, B, D):
            h.free()
    exp = accumulate_ref(want, d_rp, d_ci, cols)
    assert _diff(got, exp) is None
    assert _path(st) == dict(flow=1, small_path=0, rows_per_bin=bins, bin_cap=gen.expected_bin_caps(cols),
                             products=int(F.sum()), nnz_c=int(exp[1].size))


# ---------------------------------------------------------------- every shape, four Ds ------------------------------
@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_accumulate_shape(ctx, name):
    s = TC._shape(name)
    want = s["want"]
    R, cols = s["a_rp"].size - 1, s["ncols"]
    F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)
    rng = np.random.default_rng(R + cols % 1013)
    ds = {"random": random_d(rng, R, cols, want), "D=A": (s["a_rp"], s["a_ci"]),
          "empty": (np.zeros(R + 1, np.int32), np.zeros(0, np.int32)),
          "D=pattern(A*B)": (want[0].astype(np.int32), want[1])}
    # a random D has rows where A's row is empty or has no products (where the shape has such rows): they output D's row
    ctx.set_flow("auto")
    for k, v in (("small_path", -1), ("padded_rows", -1), ("blocked_extents", -1), ("check", 0), ("class_streams", 2)):
        ctx.set_option(k, v)
    A, B = TC._upload(ctx, s)
    failures = []
    try:
        Cm = ctx.multiply(A, B)
        plain = Cm.download()
        Cm.free()
        for dname, (d_rp, d_ci) in ds.items():
            if dname == "D=A" and s["a_ci"].size and int(s["a_ci"].max()) >= cols:
                continue                                            # (A's columns lie beyond B's: D.cols > B.cols)
            D = ctx.upload(d_rp, d_ci, cols)
            try:
                got, st = _run(ctx, A, B, D)
            finally:
                D.free()
            exp = accumulate_ref(want, d_rp, d_ci, cols)
            if dname in ("empty", "D=pattern(A*B)"):
                bad = _diff(got, plain)
                if bad:
                    failures.append("D %s: differs from bspgemm_multiply: %s" % (dname, bad))
            bad = _diff(got, exp)
            if bad:
                failures.append("D %s: %s" % (dname, bad))
            e = dict(flow=1, small_path=0, rows_per_bin=gen.expected_bins(F + _dlen(d_rp, 0, R), cols),
                     bin_cap=gen.expected_bin_caps(cols), products=int(F.sum()), nnz_c=int(exp[1].size))
            if _path(st) != e:
                failures.append("D %s: path %s, expected %s" % (dname, _path(st), e))
    finally:
        A.free()
        B.free()
    assert not failures, "%s:\n  %s" % (name, "\n  ".join(failures))


# ---------------------------------------------------------------- stacked operands ----------------------------------
@pytest.mark.parametrize("name", ["uniform", "class_boundaries", "rmat13_skewed", "rank_700k"])
def test_accumulate_equals_stacked_product(ctx, name):
    s = TC._shape(name)
    R, cols = s["a_rp"].size - 1, s["ncols"]
    d_rp, d_ci = random_d(np.random.default_rng(77), R, cols, s["want"], in_range=True)
    sa_rp, sa_ci, sb_rp, sb_ci, nsb = _stacked(s, d_rp, d_ci)
    A, B = TC._upload(ctx, s)
    D = ctx.upload(d_rp, d_ci, cols)
    SA = ctx.upload(sa_rp, sa_ci, nsb)
    SB = ctx.upload(sb_rp, sb_ci, cols)
    try:
        got, _ = _run(ctx, A, B, D)
        Cs = ctx.multiply(SA, SB)
        stacked = Cs.download()
        Cs.free()
    finally:
        for h in (A, B, D, SA, SB):
            h.free()
    assert _diff(got, stacked) is None


# ---------------------------------------------------------------- knobs and ranges ----------------------------------
@pytest.mark.parametrize("name", ["rmat14_skewed_wide", "tiny_b_wide_40M", "class_boundaries"])
def test_accumulate_knobs_and_ranges(ctx, name):
    """padded_rows x blocked_extents x class_streams 1..3, each over the whole A, an interior range, one row and none; then
    the exact flow and the small path asked for, which the accumulating product does not take"""
    s = TC._shape(name)
    want = s["want"]
    R, cols = s["a_rp"].size - 1, s["ncols"]
    d_rp, d_ci = random_d(np.random.default_rng(41), R, cols, want)
    full = accumulate_ref(want, d_rp, d_ci, cols)
    F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)
    heavy = int(np.argmax(F))
    ctx.set_flow("auto")
    ctx.set_option("small_path", -1)
    ctx.set_option("check", 0)
    D = ctx.upload(d_rp, d_ci, cols)
    failures, runs = [], 0
    try:
        for k, (pad, blk, cs) in enumerate(np.ndindex(2, 2, 3)):
            cs += 1
            for opt, v in (("padded_rows", pad), ("blocked_extents", blk), ("class_streams", cs)):
                ctx.set_option(opt, v)
            A, B = TC._upload(ctx, s)
            try:
                inner = (min(R // 7 + k, R // 2), max(R - R // 5 - k, R // 2 + 1))
                for r0, r1 in ((0, R), inner, (heavy, heavy + 1), (R // 2, R // 2)):
                    got, st = _run(ctx, A, B, D, r0, r1)
                    runs += 1
                    tag = "padded_rows=%d blocked_extents=%d class_streams=%d rows=[%d,%d)" % (pad, blk, cs, r0, r1)
                    # D indexed by absolute row: the reference of the slice is the slice of the whole reference
                    bad = _diff(got, _slice(full, r0, r1))
                    if bad:
                        failures.append("%s: %s" % (tag, bad))
                    if r1 > r0:
                        p = {k2: st[k2] for k2 in ("flow", "small_path", "class_streams")}
                        if p != dict(flow=1, small_path=0, class_streams=cs):
                            failures.append("%s: path %s" % (tag, p))
                        if st["rows_per_bin"] != gen.expected_bins(F[r0:r1] + _dlen(d_rp, r0, r1), cols):
                            failures.append("%s: rows_per_bin %s" % (tag, st["rows_per_bin"]))
            finally:
                A.free()
                B.free()
        for opt, v in (("padded_rows", -1), ("blocked_extents", -1), ("class_streams", 2)):
            ctx.set_option(opt, v)
        A, B = TC._upload(ctx, s)
        try:
            for flow, small in (("exact", -1), ("auto", 1), ("exact", 1)):
                ctx.set_flow(flow)
                ctx.set_option("small_path", small)
                got, st = _run(ctx, A, B, D)
                runs += 1
                if _diff(got, full) or (st["flow"], st["small_path"]) != (1, 0):
                    failures.append("flow=%s small_path=%d: %s, path %s" % (flow, small, _diff(got, full), (st["flow"], st["small_path"])))
        finally:
            A.free()
            B.free()
    finally:
        D.free()
        ctx.set_flow("auto")
        for opt, v in (("small_path", -1), ("padded_rows", -1), ("blocked_extents", -1), ("class_streams", 2)):
            ctx.set_option(opt, v)
    assert not failures, "%s: %d of %d runs wrong:\n  %s" % (name, len(failures), runs, "\n  ".join(failures))


# ---------------------------------------------------------------- errors -------------------------------------------
def test_accumulate_errors(ctx):
    rp, ci, n = gen.uniform(700, 6, 5301)
    A = ctx.upload(rp, ci, n)
    short = ctx.upload(rp[:301], ci[:rp[300]], n)
    wide = ctx.upload(rp, ci, n + 1)
    other = bspgemm.Context(0)
    Dx = other.upload(rp, ci, n)
    L = bspgemm.lib()
    try:
        cases = [(A, A, Dx, 0, n), (A, A, short, 0, n), (A, A, short, 0, 301), (A, A, wide, 0, n), (A, A, A, 5, 3),
                 (A, A, A, 0, n + 1), (A, A, A, -1, 3)]
        for a, b, d, r0, r1 in cases:
            out = C.c_void_p(1)
            st = L.bspgemm_multiply_accumulate(ctx._h, a._h, b._h, d._h, r0, r1, C.byref(out))
            assert st == ERR_INVALID and not out.value, (r0, r1, st)
        for args in ((None, A._h, A._h, A._h), (ctx._h, None, A._h, A._h), (ctx._h, A._h, None, A._h), (ctx._h, A._h, A._h, None)):
            out = C.c_void_p(1)
            assert L.bspgemm_multiply_accumulate(*args, 0, n, C.byref(out)) == ERR_INVALID and not out.value
        assert L.bspgemm_multiply_accumulate(ctx._h, A._h, A._h, A._h, 0, n, None) == ERR_INVALID
        # a D of exactly row_end rows is enough, and a narrower one is fine
        got, _ = _run(ctx, A, A, short, 0, 300)
        want = O.spgemm(rp, ci, rp, ci, n)
        assert _diff(got, accumulate_ref(_slice(want, 0, 300), rp[:301], ci[:rp[300]], n)) is None
    finally:
        for h in (A, short, wide, Dx):
            h.free()
        other.close()


# ---------------------------------------------------------------- closures -----------------------------------------
def _reach_plus(n, edges):
    """A+ by scipy: off the diagonal the finite shortest paths, on it the nodes that lie on a cycle (self-loop or a
    strongly connected component of two or more)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components, shortest_path
    r, c = (np.asarray(edges, np.int64).reshape(-1, 2).T if len(edges) else (np.zeros(0, np.int64), np.zeros(0, np.int64)))
    G = csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    reach = np.isfinite(shortest_path(G, directed=True, unweighted=True))
    np.fill_diagonal(reach, False)
    _, lab = connected_components(G, directed=True, connection="strong")
    size = np.bincount(lab)
    diag = (size[lab] > 1)
    diag[r[r == c]] = True
    reach[np.arange(n), np.arange(n)] = diag
    return reach


def _graph(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "empty":
        return []
    m = 3 * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    if kind == "dag":
        r, c = np.minimum(r, c), np.maximum(r, c)
        keep = r != c
        r, c = r[keep], c[keep]
    elif kind == "cycles":
        keep = r != c
        r, c = r[keep], c[keep]
        ring = np.arange(0, 40)                                     # one long cycle, plus the random edges' own
        r, c = np.concatenate([r, ring]), np.concatenate([c, np.roll(ring, -1)])
    elif kind == "self_loops":
        r, c = np.minimum(r, c), np.maximum(r, c)                   # a DAG ...
        s = rng.choice(n, 25, replace=False)                        # ... with self-loops: only those are on the diagonal
        r, c = np.concatenate([r, s]), np.concatenate([c, s])
    return list(zip(r.tolist(), c.tolist()))


@pytest.mark.parametrize("kind", ["dag", "cycles", "self_loops", "empty"])
def test_transitive_closure(ctx, kind):
    n = 700
    edges = _graph(kind, n, 8100 + len(kind))
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[a].append(b)
    for k in range(0, len(rows), 5):                                 # repeats in T0
        rows[k] = rows[k] + rows[k][:2]
    rp, ci = _csr(rows)
    A = ctx.upload(rp, ci, n)
    try:
        T, it = ctx.closure(A, transitive=True)
        trp, tci = T.download()
        T.free()
        Tstar, it0 = ctx.closure(A)
        star = Tstar.download()
        Tstar.free()
        # flags = 0 is bspgemm_closure, bit for bit
        L = bspgemm.lib()
        r, i0 = C.c_void_p(), C.c_int()
        assert L.bspgemm_closure_ex(ctx._h, A._h, 0, 64, C.byref(r), C.byref(i0)) == 0
        ex = bspgemm.Result(ctx, r)
        assert _diff(ex.download(), star) is None and i0.value == it0
        ex.free()
        r = C.c_void_p(1)
        assert L.bspgemm_closure_ex(ctx._h, A._h, 2, 64, C.byref(r), None) == ERR_INVALID and not r.value
    finally:
        A.free()
    reach = _reach_plus(n, edges)
    exp_rp = np.concatenate([[0], np.cumsum(reach.sum(axis=1))]).astype(np.int64)
    exp_ci = np.nonzero(reach)[1].astype(np.int32)
    assert _diff((trp, tci), (exp_rp, exp_ci)) is None
    assert 1 <= it <= math.ceil(math.log2(n)) + 2, it
    if kind == "dag":
        assert not reach.diagonal().any()
    # A* is A+ with the whole diagonal
    k_star = _keys(*star)
    k_plus = np.union1d(_keys(trp, tci), (np.arange(n, dtype=np.int64) << 32) | np.arange(n))
    assert np.array_equal(k_star, k_plus)


# ---------------------------------------------------------------- visited-set BFS -------------------------------------
def test_bfs_with_visited_set(ctx):
    """next = frontier*A and not visited (complement mask), visited = visited | frontier*A (accumulate), both on the device
    and kept there between levels: the levels are scipy's unweighted shortest paths"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    rp, ci, n = gen.rmat(14, 8, (0.57, 0.19, 0.19, 0.05), 5601)
    sources = np.random.default_rng(10).choice(n, size=8, replace=False)
    S = sources.size
    A = ctx.upload(rp, ci, n)
    level = np.full((S, n), -1, np.int64)
    level[np.arange(S), sources] = 0
    f_rp, f_ci = _csr([[s] for s in sources])
    frontier = ctx.upload(f_rp, f_ci, n)
    visited = ctx.upload(f_rp, f_ci, n)
    d = 0
    try:
        while True:
            d += 1
            nx = ctx.multiply_masked(frontier, A, visited, complement=True)
            vx = ctx.multiply_accumulate(frontier, A, visited)
            nrp, nci = nx.download()
            if nci.size == 0:
                nx.free()
                vx.free()
                break
            for s in range(S):
                cols = nci[nrp[s]:nrp[s + 1]]
                assert (level[s, cols] < 0).all()
                level[s, cols] = d
            frontier.free()
            visited.free()
            frontier = ctx.matrix_from_result(nx, n)
            visited = ctx.matrix_from_result(vx, n)
            nx.free()
            vrp, vci = vx.download()
            vx.free()
            exp_v = [np.flatnonzero(level[s] >= 0) for s in range(S)]
            assert np.array_equal(vrp, np.cumsum([0] + [v.size for v in exp_v])), d
            assert np.array_equal(vci, np.concatenate(exp_v)), d
    finally:
        for h in (A, frontier, visited):
            h.free()
    G = csr_matrix((np.ones(ci.size), ci, rp), shape=(n, n))
    dist = shortest_path(G, directed=True, unweighted=True, indices=sources)
    exp = np.where(np.isinf(dist), -1, dist).astype(np.int64)
    assert level.max() >= 3
    assert np.array_equal(level, exp)


# ---------------------------------------------------------------- one large product ------------------------------
def test_accumulate_rmat18_d_equals_a(ctx):
    rp, ci, n = bspgemm.gen_rmat(18, 16, (0.45, 0.15, 0.15), seed=5701)       # the benchmark's mild skew (bench.py RMAT_MILD)
    want = O.spgemm(rp, ci, rp, ci, n)
    A = ctx.upload(rp, ci, n)
    try:
        got, st = _run(ctx, A, A, A)
    finally:
        A.free()
    exp = accumulate_ref(want, rp, ci, n)
    assert exp[1].size > want[1].size
    assert st["flow"] == 1 and st["small_path"] == 0 and st["nnz_c"] == exp[1].size
    assert _diff(got, exp) is None
