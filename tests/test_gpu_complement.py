"""The complemented-mask product C = !F .* (A*B) (bspgemm_multiply_masked_ex with BSPGEMM_MASK_COMPLEMENT,
Context.multiply_masked(..., complement=True)), bit for bit against the CPU oracle's product minus F, row by row.

Every shape runs with two masks: a random one (unsorted rows, repeats, half of the product's columns, columns beyond B's)
and F = A.  Per shape also: an empty mask gives the plain product, F = pattern(A*B) an empty result, and the masked and the
complemented product of the same F are disjoint with the product as their union.  The launch is asserted from the stats:
upper-bound flow, no small path, and the rows per class of the unmasked product -- so the drop twin of every class that the
shape populates really ran.  Then the knobs, row ranges, errors, a multi-source BFS and one large product.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
from oracle import oracle as O

pytestmark = pytest.mark.gpu
RANK_BIN, MID_BIN, DENSE_BIN = gen.RANK_BIN, gen.MID_BIN, gen.DENSE_BIN
ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- reference ---------------------------------------
def _keys(rp, ci, r0=0):
    rows = np.repeat(np.arange(r0, r0 + rp.size - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    return (rows << 32) | np.asarray(ci, np.int64)


def complement_ref(want, f_rp, f_ci):
    """the oracle's product minus F: (row_ptr int64, col_idx)"""
    rp, ci = want
    R = rp.size - 1
    kc = _keys(rp, ci)
    keep = ~np.isin(kc, _keys(f_rp, f_ci))
    counts = np.bincount((kc[keep] >> 32).astype(np.int64), minlength=R)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(ci)[keep]


def random_mask(rng, R, cols, want, beyond=1000):
    """half of the product's entries (some twice), three random columns per row of which some lie beyond B's columns
    (up to cols + beyond), all in random order within their rows"""
    rp, ci = want
    rows_c = np.repeat(np.arange(R, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    pick = rng.random(ci.size) < 0.5
    r1, c1 = rows_c[pick], np.asarray(ci, np.int64)[pick]
    twice = rng.random(r1.size) < 0.2
    r3 = rng.integers(0, R, size=3 * R)
    c3 = rng.integers(0, cols + beyond, size=r3.size)
    rows = np.concatenate([r1, r1[twice], r3])
    cols_ = np.concatenate([c1, c1[twice], c3])
    perm = rng.permutation(rows.size)
    return gen._csr_from_pairs(rows[perm], cols_[perm], R, dedup=False, sort=False)


def _slice(res, r0, r1):
    rp, ci = res
    return rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]]


def _diff(got, exp):
    (grp, gci), (erp, eci) = got, exp
    if grp.shape != erp.shape or not np.array_equal(grp, erp):
        return "row_ptr differs (first rows %s)" % (np.flatnonzero(grp != erp)[:5] if grp.shape == erp.shape else "shape")
    if not np.array_equal(gci, eci):
        return "col_idx differs (first at %s)" % (np.flatnonzero(gci != eci)[:5] if gci.shape == eci.shape else "nnz %d != %d" % (gci.size, eci.size))
    return None


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.array([c for r in rows for c in r], dtype=np.int32)


# ---------------------------------------------------------------- shapes: (a_rp, a_ci, b_rp, b_ci, ncols) -------------
def _uniform():
    rp, ci, n = gen.uniform(3000, 8, 5101)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, scipy=True)


def _class_boundaries():
    a_rp, a_ci, b_rp, b_ci = gen.class_boundary_rows(repeat=1, seed=1301)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=6000, need=list(range(1, 17)) + [MID_BIN, DENSE_BIN])


def _rank(ncols, seed):
    a_rp, a_ci, b_rp, b_ci = gen.rank_rows(ncols, [2049, 4097, 6144, 6145, 3000, 5000] * 3, short_rows=(4, 10), ones_rows=(5,),
                                           seed=seed, counts=(6000, 1000, 100))
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols, need=[RANK_BIN, MID_BIN])


def _tiny_b_heavy(nnzb):
    a_rp, a_ci, b_rp, b_ci = gen.tiny_b_heavy(nnzb)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=11, need=[MID_BIN])


def _rmat13_skewed():
    rp, ci, n = gen.rmat(13, 16, (0.57, 0.19, 0.19, 0.05), 1601)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, need=list(range(1, 17)) + [MID_BIN])


def _rmat14_skewed_wide():
    """skewed R-MAT A times the same pattern spread over 2^21 columns: hub rows over eight windows of the small shape and
    two of the hub shape, the rank class and every one-wave class"""
    rp, ci, n = gen.rmat(14, 16, (0.57, 0.19, 0.19, 0.05), 1602)
    rows = np.repeat(np.arange(n), np.diff(rp))
    b_ci = (ci.astype(np.int64) * 128 + (rows * 37) % 128).astype(np.int32)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=b_ci, ncols=1 << 21, need=list(range(1, 17)) + [RANK_BIN, MID_BIN, DENSE_BIN])


def _powerlaw():
    rp, ci, n = gen.powerlaw(20000, 8, 77)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, scipy=True, need=list(range(1, 17)) + [MID_BIN])


W40 = 40_000_000


def _tiny_b_wide():
    """B of 3 nonzeros over 40 M columns (LEVELS 4); A row 0 has 5000 repeated entries: a hub row over 39 windows"""
    b_rp, b_ci = _csr([[W40 - 2], [4, W40 - 1], []])
    rng = np.random.default_rng(1103)
    a_rp, a_ci = _csr([list(rng.integers(0, 3, size=5000))] + [[2], [1], [0, 2], [1, 2, 0], [], [2, 2], [1]])
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=W40, need=[DENSE_BIN])


def _five_levels():
    ncols = 300_000_000
    a_rp, a_ci = gen.uniform_rect(300, 400, 5, seed=1501)
    rng = np.random.default_rng(1502)
    rows = np.repeat(np.arange(400), 20)
    cols = np.concatenate([rng.integers(0, ncols, size=4000), rng.integers(ncols - 3000, ncols, size=4000)])
    b_rp, b_ci = gen._csr_from_pairs(rows, cols, 400)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols)


def _one_level():
    """1000 columns (LEVELS 1: the top bitmap is the column bitmap), rows of 20 to 2000 products"""
    a_rp, a_ci = gen.uniform_rect(2000, 500, 6, seed=1503)
    rng = np.random.default_rng(1504)
    lens = rng.integers(1, 60, size=500)
    b_rp, b_ci = gen._csr_from_pairs(np.repeat(np.arange(500), lens), rng.integers(0, 1000, size=int(lens.sum())), 500)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=1000, scipy=True)


def _wave_case(cols):
    s = gen.wave_rows_case(cols, {b: 420 for b in range(1, 17)}, seed=5200 + cols % 97)
    return dict(a_rp=s["a_rp"], a_ci=s["a_ci"], b_rp=s["b_rp"], b_ci=s["b_ci"], ncols=cols, need=list(range(1, 17)))


SHAPES = {
    "uniform": _uniform,
    "class_boundaries": _class_boundaries,
    "rank_700k": lambda: _rank(700_001, 7001),
    "rank_5M_spans": lambda: _rank(5_000_000, 7002),
    "tiny_b_heavy_nnz3": lambda: _tiny_b_heavy(3),
    "tiny_b_heavy_nnz5": lambda: _tiny_b_heavy(5),
    "rmat13_skewed": _rmat13_skewed,
    "rmat14_skewed_wide": _rmat14_skewed_wide,
    "powerlaw": _powerlaw,
    "tiny_b_wide_40M": _tiny_b_wide,
    "five_levels_300M": _five_levels,
    "one_level_1000": _one_level,
    **{"wave_rows_cols%d" % c: (lambda c=c: _wave_case(c)) for c in (4096, 131073, 4194305, 16777217, 268435457)},
}
_cache = {}


def _shape(name):
    if name not in _cache:
        s = SHAPES[name]()
        for k in ("a_rp", "a_ci", "b_rp", "b_ci"):
            s[k] = np.ascontiguousarray(s[k], np.int32)
        s["want"] = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], s["ncols"])
        _cache.clear()
        _cache[name] = s
    return _cache[name]


def _upload(ctx, s):
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], s["ncols"])
    return A, B


def _run(ctx, A, B, Fm, r0=0, r1=None, complement=True):
    C = ctx.multiply_masked(A, B, Fm, r0, r1, complement=complement)
    st = ctx.stats()
    got = C.download()
    C.free()
    return got, st


# ---------------------------------------------------------------- 1-3: shapes, identities, classes -----------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_complement_shape(ctx, name):
    s = _shape(name)
    want = s["want"]
    R = s["a_rp"].size - 1
    cols = s["ncols"]
    F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)
    bins = gen.expected_bins(F, cols)
    assert all(bins[b] > 0 for b in s.get("need", [])), bins
    rng = np.random.default_rng(R + cols % 1009)
    masks = {"random": random_mask(rng, R, cols, want), "F=A": (s["a_rp"], s["a_ci"]),
             "empty": (np.zeros(R + 1, np.int32), np.zeros(0, np.int32)),
             "F=pattern(A*B)": (want[0].astype(np.int32), want[1])}
    ctx.set_flow("auto")
    for k, v in (("small_path", -1), ("padded_rows", -1), ("blocked_extents", -1), ("check", 0), ("class_streams", 2)):
        ctx.set_option(k, v)
    A, B = _upload(ctx, s)
    failures = []
    try:
        # the unmasked product's launch, on the general flow, is what the complemented one must repeat
        ctx.set_option("small_path", 0)
        ctx.set_flow("upper-bound")
        Cm = ctx.multiply(A, B)
        st_mul = ctx.stats()
        Cm.free()
        ctx.set_option("small_path", -1)
        ctx.set_flow("auto")
        assert st_mul["rows_per_bin"] == bins, (st_mul["rows_per_bin"], bins)
        # masked(F) and complemented(F) split the product: for a mask within B's columns, for one whose extra columns start
        # where the one-wave masked kernel's top bitmap ends, and (below) for the random mask with columns up to B.cols + 1000
        top = 256 << (5 * gen.mask_levels(cols)) if gen.mask_levels(cols) else cols
        f_in = random_mask(rng, R, cols, want, beyond=0)
        far_rows = rng.integers(0, R, size=3 * R)
        far_cols = np.concatenate([np.full(R, top), rng.integers(top, min(4 * top, gen.INT_MAX), size=R),
                                   rng.integers(top, gen.INT_MAX, size=R)])
        all_rows = np.concatenate([np.repeat(np.arange(R, dtype=np.int64), np.diff(f_in[0])), far_rows])
        perm = rng.permutation(all_rows.size)
        f_far = gen._csr_from_pairs(all_rows[perm], np.concatenate([f_in[1].astype(np.int64), far_cols])[perm], R,
                                    dedup=False, sort=False)      # (the in-range mask's entries and the far columns)
        wk = _keys(*want)

        def split(sname, f_rp, f_ci, comp, kept):
            """comp = the product minus F, kept = the product within F, and the two results themselves are disjoint and make up
            the product (one np.isin for both references, one sort for the identity)"""
            inside = np.isin(wk, _keys(f_rp, f_ci))
            for what, got, sel in (("", comp, ~inside), (", masked product", kept, inside)):
                counts = np.bincount((wk[sel] >> 32).astype(np.int64), minlength=R)
                bad = _diff(got, (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(want[1])[sel]))
                if bad:
                    failures.append("%s mask%s: %s" % (sname, what, bad))
            both = np.sort(np.concatenate([_keys(*kept), _keys(*comp)]))
            if np.any(both[1:] == both[:-1]):
                failures.append("%s mask: masked and complemented product share entries" % sname)
            elif not np.array_equal(both, wk):
                failures.append("%s mask: masked and complemented product do not make up the product" % sname)

        for sname, (f_rp, f_ci), fcols in (("in-range", f_in, cols),
                                           ("beyond the top bitmap", f_far, gen.INT_MAX)):
            Fm = ctx.upload(f_rp, f_ci, fcols)
            try:
                comp, _ = _run(ctx, A, B, Fm)
                kept, _ = _run(ctx, A, B, Fm, complement=False)
            finally:
                Fm.free()
            split(sname, f_rp, f_ci, comp, kept)
        for mname, (f_rp, f_ci) in masks.items():
            Fm = ctx.upload(f_rp, f_ci, cols + 1000)
            try:
                got, st = _run(ctx, A, B, Fm)
                if mname == "random":                       # (columns up to B.cols + 1000: the split once more)
                    split(mname, f_rp, f_ci, got, _run(ctx, A, B, Fm, complement=False)[0])
                exp = complement_ref(want, f_rp, f_ci)
                if mname == "empty":
                    exp = (want[0].astype(np.int64), want[1])
                elif mname == "F=pattern(A*B)":
                    if not (got[1].size == 0 and not got[0].any()):
                        failures.append("%s: nnz %d, row_ptr not all zero" % (mname, got[1].size))
                bad = _diff(got, exp)
                if bad:
                    failures.append("mask %s: %s" % (mname, bad))
                path = dict(flow=st["flow"], small_path=st["small_path"], rows_per_bin=st["rows_per_bin"], bin_cap=st["bin_cap"],
                            products=st["products"])
                exp_path = dict(flow=1, small_path=0, rows_per_bin=st_mul["rows_per_bin"], bin_cap=gen.expected_bin_caps(cols),
                                products=int(F.sum()))
                if path != exp_path:
                    failures.append("mask %s: path %s, expected %s" % (mname, path, exp_path))
                if mname == "random" and s.get("scipy"):
                    import scipy.sparse as sp
                    nb = s["b_rp"].size - 1
                    As = sp.csr_matrix((np.ones(s["a_ci"].size), s["a_ci"], s["a_rp"]), shape=(R, nb))
                    Bs = sp.csr_matrix((np.ones(s["b_ci"].size), s["b_ci"], s["b_rp"]), shape=(nb, cols))
                    P = (As @ Bs).tocoo()
                    pk = (P.row.astype(np.int64) << 32) | P.col.astype(np.int64)
                    pk = np.unique(pk[P.data > 0])
                    ref = pk[~np.isin(pk, _keys(f_rp, f_ci))]
                    if not np.array_equal(ref, _keys(*got)):
                        failures.append("differs from scipy's (A @ B > 0) minus F")
            finally:
                Fm.free()
    finally:
        A.free()
        B.free()
    assert not failures, "%s:\n  %s" % (name, "\n  ".join(failures))


# ---------------------------------------------------------------- 4: knobs and ranges -------------------------------
@pytest.mark.parametrize("name", ["rmat14_skewed_wide", "tiny_b_wide_40M", "class_boundaries"])
def test_complement_knobs_and_ranges(ctx, name):
    """padded_rows x blocked_extents x check x class_streams, each over the whole A, an interior range, one row and none"""
    s = _shape(name)
    want = s["want"]
    R = s["a_rp"].size - 1
    f_rp, f_ci = random_mask(np.random.default_rng(31), R, s["ncols"], want)
    exp = complement_ref(want, f_rp, f_ci)
    nnz_b = int(s["b_rp"][-1])
    ctx.set_flow("auto")
    ctx.set_option("small_path", -1)
    Fm = ctx.upload(f_rp, f_ci, s["ncols"] + 1000)
    failures, runs = [], 0
    try:
        for k, (pad, blk, chk, cs) in enumerate(np.ndindex(2, 2, 2, 2)):
            cs = 1 + 2 * cs
            for opt, v in (("padded_rows", pad), ("blocked_extents", blk), ("check", chk), ("class_streams", cs)):
                ctx.set_option(opt, v)
            A, B = _upload(ctx, s)
            try:
                heavy = int(np.argmax(gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)))
                # interior: starts at or before the middle row, ends after it (a valid range for any R >= 2, also R = 8)
                inner = (min(R // 7 + k, R // 2), max(R - R // 5 - k, R // 2 + 1))
                for r0, r1 in ((0, R), inner, (heavy, heavy + 1), (R // 2, R // 2)):
                    got, st = _run(ctx, A, B, Fm, r0, r1)
                    runs += 1
                    tag = "padded_rows=%d blocked_extents=%d check=%d class_streams=%d rows=[%d,%d)" % (pad, blk, chk, cs, r0, r1)
                    bad = _diff(got, _slice(exp, r0, r1))
                    if bad:
                        failures.append("%s: %s" % (tag, bad))
                    if r1 > r0:
                        p = {k2: st[k2] for k2 in ("flow", "small_path", "padded_rows", "prepass_kernel", "checked", "class_streams")}
                        e = dict(flow=1, small_path=0, padded_rows=int(pad == 1 and nnz_b > 0), prepass_kernel=blk, checked=chk,
                                 class_streams=cs)
                        if p != e:
                            failures.append("%s: path %s, expected %s" % (tag, p, e))
            finally:
                A.free()
                B.free()
    finally:
        Fm.free()
        for opt, v in (("padded_rows", -1), ("blocked_extents", -1), ("check", 0), ("class_streams", 2)):
            ctx.set_option(opt, v)
    assert not failures, "%s: %d of %d runs wrong:\n  %s" % (name, len(failures), runs, "\n  ".join(failures))


# ---------------------------------------------------------------- 5: errors and compatibility -----------------------
def test_complement_errors_and_flags_zero(ctx):
    rp, ci, n = gen.uniform(700, 6, 5301)
    A = ctx.upload(rp, ci, n)
    # (within B's columns: the masked ORACLE, which flags columns in an array of n entries, is compared below)
    f_rp, f_ci = random_mask(np.random.default_rng(5), n, n, O.spgemm(rp, ci, rp, ci, n), beyond=0)
    Fm = ctx.upload(f_rp, f_ci, n)
    short = ctx.upload(rp[:301], ci[:rp[300]], n)
    L = bspgemm.lib()
    try:
        for flags, F, r1 in ((2, Fm, n), (3, Fm, n), (0x80000000, Fm, n), (1, short, n), (1, short, 301)):
            out = C.c_void_p(1)
            st = L.bspgemm_multiply_masked_ex(ctx._h, A._h, A._h, F._h, flags, 0, r1, C.byref(out))
            assert st == ERR_INVALID and not out.value, (flags, r1, st)
        out = C.c_void_p(1)
        assert L.bspgemm_multiply_masked_ex(ctx._h, A._h, A._h, None, 1, 0, n, C.byref(out)) == ERR_INVALID
        # a mask of exactly row_end rows is enough
        got, _ = _run(ctx, A, A, short, 0, 300)
        want = O.spgemm(rp, ci, rp, ci, n)
        assert _diff(got, _slice(complement_ref(want, rp[:301], ci[:rp[300]]), 0, 300)) is None
        # flags = 0 is the masked product
        r = C.c_void_p()
        assert L.bspgemm_multiply_masked_ex(ctx._h, A._h, A._h, Fm._h, 0, 0, n, C.byref(r)) == 0
        ex = bspgemm.Result(ctx, r)
        got0 = ex.download()
        ex.free()
        ref, _ = _run(ctx, A, A, Fm, complement=False)
        assert _diff(got0, ref) is None
        assert _diff(ref, _slice(O.spgemm_masked(rp, ci, rp, ci, n, f_rp, f_ci), 0, n)) is None
    finally:
        for h in (A, Fm, short):
            h.free()


# ---------------------------------------------------------------- 6: multi-source BFS -------------------------------
def _bfs_levels(ctx, rp, ci, n, sources):
    """next = (frontier * A) and not visited, on the device; frontier and visited kept on the host"""
    S = len(sources)
    A = ctx.upload(rp, ci, n)
    level = np.full((S, n), -1, np.int64)
    level[np.arange(S), sources] = 0
    frontier = [[s] for s in sources]
    d = 0
    try:
        while any(len(f) for f in frontier):
            d += 1
            f_rp, f_ci = _csr(frontier)
            v_rp, v_ci = _csr([np.flatnonzero(level[s] >= 0) for s in range(S)])
            Fr = ctx.upload(f_rp, f_ci, n)
            V = ctx.upload(v_rp, v_ci, n)
            try:
                C_ = ctx.multiply_masked(Fr, A, V, complement=True)
                nrp, nci = C_.download()
                C_.free()
            finally:
                Fr.free()
                V.free()
            frontier = [nci[nrp[s]:nrp[s + 1]] for s in range(S)]
            for s in range(S):
                assert (level[s, frontier[s]] < 0).all(), "a visited vertex came back"
                level[s, frontier[s]] = d
    finally:
        A.free()
    return level


@pytest.mark.parametrize("graph", ["rmat12", "powerlaw"])
def test_multi_source_bfs(ctx, graph):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    if graph == "rmat12":
        rp, ci, n = gen.rmat(12, 8, (0.57, 0.19, 0.19, 0.05), 5401)
    else:
        rp, ci, n = gen.powerlaw(6000, 3, 5402)
    sources = np.random.default_rng(9).choice(n, size=8, replace=False)
    level = _bfs_levels(ctx, rp, ci, n, sources)
    G = csr_matrix((np.ones(ci.size), ci, rp), shape=(n, n))
    dist = shortest_path(G, directed=True, unweighted=True, indices=sources)
    exp = np.where(np.isinf(dist), -1, dist).astype(np.int64)
    assert level.max() >= 3
    assert np.array_equal(level, exp)


# ---------------------------------------------------------------- 7: one large product ------------------------------
def test_complement_rmat18_f_equals_a(ctx):
    rp, ci, n = bspgemm.gen_rmat(18, 16, (0.45, 0.15, 0.15), seed=5501)       # the benchmark's mild skew (bench.py RMAT_MILD)
    want = O.spgemm(rp, ci, rp, ci, n)
    A = ctx.upload(rp, ci, n)
    try:
        got, st = _run(ctx, A, A, A)
    finally:
        A.free()
    exp = complement_ref(want, rp, ci)
    assert exp[1].size > 0
    assert st["flow"] == 1 and st["small_path"] == 0
    assert _diff(got, exp) is None
