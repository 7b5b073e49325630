"""The counting masked product C = F .* (A*B) with path counts (bspgemm_multiply_masked_count,
Context.multiply_masked_count), complete results compared: the pattern bit for bit with bspgemm_multiply_masked on the same
arguments, the values with the reference count -- A1 @ B1 with a 1 per stored entry (repeats not merged), restricted to
pattern(F) within [0, B.cols).  The reference is cross-checked against scipy on the small shapes.

Every shape runs with a random mask (unsorted rows, repeats, columns beyond B's), the same within B's columns, F = A,
F = pattern(A*B) (each row's counts then sum to its product count) and an empty mask.  For every mask the pattern and
rows_per_bin must equal the masked product's on the same arguments, so the counting twin of every class ran.  Then counts
above 16 bits, the int32 refusal, ranges and knobs, graph identities (triangles, support), errors and
the result object.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen

pytestmark = pytest.mark.gpu
RANK_BIN, MID_BIN, DENSE_BIN = gen.RANK_BIN, gen.MID_BIN, gen.DENSE_BIN
ERR_INVALID, ERR_OVERFLOW = 1, 5


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- reference ---------------------------------------
def expand(a_rp, a_ci, b_rp, b_ci, r0=0, r1=None):
    """every product (i, j) of rows [r0, r1), repeats of A and B included, counted: (sorted keys i << 32 | j, counts)"""
    r1 = a_rp.size - 1 if r1 is None else r1
    a_rp, b_rp = np.asarray(a_rp, np.int64), np.asarray(b_rp, np.int64)
    p0, p1 = a_rp[r0], a_rp[r1]
    arow = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(a_rp[r0:r1 + 1]))
    k = np.asarray(a_ci[p0:p1], np.int64)
    starts, lens = b_rp[k], b_rp[k + 1] - b_rp[k]
    tot = int(lens.sum())
    excl = np.repeat(np.cumsum(lens) - lens, lens)
    idx = np.arange(tot, dtype=np.int64) - excl + np.repeat(starts, lens)
    keys = (np.repeat(arow, lens) << 32) | np.asarray(b_ci, np.int64)[idx]
    return np.unique(keys, return_counts=True)


def count_ref(a_rp, a_ci, b_rp, b_ci, f_rp, f_ci, cols, r0=0, r1=None, prod=None):
    """the expanded products kept where j is a column of F's row i below cols: (row_ptr int64 slice-local, col_idx, values)"""
    r1 = a_rp.size - 1 if r1 is None else r1
    uk, cnt = expand(a_rp, a_ci, b_rp, b_ci, r0, r1) if prod is None else prod
    f_rp = np.asarray(f_rp, np.int64)
    frow = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(f_rp[r0:r1 + 1]))
    fc = np.asarray(f_ci[f_rp[r0]:f_rp[r1]], np.int64)
    ok = (fc >= 0) & (fc < cols)
    keep = np.isin(uk, np.unique((frow[ok] << 32) | fc[ok]))
    uk, cnt = uk[keep], cnt[keep]
    counts = np.bincount((uk >> 32) - r0, minlength=r1 - r0)
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return rp, (uk & 0xFFFFFFFF).astype(np.int32), cnt.astype(np.int32)


def scipy_ref(a_rp, a_ci, b_rp, b_ci, f_rp, f_ci, cols):
    """A1 @ B1 (a 1 per stored entry, duplicates not merged) restricted to pattern(F) within [0, cols), as sorted keys + values"""
    import scipy.sparse as sp
    R, nb = a_rp.size - 1, b_rp.size - 1
    As = sp.csr_matrix((np.ones(a_ci.size, np.int64), a_ci, a_rp), shape=(R, nb))
    Bs = sp.csr_matrix((np.ones(b_ci.size, np.int64), b_ci, b_rp), shape=(nb, cols))
    P = (As @ Bs).tocoo()
    pk = (P.row.astype(np.int64) << 32) | P.col.astype(np.int64)
    o = np.argsort(pk)
    pk, pv = pk[o], P.data[o]
    frow = np.repeat(np.arange(R, dtype=np.int64), np.diff(np.asarray(f_rp, np.int64)))
    fc = np.asarray(f_ci, np.int64)
    ok = (fc >= 0) & (fc < cols)
    keep = np.isin(pk, (frow[ok] << 32) | fc[ok]) & (pv > 0)
    return pk[keep], pv[keep]


def _keys(rp, ci):
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    return (rows << 32) | np.asarray(ci, np.int64)


def random_mask(rng, R, cols, a_rp, a_ci, beyond=1000):
    """about half of each row's columns of A plus B-range noise: unsorted rows, repeats, columns up to cols + beyond"""
    rows_a = np.repeat(np.arange(R, dtype=np.int64), np.diff(np.asarray(a_rp, np.int64)))
    pick = rng.random(a_ci.size) < 0.5
    r1, c1 = rows_a[pick], np.asarray(a_ci, np.int64)[pick]
    twice = rng.random(r1.size) < 0.2
    r3 = rng.integers(0, R, size=4 * R)
    c3 = rng.integers(0, cols + beyond, size=r3.size)
    rows = np.concatenate([r1, r1[twice], r3])
    cc = np.concatenate([c1, c1[twice], c3])
    perm = rng.permutation(rows.size)
    return gen._csr_from_pairs(rows[perm], cc[perm], R, dedup=False, sort=False)


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.array([c for r in rows for c in r], dtype=np.int32)


# ---------------------------------------------------------------- shapes: (a_rp, a_ci, b_rp, b_ci, ncols) -------------
def _uniform():
    rp, ci, n = gen.uniform(3000, 8, 5101)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, scipy=True)


def _class_boundaries():
    a_rp, a_ci, b_rp, b_ci = gen.class_boundary_rows(repeat=1, seed=1301)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=6000, scipy=True)


def _rank(ncols, seed):
    a_rp, a_ci, b_rp, b_ci = gen.rank_rows(ncols, [2049, 4097, 6144, 6145, 3000, 5000] * 3, short_rows=(4, 10), ones_rows=(5,),
                                           seed=seed, counts=(6000, 1000, 100))
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols)


def _rmat13_skewed():
    rp, ci, n = gen.rmat(13, 16, (0.57, 0.19, 0.19, 0.05), 1601)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, scipy=True)


def _rmat14_skewed_wide():
    rp, ci, n = gen.rmat(14, 16, (0.57, 0.19, 0.19, 0.05), 1602)
    rows = np.repeat(np.arange(n), np.diff(rp))
    b_ci = (ci.astype(np.int64) * 128 + (rows * 37) % 128).astype(np.int32)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=b_ci, ncols=1 << 21)


def _powerlaw():
    rp, ci, n = gen.powerlaw(20000, 8, 77)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, scipy=True)


def _dups_unsorted():
    rp, ci, n = gen.dups_unsorted(4000, 12, 91)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, scipy=True)


W40 = 40_000_000


def _tiny_b_wide():
    """B of 3 nonzeros over 40 M columns: cols > 2^23 sends every row to the window twin"""
    b_rp, b_ci = _csr([[W40 - 2], [4, W40 - 1], []])
    rng = np.random.default_rng(1103)
    a_rp, a_ci = _csr([list(rng.integers(0, 3, size=5000))] + [[2], [1], [0, 2], [1, 2, 0], [], [2, 2], [1]])
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=W40)


def _wide_uniform():
    """uniform rows over 12 M columns (> 2^23): the window twin for rows of every size"""
    ncols = 12_000_000
    a_rp, a_ci = gen.uniform_rect(3000, 2000, 6, seed=1505)
    rng = np.random.default_rng(1506)
    lens = rng.integers(1, 40, size=2000)
    b_rp, b_ci = gen._csr_from_pairs(np.repeat(np.arange(2000), lens), rng.integers(0, ncols, size=int(lens.sum())), 2000)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols)


def _one_level():
    a_rp, a_ci = gen.uniform_rect(2000, 500, 6, seed=1503)
    rng = np.random.default_rng(1504)
    lens = rng.integers(1, 60, size=500)
    b_rp, b_ci = gen._csr_from_pairs(np.repeat(np.arange(500), lens), rng.integers(0, 1000, size=int(lens.sum())), 500)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=1000, scipy=True)


def _dense_window():
    """a row whose mask holds far more distinct columns in one 2^18-column window than a window has counters (20480): the
    window twin narrows its windows; other rows spread over 2^20 columns"""
    ncols = 1 << 20
    rng = np.random.default_rng(1701)
    nb = 400
    lens = rng.integers(100, 400, size=nb)
    b_rows = np.repeat(np.arange(nb), lens)
    b_cols = np.where(rng.random(b_rows.size) < 0.8, rng.integers(0, 120_000, size=b_rows.size),
                      rng.integers(0, ncols, size=b_rows.size))
    b_rp, b_ci = gen._csr_from_pairs(b_rows, b_cols, nb, dedup=False, sort=False)
    rows = [list(range(nb)) + list(rng.integers(0, nb, size=50))] + [list(rng.integers(0, nb, size=int(rng.integers(1, 30))))
                                                                       for _ in range(300)]
    a_rp, a_ci = _csr(rows)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols,
                extra_mask=(0, np.concatenate([rng.integers(0, 120_000, size=60_000), rng.integers(0, ncols, size=20_000)])))


def _unaligned(ncols, dense_lo, seed):
    """B.cols not a multiple of 32, and a hub row whose mask covers every column of [dense_lo, ncols) (more than a window has
    counters): the window twin narrows windows, the last one clamped to the last column, so a narrowed window may begin
    inside a 32-column word; products fall mostly into the dense range"""
    rng = np.random.default_rng(seed)
    nb = 300
    lens = rng.integers(100, 300, size=nb)
    b_rows = np.repeat(np.arange(nb), lens)
    b_cols = np.where(rng.random(b_rows.size) < 0.8, rng.integers(dense_lo, ncols, size=b_rows.size),
                      rng.integers(0, ncols, size=b_rows.size))
    b_rp, b_ci = gen._csr_from_pairs(b_rows, b_cols, nb, dedup=False, sort=False)
    rows = [list(range(nb)) + list(rng.integers(0, nb, size=50))] + [list(rng.integers(0, nb, size=int(rng.integers(1, 30))))
                                                                       for _ in range(200)]
    a_rp, a_ci = _csr(rows)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols, extra_mask=(0, np.arange(dense_lo, ncols)))


def _wave_case(cols):
    s = gen.wave_rows_case(cols, {b: 420 for b in range(1, 17)}, seed=5200 + cols % 97)
    return dict(a_rp=s["a_rp"], a_ci=s["a_ci"], b_rp=s["b_rp"], b_ci=s["b_ci"], ncols=cols)


SHAPES = {
    "uniform": _uniform,
    "class_boundaries": _class_boundaries,
    "rank_700k": lambda: _rank(700_001, 7001),
    "rmat13_skewed": _rmat13_skewed,
    "rmat14_skewed_wide": _rmat14_skewed_wide,
    "powerlaw": _powerlaw,
    "dups_unsorted": _dups_unsorted,
    "tiny_b_wide_40M": _tiny_b_wide,
    "wide_uniform_12M": _wide_uniform,
    "one_level_1000": _one_level,
    "dense_window": _dense_window,
    "unaligned_300001": lambda: _unaligned(300_001, 200_000, 1801),
    "unaligned_100001": lambda: _unaligned(100_001, 40_000, 1802),
    **{"wave_rows_cols%d" % c: (lambda c=c: _wave_case(c)) for c in (4096, 131073, 4194305)},
}
_cache = {}


def _shape(name):
    if name not in _cache:
        s = SHAPES[name]()
        for k in ("a_rp", "a_ci", "b_rp", "b_ci"):
            s[k] = np.ascontiguousarray(s[k], np.int32)
        _cache.clear()
        _cache[name] = s
    return _cache[name]


def _upload(ctx, s):
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], s["ncols"])
    return A, B


def _count(ctx, A, B, Fm, r0=0, r1=None):
    Cr = ctx.multiply_masked_count(A, B, Fm, r0, r1)
    st = ctx.stats()
    rp, ci = Cr.download()
    v = Cr.download_values()
    assert Cr.values_device
    Cr.free()
    return (rp, ci, v), st


def _masked(ctx, A, B, Fm, r0=0, r1=None):
    Cr = ctx.multiply_masked(A, B, Fm, r0, r1)
    st = ctx.stats()
    got = Cr.download()
    Cr.free()
    return got, st


def _diff(got, exp):
    for what, g, e in zip(("row_ptr", "col_idx", "values"), got, exp):
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape:
            return "%s: %d entries, expected %d" % (what, g.size, e.size)
        if not np.array_equal(g, e):
            return "%s differs (first at %s)" % (what, np.flatnonzero(g != e)[:5])
    return None


# ---------------------------------------------------------------- shapes x masks ------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_count_shape(ctx, name):
    s = _shape(name)
    R, cols = s["a_rp"].size - 1, s["ncols"]
    rng = np.random.default_rng(R + cols % 1009)
    masks = {"random": random_mask(rng, R, cols, s["a_rp"], s["a_ci"]), "F=A": (s["a_rp"], s["a_ci"]),
             "random in range": random_mask(rng, R, cols, s["a_rp"], s["a_ci"], beyond=0),
             "empty": (np.zeros(R + 1, np.int32), np.zeros(0, np.int32))}
    if "extra_mask" in s:                           # one row's mask with many more columns than a window has counters
        row, extra = s["extra_mask"]
        f_rp, f_ci = masks["random"]
        rows = np.repeat(np.arange(R), np.diff(f_rp)).astype(np.int64)
        masks["dense"] = gen._csr_from_pairs(np.concatenate([rows, np.full(extra.size, row)]),
                                             np.concatenate([f_ci.astype(np.int64), extra]), R, dedup=False, sort=False)
        assert np.unique(extra).size > 20480
    ctx.set_flow("auto")
    for k, v in (("small_path", -1), ("padded_rows", -1), ("blocked_extents", -1), ("check", 0), ("class_streams", 2)):
        ctx.set_option(k, v)
    A, B = _upload(ctx, s)
    failures = []
    try:
        # F = pattern(A*B): every product lands on the mask, so each row's counts sum to its product count
        Cp = ctx.multiply(A, B)
        masks["F=pattern(A*B)"] = tuple(x.astype(np.int32) for x in Cp.download())
        Cp.free()
        prefix = ctx.row_work_prefix(A, B)
        prod = expand(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"])
        for mname, (f_rp, f_ci) in masks.items():
            Fm = ctx.upload(f_rp, f_ci, cols + 1000)
            try:
                got, st = _count(ctx, A, B, Fm)
                ref, st_m = _masked(ctx, A, B, Fm)
            finally:
                Fm.free()
            if _diff(got[:2], ref):
                failures.append("mask %s: pattern differs from the masked product: %s" % (mname, _diff(got[:2], ref)))
            if st["rows_per_bin"] != st_m["rows_per_bin"] or st["bin_cap"] != st_m["bin_cap"]:
                failures.append("mask %s: classes %s, masked product %s" % (mname, st["rows_per_bin"], st_m["rows_per_bin"]))
            path = {k: st[k] for k in ("flow", "small_path", "products", "nnz_c")}
            if path != dict(flow=1, small_path=0, products=int(prefix[-1]), nnz_c=int(got[1].size)):
                failures.append("mask %s: path %s" % (mname, path))
            exp = count_ref(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], f_rp, f_ci, cols, prod=prod)
            bad = _diff(got, exp)
            if bad:
                failures.append("mask %s: %s" % (mname, bad))
            if mname == "empty" and got[1].size:
                failures.append("empty mask: %d entries" % got[1].size)
            if mname == "F=pattern(A*B)":
                sums = np.zeros(R, np.int64)
                np.add.at(sums, np.repeat(np.arange(R), np.diff(got[0])), got[2].astype(np.int64))
                if not np.array_equal(sums, np.diff(prefix)):
                    failures.append("F=pattern(A*B): row sums differ from the product counts at rows %s"
                                    % np.flatnonzero(sums != np.diff(prefix))[:5])
            if s.get("scipy") and mname in ("random", "F=A", "random in range"):
                pk, pv = scipy_ref(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], f_rp, f_ci, cols)
                if not (np.array_equal(pk, _keys(got[0], got[1])) and np.array_equal(pv, got[2])):
                    failures.append("mask %s: differs from scipy's A1 @ B1 under the mask" % mname)
    finally:
        A.free()
        B.free()
    assert not failures, "%s:\n  %s" % (name, "\n  ".join(failures))


def test_shapes_cover_every_counting_kernel():
    """host-side: over the shapes, F = pattern(A*B) puts rows of every mask capacity at every depth of the one-wave twin,
    and the window twin gets rows of long masks, rows of many products and every row of a matrix over 2^23 columns"""
    caps, levels, heavy = set(), set(), set()
    for name in SHAPES:
        s = SHAPES[name]()
        R, cols = s["a_rp"].size - 1, s["ncols"]
        F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)
        if cols > (1 << 23):
            heavy.add("wide")
            continue
        from oracle import oracle as O
        crp, _ = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
        m = np.diff(np.asarray(crp, np.int64))
        one = (F > 0) & (m > 0) & (m <= 2048) & (F <= 8192)
        for lo, hi in ((0, 64), (64, 128), (128, 256), (256, 512), (512, 768), (768, 1024), (1024, 2048)):
            if np.any(one & (m > lo) & (m <= hi)):
                caps.add(hi)
        if one.any():
            levels.add(gen.wave_levels(cols) if cols > 8192 else 1)
        if np.any((F > 0) & (m > 2048)):
            heavy.add("long mask")
        if np.any((m > 0) & (F > 8192)):
            heavy.add("many products")
    assert caps == {64, 128, 256, 512, 768, 1024, 2048}, caps
    assert {1, 2, 3} <= levels, levels
    assert heavy == {"wide", "long mask", "many products"}, heavy


@pytest.mark.parametrize("cols", [1000, 100_000, 5_000_000])
def test_one_wave_mask_columns_beyond_the_top_bitmap(ctx, cols):
    """one-wave rows (short masks, few products) at one, two and three bitmap levels whose masks hold columns far beyond
    B.cols -- at and above 256 * 32^LEVELS, past the top bitmap -- besides product columns: those columns count nothing"""
    levels = 1 if cols <= 8192 else (2 if cols <= (1 << 18) else 3)
    cap = 256 * 32 ** levels
    rng = np.random.default_rng(cols)
    a_rp, a_ci = gen.uniform_rect(2000, 500, 6, seed=1901)
    lens = rng.integers(1, 40, size=500)
    b_rp, b_ci = gen._csr_from_pairs(np.repeat(np.arange(500), lens), rng.integers(0, cols, size=int(lens.sum())), 500)
    uk, cnt = expand(a_rp, a_ci, b_rp, b_ci)
    pick = rng.random(uk.size) < 0.5
    r1, c1 = uk[pick] >> 32, uk[pick] & 0xFFFFFFFF
    r2 = rng.integers(0, 2000, size=6000)
    c2 = np.concatenate([np.full(2000, cap), rng.integers(cols, cap, size=2000), rng.integers(cap, 1 << 30, size=2000)])
    perm = rng.permutation(r1.size + r2.size)
    f_rp, f_ci = gen._csr_from_pairs(np.concatenate([r1, r2])[perm], np.concatenate([c1, c2])[perm], 2000, dedup=False, sort=False)
    assert np.diff(f_rp).max() <= 2048
    A = ctx.upload(a_rp, a_ci, 500)
    B = ctx.upload(b_rp, b_ci, cols)
    Fm = ctx.upload(f_rp, f_ci, (1 << 30) + 1)
    try:
        got, st = _count(ctx, A, B, Fm)
        kept, st_m = _masked(ctx, A, B, Fm)
    finally:
        for h in (A, B, Fm):
            h.free()
    assert sum(st["rows_per_bin"][1:17]) > 0 and not any(st["rows_per_bin"][17:]), st["rows_per_bin"]
    bad = _diff(got, count_ref(a_rp, a_ci, b_rp, b_ci, f_rp, f_ci, cols, prod=(uk, cnt)))
    assert bad is None, bad
    # the masked product on the same arguments: the same pattern from the same classes
    assert _diff(kept, got[:2]) is None, "masked product: %s" % _diff(kept, got[:2])
    assert st_m["rows_per_bin"] == st["rows_per_bin"] and st_m["bin_cap"] == st["bin_cap"]


# ---------------------------------------------------------------- counts above 16 bits, the int32 refusal -----------
def test_large_count(ctx):
    """70 000 repeats of one A column x a 64-entry B row: every count is 70 000 (above 65535)"""
    b_rp, b_ci = _csr([list(range(0, 640, 10)), [5]])
    a_rp, a_ci = _csr([[0] * 70_000, [1, 0], [1]])
    A = ctx.upload(a_rp, a_ci, 2)
    B = ctx.upload(b_rp, b_ci, 1000)
    Fm = ctx.upload(*_csr([list(range(0, 1000, 5)), [5, 10, 20], [5, 6]]), 1000)
    try:
        (rp, ci, v), _ = _count(ctx, A, B, Fm)
        exp = count_ref(a_rp, a_ci, b_rp, b_ci, *_csr([list(range(0, 1000, 5)), [5, 10, 20], [5, 6]]), 1000)
        assert _diff((rp, ci, v), exp) is None, _diff((rp, ci, v), exp)
        assert np.all(v[:rp[1]] == 70_000) and rp[1] == 64
    finally:
        for h in (A, B, Fm):
            h.free()


def test_overflow_refused_and_context_usable(ctx):
    """65 536 repeats of one A column x a 32 768-entry B row: F_i = 2^31 > INT_MAX -> BSPGEMM_ERR_OVERFLOW, no result"""
    b_rp, b_ci = _csr([list(range(32768))])
    a_rp, a_ci = _csr([[0] * 65536, [0]])
    A = ctx.upload(a_rp, a_ci, 1)
    B = ctx.upload(b_rp, b_ci, 32768)
    Fm = ctx.upload(*_csr([[3], [4]]), 32768)
    L = bspgemm.lib()
    try:
        out = C.c_void_p(1)
        assert L.bspgemm_multiply_masked_count(ctx._h, A._h, B._h, Fm._h, 0, 2, C.byref(out)) == ERR_OVERFLOW
        assert not out.value
        # row 1 alone has one product: fine, and the context goes on working
        (rp, ci, v), _ = _count(ctx, A, B, Fm, 1, 2)
        assert rp.tolist() == [0, 1] and ci.tolist() == [4] and v.tolist() == [1]
    finally:
        for h in (A, B, Fm):
            h.free()


# ---------------------------------------------------------------- ranges and knobs -----------------------------------
@pytest.mark.parametrize("name", ["rmat14_skewed_wide", "tiny_b_wide_40M", "dense_window", "unaligned_300001"])
def test_count_knobs_and_ranges(ctx, name):
    """padded_rows x blocked_extents x check x class_streams, each over the whole A, an interior range, one row and none"""
    s = _shape(name)
    R, cols = s["a_rp"].size - 1, s["ncols"]
    f_rp, f_ci = random_mask(np.random.default_rng(31), R, cols, s["a_rp"], s["a_ci"])
    if "extra_mask" in s:                           # the row whose mask narrows the windows
        row, extra = s["extra_mask"]
        rows = np.repeat(np.arange(R), np.diff(f_rp)).astype(np.int64)
        f_rp, f_ci = gen._csr_from_pairs(np.concatenate([rows, np.full(extra.size, row)]),
                                         np.concatenate([f_ci.astype(np.int64), extra]), R, dedup=False, sort=False)
    ctx.set_flow("auto")
    ctx.set_option("small_path", -1)
    Fm = ctx.upload(f_rp, f_ci, cols + 1000)
    heavy = int(np.argmax(gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R)))
    failures, runs, exp = [], 0, {}
    try:
        for k, (pad, blk, chk, cs) in enumerate(np.ndindex(2, 2, 2, 2)):
            cs = 1 + 2 * cs
            for opt, v in (("padded_rows", pad), ("blocked_extents", blk), ("check", chk), ("class_streams", cs)):
                ctx.set_option(opt, v)
            A, B = _upload(ctx, s)
            try:
                inner = (min(R // 7 + k, R // 2), max(R - R // 5 - k, R // 2 + 1))
                for r0, r1 in ((0, R), inner, (heavy, heavy + 1), (R // 2, R // 2)):
                    if (r0, r1) not in exp:
                        exp[(r0, r1)] = count_ref(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], f_rp, f_ci, cols, r0, r1)
                    got, _ = _count(ctx, A, B, Fm, r0, r1)
                    runs += 1
                    bad = _diff(got, exp[(r0, r1)])
                    if bad:
                        failures.append("padded_rows=%d blocked_extents=%d check=%d class_streams=%d rows=[%d,%d): %s"
                                        % (pad, blk, chk, cs, r0, r1, bad))
            finally:
                A.free()
                B.free()
    finally:
        Fm.free()
        for opt, v in (("padded_rows", -1), ("blocked_extents", -1), ("check", 0), ("class_streams", 2)):
            ctx.set_option(opt, v)
    assert not failures, "%s: %d of %d runs wrong:\n  %s" % (name, len(failures), runs, "\n  ".join(failures))


# ---------------------------------------------------------------- graphs ----------------------------------------------
def _symmetrise(rp, ci, n):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    r, c = np.concatenate([rows, ci]), np.concatenate([ci, rows])
    off = r != c
    return gen._csr_from_pairs(r[off], c[off], n)


def _graph(kind):
    if kind == "rmat12":
        rp, ci, n = gen.rmat(12, 16, (0.57, 0.19, 0.19, 0.05), 2101)
    else:
        rp, ci, n = gen.powerlaw(6000, 6, 2102)
    s_rp, s_ci = _symmetrise(rp, ci, n)
    return s_rp, s_ci, n


@pytest.mark.parametrize("kind", ["rmat12", "powerlaw"])
def test_triangles_and_support(ctx, kind):
    import scipy.sparse as sp
    s_rp, s_ci, n = _graph(kind)
    S = sp.csr_matrix((np.ones(s_ci.size, np.int64), s_ci, s_rp), shape=(n, n))
    Ls = sp.tril(S, k=-1).tocsr()
    Ls.sort_indices()
    l_rp, l_ci = Ls.indptr.astype(np.int32), Ls.indices.astype(np.int32)
    A = ctx.upload(s_rp, s_ci, n)
    L = ctx.upload(l_rp, l_ci, n)
    try:
        Cr = ctx.multiply_masked_count(L, L, L)
        tri = int(Cr.download_values().astype(np.int64).sum())
        Cr.free()
        assert tri == int((S @ S @ S).diagonal().sum()) // 6 and tri > 0
        Cr = ctx.multiply_masked_count(A, A, A)
        rp, ci = Cr.download()
        v = Cr.download_values()
        Cr.free()
        sup = (S @ S).multiply(S).tocsr()
        sup.eliminate_zeros()
        sup.sort_indices()
        assert np.array_equal(rp, sup.indptr) and np.array_equal(ci, sup.indices) and np.array_equal(v, sup.data)
    finally:
        A.free()
        L.free()


def test_rmat18_pattern_identity(ctx):
    """R-MAT scale 18, F = pattern(A*A) through matrix_from_result: each row's counts sum to its product count, and the
    pattern is the product's"""
    rp, ci, n = bspgemm.gen_rmat(18, 16, (0.30, 0.25, 0.25), seed=18)
    A = ctx.upload(rp, ci, n)
    try:
        P = ctx.multiply(A, A)
        prp, pci = P.download()
        Fm = ctx.matrix_from_result(P, n)
        P.free()
        try:
            Cr = ctx.multiply_masked_count(A, A, Fm)
            crp, cci = Cr.download()
            v = Cr.download_values()
            Cr.free()
        finally:
            Fm.free()
        prefix = ctx.row_work_prefix(A, A)
        assert np.array_equal(crp, prp) and np.array_equal(cci, pci)
        assert v.min() >= 1
        sums = np.add.reduceat(v.astype(np.int64), crp[:-1][np.diff(crp) > 0]) if v.size else np.zeros(0, np.int64)
        assert np.array_equal(sums, np.diff(prefix)[np.diff(crp) > 0])
        assert np.all(np.diff(prefix)[np.diff(crp) == 0] == 0)
    finally:
        A.free()


# ---------------------------------------------------------------- errors and the result object -----------------------
def test_errors_and_result_object(ctx):
    rp, ci, n = gen.uniform(700, 6, 5301)
    A = ctx.upload(rp, ci, n)
    Fm = ctx.upload(rp, ci, n)
    short = ctx.upload(rp[:301], ci[:rp[300]], n)
    other = bspgemm.Context(0)
    Fo = other.upload(rp, ci, n)
    L = bspgemm.lib()
    try:
        for F, r0, r1 in ((short, 0, n), (short, 0, 301), (Fo, 0, n), (Fm, -1, n), (Fm, 5, 4), (Fm, 0, n + 1), (None, 0, n)):
            out = C.c_void_p(1)
            st = L.bspgemm_multiply_masked_count(ctx._h, A._h, A._h, F._h if F else None, r0, r1, C.byref(out))
            assert st == ERR_INVALID and not out.value, (r0, r1, st)
        # a mask of exactly row_end rows is enough
        got, _ = _count(ctx, A, A, short, 0, 300)
        assert _diff(got, count_ref(rp, ci, rp, ci, rp[:301], ci[:rp[300]], n, 0, 300)) is None
        # a pattern-only result never reports values, also when its buffers come from a freed counted result
        Cr = ctx.multiply_masked_count(A, A, Fm)
        assert Cr.values_device
        Cr.free()
        ctx.set_flow("upper-bound")
        ctx.set_option("small_path", 0)
        P = ctx.multiply(A, A)
        try:
            assert not P.values_device
            assert L.bspgemm_result_download_values(ctx._h, P._h, C.c_void_p(16)) == ERR_INVALID
            with pytest.raises(bspgemm.BspgemmError):
                P.download_values()
        finally:
            P.free()
            ctx.set_flow("auto")
            ctx.set_option("small_path", -1)
        M = ctx.multiply_masked(A, A, Fm)
        assert not M.values_device
        M.free()
    finally:
        for h in (A, Fm, short):
            h.free()
        Fo.free()
        other.close()
