"""The on-device stable filters and the value sum (bspgemm_matrix_select, bspgemm_matrix_from_result_where,
bspgemm_result_values_sum), complete results compared bit for bit with the numpy references of ktruss_ref.py.

The kernels work in tiles of 4096 entries and flag words of 64, whatever rows the entries belong to: the shapes hold
sizes that are no multiple of either, rows longer than three tiles, tiles that span more than 4096 (empty) rows -- the
row_ptr window is then searched in global memory instead of LDS -- and col_idx arrays that are not 16-byte aligned.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import empty_ref
import gen
from ktruss_ref import dedup_ref, select_ref, symmetrise, where_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
OPS = ("tril", "triu", "offdiag")
CMPS = (">=", ">", "<=", "<", "==", "!=")
INT32_MAX = 0x7fffffff


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[0].dtype == np.int32


def _check_select(ctx, A, rp, ci, what):
    """the three selects of operand A (host copy rp, ci) against the reference"""
    bad = []
    for op in OPS:
        S = ctx.select(A, op)
        exp = select_ref(rp, ci, op)
        if (S.rows, S.cols, S.nnz) != (A.rows, A.cols, exp[1].size) or not _same(S.download(), exp):
            bad.append("%s %s" % (what, op))
        S.free()
    return bad


# ---------------------------------------------------------------- structural select: shapes --------------------------
def _hub_and_empty():
    """20000 rows, all empty but row 5 (13001 entries: more than three tiles, unsorted, repeats), row 6 (one entry) and the
    last row: the tiles after the hub span thousands of empty rows"""
    n = 20000
    rng = np.random.default_rng(77)
    rows = np.concatenate([np.full(13001, 5), [6], np.full(70, n - 1)])
    cols = np.concatenate([rng.integers(0, 40, size=13001), [6], rng.integers(0, n, size=70)])
    rp, ci = gen._csr_from_pairs(rows, cols, n, dedup=False, sort=False)
    return rp, ci, n


def _rect(nr, nc, d, seed):
    rp, ci = gen.uniform_rect(nr, nc, d, seed)
    return rp, ci, nc


SELECT_SHAPES = {
    "uniform": lambda: gen.uniform(3000, 8, 6101),
    "rmat13_skewed": lambda: gen.rmat(13, 16, (0.57, 0.19, 0.19, 0.05), 6102),
    "powerlaw": lambda: gen.powerlaw(20000, 8, 6103),
    "dups_unsorted": lambda: gen.dups_unsorted(4000, 12, 6104),
    "rect_tall": lambda: _rect(2500, 700, 9, 6105),
    "rect_wide": lambda: _rect(700, 2500, 9, 6106),
    "hub_and_empty": _hub_and_empty,
    "one_tile_exactly": lambda: gen.uniform_rect(4096, 100000, 1, 6107) + (100000,),
    "sixty_three": lambda: gen.uniform_rect(63, 63, 1, 6108) + (63,),
}


@pytest.mark.parametrize("name", list(SELECT_SHAPES))
def test_select_shape(ctx, name):
    rp, ci, cols = SELECT_SHAPES[name]()
    A = ctx.upload(rp, ci, cols)
    try:
        bad = _check_select(ctx, A, rp, ci, name)
    finally:
        A.free()
    assert not bad, bad


def test_select_empty_shapes(ctx):
    for rows, cols in ((0, 5), (0, 0), (100, 100), (1, 0)):
        rp = np.zeros(rows + 1, np.int32)
        A = ctx.upload(rp, np.zeros(0, np.int32), cols)
        for op in OPS:
            S = ctx.select(A, op)
            grp, gci = S.download()
            assert (S.rows, S.cols, S.nnz) == (rows, cols, 0) and not grp.any() and gci.size == 0
            S.free()
        A.free()
    # entries, but none is kept / every one is kept
    n = 5000
    diag = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    assert ctx.select(diag, "offdiag").nnz == 0 and ctx.select(diag, "tril").nnz == 0
    rp, ci = np.arange(n + 1, dtype=np.int32), np.full(n, n, np.int32)        # column n: above every row
    up = ctx.upload(rp, ci, n + 1)
    assert _same(ctx.select(up, "triu").download(), (rp, ci)) and ctx.select(up, "tril").nnz == 0
    diag.free()
    up.free()


@pytest.mark.parametrize("rows,cols", empty_ref.SHAPES, ids=empty_ref.IDS)
def test_select_of_nothing_is_an_operand(ctx, rows, cols):
    rp, ci = empty_ref.csr(rows)
    A = ctx.upload(rp, ci, cols)
    for op in OPS:
        S = ctx.select(A, op)
        assert _same(S.download(), select_ref(rp, ci, op))
        empty_ref.check(ctx, S, rows, cols)
        S.free()
    # by value: the counted product of operands without entries
    Y = ctx.upload(*empty_ref.csr(cols), cols)
    Cc = ctx.multiply_masked_count(A, Y, A)
    assert (Cc.rows, Cc.nnz, Cc.values_sum()) == (rows, 0, 0)
    for cmp in CMPS:
        M = ctx.matrix_from_result_where(Cc, cols, cmp, 1)
        empty_ref.check(ctx, M, rows, cols)
        M.free()
    for h in (Cc, Y, A):
        h.free()


def test_select_that_keeps_nothing_is_an_operand(ctx):
    """a 4 x 4 diagonal: no entry is off it, and no count of D .* (D * D) is above 1"""
    n = 4
    rp, ci = empty_ref.diagonal(n)
    D = ctx.upload(rp, ci, n)
    for op in OPS:
        S = ctx.select(D, op)
        assert _same(S.download(), select_ref(rp, ci, op))
        empty_ref.check(ctx, S, n, n)
        S.free()
    Cc = ctx.multiply_masked_count(D, D, D)
    assert np.array_equal(Cc.download_values(), np.ones(n, np.int32))
    M = ctx.matrix_from_result_where(Cc, n, ">", 1)
    assert _same(M.download(), where_ref(*Cc.download(), Cc.download_values(), ">", 1))
    empty_ref.check(ctx, M, n, n)
    for h in (M, Cc, D):
        h.free()


def test_select_operand_sources(ctx):
    """interior-row_ptr upload, wrapped device arrays (col_idx 16-byte aligned and not), a transpose's output, a product
    turned operand, an earlier select"""
    import torch
    rp, ci, n = gen.rmat(12, 8, (0.57, 0.19, 0.19, 0.05), seed=6201)
    bad = []
    r0, rows = 1000, 2000
    A = ctx.upload(rp, ci, n, row0=r0, rows=rows)
    sub_rp = (rp[r0:r0 + rows + 1] - rp[r0]).astype(np.int32)
    bad += _check_select(ctx, A, sub_rp, ci[rp[r0]:rp[r0 + rows]], "interior upload")
    trp = torch.from_numpy(rp).cuda()
    for shift in (0, 1, 3):
        buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
        buf[shift:shift + ci.size] = torch.from_numpy(ci).cuda()
        torch.cuda.synchronize()
        tci = buf[shift:]
        assert tci.data_ptr() % 16 == 4 * shift
        W = ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf))
        bad += _check_select(ctx, W, rp, ci, "wrapped, col_idx %d bytes off alignment" % (4 * shift))
        W.free()
    B = ctx.upload(rp, ci, n)
    T = ctx.transpose(B)
    bad += _check_select(ctx, T, *T.download(), "transpose")
    P = ctx.multiply(B, B)
    M = ctx.matrix_from_result(P, n)
    P.free()
    bad += _check_select(ctx, M, *M.download(), "matrix_from_result")
    S = ctx.select(M, "offdiag")
    bad += _check_select(ctx, S, *S.download(), "earlier select")
    for h in (A, B, T, M, S):
        h.free()
    assert not bad, bad


def _keys(rp, ci):
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    return (rows << 32) | np.asarray(ci, np.int64)


def test_select_identities(ctx):
    rp, ci, n = gen.dups_unsorted(3000, 20, 6301)
    A = ctx.upload(rp, ci, n)
    lo, up, off = (ctx.select(A, op) for op in OPS)
    kl, ku, ko = (_keys(*m.download()) for m in (lo, up, off))
    assert np.array_equal(np.union1d(kl, ku), np.unique(ko)) and np.intersect1d(kl, ku).size == 0
    assert lo.nnz + up.nnz == off.nnz
    # select(transpose(A), TRIU) == transpose(select(A, TRIL)): both sorted and duplicate-free
    AT = ctx.transpose(A)
    left = ctx.select(AT, "triu")
    right = ctx.transpose(lo)
    assert _same(left.download(), right.download()) and left.nnz > 0
    # ... and transposing back gives the deduplicated lower triangle
    back = ctx.transpose(right)
    assert _same(back.download(), dedup_ref(*select_ref(rp, ci, "tril"), n))
    for h in (A, lo, up, off, AT, left, right, back):
        h.free()


def test_select_leaves_the_statistics_alone(ctx):
    rp, ci, n = gen.uniform(2000, 6, 6401)
    A = ctx.upload(rp, ci, n)
    P = ctx.multiply(A, A, 0, n // 2)
    Q = ctx.multiply(A, A)
    before = [ctx.stats(age) for age in range(2)]
    assert before[0]["rows"] == n and before[1]["rows"] == n // 2
    S = ctx.select(A, "tril")
    assert [ctx.stats(age) for age in range(2)] == before
    Cc = ctx.multiply_masked_count(A, A, A)
    after_count = [ctx.stats(age) for age in range(3)]
    assert after_count[1:] == before
    W = ctx.matrix_from_result_where(Cc, n, ">=", 1)
    total = Cc.values_sum()
    ctx.select(S, "triu").free()
    assert [ctx.stats(age) for age in range(3)] == after_count
    assert total == int(Cc.download_values().astype(np.int64).sum())
    for h in (A, P, Q, S, Cc, W):
        h.free()


# ---------------------------------------------------------------- the product of a selected operand ------------------
@pytest.mark.parametrize("tables", [(-1, -1), (1, 1)])
def test_product_of_selected_operand(ctx, tables):
    """a selected operand multiplies like the same selection uploaded from the host, also when the derived tables (blocked
    extents, padded rows) are forced into use"""
    rp, ci, n = gen.rmat(12, 16, (0.57, 0.19, 0.19, 0.05), seed=6501)
    ctx.set_option("blocked_extents", tables[0])
    ctx.set_option("padded_rows", tables[1])
    try:
        A = ctx.upload(rp, ci, n)
        Cc = ctx.multiply_masked_count(A, A, A)
        crp, cci = Cc.download()
        v = Cc.download_values()
        pairs = [(ctx.select(A, op), ctx.upload(*select_ref(rp, ci, op), n)) for op in OPS]
        pairs.append((ctx.matrix_from_result_where(Cc, n, ">=", 2), ctx.upload(*where_ref(crp, cci, v, ">=", 2), n)))
        Cc.free()
        for dev, host in pairs:
            assert dev.nnz == host.nnz > 0
            got, exp = ctx.multiply(dev, dev), ctx.multiply(host, host)
            assert got.nnz == exp.nnz and all(np.array_equal(g, e) for g, e in zip(got.download(), exp.download()))
            got.free()
            exp.free()
            got, exp = ctx.multiply_masked_count(A, dev, dev), ctx.multiply_masked_count(A, host, host)
            assert all(np.array_equal(g, e) for g, e in zip(got.download(), exp.download()))
            assert np.array_equal(got.download_values(), exp.download_values())
            for h in (got, exp, dev, host):
                h.free()
        A.free()
    finally:
        ctx.set_option("blocked_extents", -1)
        ctx.set_option("padded_rows", -1)


# ---------------------------------------------------------------- select by value ------------------------------------
def _counted_uniform(ctx):
    """one-wave rows: A .* (A*A) of a uniform matrix with repeated entries (counts above 1)"""
    rp, ci, n = gen.dups_unsorted(3000, 10, 6601)
    A = ctx.upload(rp, ci, n)
    return ctx.multiply_masked_count(A, A, A), n, [A]


def _counted_pattern(ctx, a_rp, a_ci, b_rp, b_ci, cols):
    """F = pattern(A*B): every product is kept, rows of every class"""
    A = ctx.upload(a_rp, a_ci, b_rp.size - 1)
    B = ctx.upload(b_rp, b_ci, cols)
    P = ctx.multiply(A, B)
    Fm = ctx.matrix_from_result(P, cols)
    P.free()
    return ctx.multiply_masked_count(A, B, Fm), cols, [A, B, Fm]


def _counted_class_boundaries(ctx):
    """one-wave rows at every class boundary and dense-window rows of up to 600000 products"""
    return _counted_pattern(ctx, *gen.class_boundary_rows(repeat=1, seed=6602), 6000)


def _counted_rank(ctx):
    """rank-class rows (2048 < products <= 6144 over 700001 columns)"""
    return _counted_pattern(ctx, *gen.rank_rows(700_001, [2049, 4097, 6144, 6145, 3000, 5000] * 2, short_rows=(4, 10),
                                                ones_rows=(5,), seed=6603, counts=(6000, 1000, 100)), 700_001)


def _counted_support(ctx):
    """edge supports of a skewed graph"""
    rp, ci, n = gen.rmat(12, 16, (0.57, 0.19, 0.19, 0.05), 6604)
    s_rp, s_ci = symmetrise(rp, ci, n)
    A = ctx.upload(s_rp, s_ci, n)
    return ctx.multiply_masked_count(A, A, A), n, [A]


COUNTED = {"uniform_one_wave": _counted_uniform, "class_boundaries_dense": _counted_class_boundaries, "rank_rows": _counted_rank,
           "graph_support": _counted_support}


@pytest.mark.parametrize("name", list(COUNTED))
def test_from_result_where(ctx, name):
    Cc, cols, operands = COUNTED[name](ctx)
    try:
        rp, ci = Cc.download()
        v = Cc.download_values()
        assert v.size > 4096 and v.min() >= 1
        assert Cc.values_sum() == int(v.astype(np.int64).sum())
        vmax = int(v.max())
        thresholds = sorted({-1, 0, 1, 2, int(np.median(v)), vmax, vmax + 1, INT32_MAX})
        bad, kept = [], set()
        for cmp in CMPS:
            for t in thresholds:
                M = ctx.matrix_from_result_where(Cc, cols, cmp, t)
                exp = where_ref(rp, ci, v, cmp, t)
                kept.add("none" if exp[1].size == 0 else "all" if exp[1].size == v.size else "some")
                if (M.rows, M.cols, M.nnz) != (Cc.rows, cols, exp[1].size) or not _same(M.download(), exp):
                    bad.append("%s %d" % (cmp, t))
                M.free()
        assert not bad, "%s: wrong for %s" % (name, bad)
        assert kept == {"none", "all", "some"}
        # GE 1 (and below) is matrix_from_result itself
        plain = ctx.matrix_from_result(Cc, cols)
        for t in (1, 0, -5):
            M = ctx.matrix_from_result_where(Cc, cols, ">=", t)
            assert _same(M.download(), plain.download())
            M.free()
        plain.free()
    finally:
        Cc.free()
        for h in operands:
            h.free()


def test_from_result_where_errors(ctx):
    rp, ci, n = gen.uniform(700, 6, 6701)
    A = ctx.upload(rp, ci, n)
    L = bspgemm.lib()
    P = ctx.multiply(A, A)
    Cc = ctx.multiply_masked_count(A, A, A)
    other = bspgemm.Context(0)
    Ao = other.upload(rp, ci, n)
    try:
        assert not P.values_device
        out = C.c_void_p(1)
        assert L.bspgemm_matrix_from_result_where(ctx._h, P._h, n, 1, 1, C.byref(out)) == ERR_INVALID and not out.value
        assert "pattern-only" in L.bspgemm_last_error().decode()
        s = C.c_int64(-7)
        assert L.bspgemm_result_values_sum(ctx._h, P._h, C.byref(s)) == ERR_INVALID and s.value == -7
        with pytest.raises(bspgemm.BspgemmError):
            P.values_sum()
        for cmp in (0, 7, -1):
            out = C.c_void_p(1)
            assert L.bspgemm_matrix_from_result_where(ctx._h, Cc._h, n, cmp, 1, C.byref(out)) == ERR_INVALID and not out.value
        for op in (0, 4, -1):
            out = C.c_void_p(1)
            assert L.bspgemm_matrix_select(ctx._h, A._h, op, C.byref(out)) == ERR_INVALID and not out.value
        # handles of another context
        out = C.c_void_p(1)
        assert L.bspgemm_matrix_select(ctx._h, Ao._h, 1, C.byref(out)) == ERR_INVALID and not out.value
        out = C.c_void_p(1)
        assert L.bspgemm_matrix_from_result_where(other._h, Cc._h, n, 1, 1, C.byref(out)) == ERR_INVALID and not out.value
        assert L.bspgemm_result_values_sum(other._h, Cc._h, C.byref(s)) == ERR_INVALID and s.value == -7
        # the context goes on working
        assert _same(ctx.select(A, "tril").download(), select_ref(rp, ci, "tril"))
    finally:
        for h in (A, P, Cc):
            h.free()
        Ao.free()
        other.close()


def test_values_sum_above_int32(ctx):
    """64 hub rows of 1250 repeated entries each on a 40000-entry B row: every count is 1250 per column and row, 3.2e9 in all"""
    width, reps, hubs = 40_000, 1250, 64
    b_rp = np.array([0, width], np.int32)
    b_ci = np.arange(width, dtype=np.int32)
    a_rp = (np.arange(hubs + 1) * reps).astype(np.int32)
    a_ci = np.zeros(hubs * reps, np.int32)
    f_rp = (np.arange(hubs + 1) * width).astype(np.int32)
    f_ci = np.tile(b_ci, hubs)
    A, B, Fm = ctx.upload(a_rp, a_ci, 1), ctx.upload(b_rp, b_ci, width), ctx.upload(f_rp, f_ci, width)
    try:
        Cc = ctx.multiply_masked_count(A, B, Fm)
        v = Cc.download_values()
        assert v.size == hubs * width and np.all(v == reps)
        total = Cc.values_sum()
        assert total == hubs * width * reps == int(v.astype(np.int64).sum()) and total > 2 ** 31
        Cc.free()
    finally:
        for h in (A, B, Fm):
            h.free()


# ---------------------------------------------------------------- one size case --------------------------------------
def test_rmat16_counted_result_thousands_of_tiles(ctx):
    """symmetrised R-MAT scale 16, edge factor 6, F = pattern(A*A): a counted result of 11 M entries, 2700 tiles of 4096,
    filtered three ways and compared completely; the structural selects of the same pattern as an operand as well.
    (0.5 s on an MI355X, what test_from_result_where's four cases take together; nearly all of it is the generator, the
    downloads and the numpy references.)"""
    rp, ci, n = bspgemm.gen_rmat(16, 6, (0.30, 0.25, 0.25), seed=16)
    s_rp, s_ci = symmetrise(rp, ci, n)
    A = ctx.upload(s_rp, s_ci, n)
    P = ctx.multiply(A, A)
    Fm = ctx.matrix_from_result(P, n)
    P.free()
    Cc = ctx.multiply_masked_count(A, A, Fm)
    try:
        crp, cci = Cc.download()
        v = Cc.download_values()
        assert v.size >= 2000 * 4096 and v.size % 4096 != 0
        assert Cc.values_sum() == int(v.astype(np.int64).sum())
        for cmp, t in ((">=", 2), ("<=", 1), ("!=", 3)):
            M = ctx.matrix_from_result_where(Cc, n, cmp, t)
            exp = where_ref(crp, cci, v, cmp, t)
            assert 0 < exp[1].size < v.size and M.nnz == exp[1].size and _same(M.download(), exp), (cmp, t)
            M.free()
        frp = crp.astype(np.int32)
        for op in OPS:
            S = ctx.select(Fm, op)
            assert _same(S.download(), select_ref(frp, cci, op)), op
            S.free()
    finally:
        for h in (A, Fm, Cc):
            h.free()
