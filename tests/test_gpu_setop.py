"""The on-device set operations (bspgemm_matrix_setop, bspgemm_matrix_equal, bspgemm_matrix_symmetrize), complete results
compared bit for bit with the numpy reference of setop_ref.py.

The kernels work in tiles of 4096 entries and flag words of 64, whatever rows the entries belong to: the shapes are chosen
around those two sizes -- rows that start and end on and off the boundaries, rows longer than two tiles against rows of
three entries or none, tiles that span more than 4096 (empty) rows, operands whose rows are unsorted and hold repeats (they
take the transposed-twice path) and col_idx arrays that are not 16-byte aligned.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import empty_ref
import gen
import ktruss_ref
from oracle import oracle as O
from setop_ref import canonical_ref, setop_ref, symmetrize_ref, transpose_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
OPS = ("or", "and", "andnot", "xor")
SKEW = (0.57, 0.19, 0.19, 0.05)


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[0].dtype == np.int32


def _check_handles(ctx, A, B, a, b, rows, cols, what, ops=OPS):
    """the set operations of operands A and B (host copies a, b = (row_ptr, col_idx)) against the reference"""
    bad = []
    for op in ops:
        S = ctx.setop(A, B, op)
        exp = setop_ref(a[0], a[1], b[0], b[1], rows, cols, op)
        if (S.rows, S.cols, S.nnz) != (rows, cols, exp[1].size) or not _same(S.download(), exp):
            bad.append("%s %s" % (what, op))
        S.free()
    return bad


def _check(ctx, a, b, rows, cols, what, ops=OPS):
    A, B = ctx.upload(a[0], a[1], cols), ctx.upload(b[0], b[1], cols)
    try:
        return _check_handles(ctx, A, B, a, b, rows, cols, what, ops)
    finally:
        A.free()
        B.free()


def _csr(rows_of, cols_of, n, dedup=True, sort=True):
    return gen._csr_from_pairs(np.asarray(rows_of), np.asarray(cols_of), n, dedup=dedup, sort=sort)


def _from_rows(lists, n):
    """CSR of a list of per-row column arrays, as given"""
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    ci = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    assert rp.size == n + 1
    return rp, ci


def _noisy(rp, ci, n, seed, repeats=0.3):
    """the same pattern with every row shuffled and some entries repeated"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), np.diff(rp))
    extra = rng.random(rows.size) < repeats
    r, c = np.concatenate([rows, rows[extra]]), np.concatenate([ci, ci[extra]])
    perm = rng.permutation(r.size)
    return _csr(r[perm], c[perm], n, dedup=False, sort=False)


# ---------------------------------------------------------------- 1. random ------------------------------------------
def test_random_pairs(ctx):
    rp, ci, n = gen.uniform(300, 6, 9101)
    rp2, ci2, _ = gen.uniform(300, 6, 9102)
    bad = _check(ctx, (rp, ci), (rp2, ci2), n, n, "uniform")
    rp, ci, n = gen.rmat(8, 12, SKEW, 9103)
    bad += _check(ctx, (rp, ci), transpose_ref(rp, ci, n, n), n, n, "rmat8 against its transpose")
    assert not bad, bad


# ---------------------------------------------------------------- 2. tile and word boundaries ------------------------
def _boundary_pair(lengths, last_common=True, cols=2048):
    """A: rows of the given lengths, columns ascending from a random set; B: every second column of A's row and columns
    that A lacks; the very last entry of A is common or not"""
    rng = np.random.default_rng(sum(lengths) + len(lengths))
    a_rows, b_rows = [], []
    for i, ln in enumerate(lengths):
        pick = np.sort(rng.choice(cols, size=min(cols, ln + 20), replace=False))
        a = pick[:ln] if i % 2 else pick[-ln:] if ln else pick[:0]
        others = np.setdiff1d(pick, a)
        b = np.union1d(a[::2], others[: 7 + i % 5])
        a_rows.append(a)
        b_rows.append(b)
    last = max(i for i, ln in enumerate(lengths) if ln)
    tail = a_rows[last][-1]
    b_rows[last] = np.union1d(b_rows[last], [tail]) if last_common else np.setdiff1d(b_rows[last], [tail])
    n = len(lengths)
    return _from_rows(a_rows, n), _from_rows(b_rows, n), n, cols


def _lengths_summing_to(total, seed):
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) + 310 < total:
        lens.append(int(rng.integers(300, 311)))
    lens.append(total - sum(lens))
    return lens


BOUNDARY = {
    "three_tiles_off_boundaries": lambda: _boundary_pair([300 + (7 * i) % 11 for i in range(40)]),
    "nnz_4096": lambda: _boundary_pair(_lengths_summing_to(4096, 1)),
    "nnz_4097": lambda: _boundary_pair(_lengths_summing_to(4097, 2)),
    "nnz_64": lambda: _boundary_pair([20, 0, 30, 14]),
    "row_ends_at_4096": lambda: _boundary_pair(_lengths_summing_to(4096, 3) + [0, 305, 64, 1]),
    "last_entry_common": lambda: _boundary_pair(_lengths_summing_to(5000, 4), last_common=True),
    "last_entry_not_common": lambda: _boundary_pair(_lengths_summing_to(5000, 4), last_common=False),
}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_tile_and_word_boundaries(ctx, name):
    a, b, n, cols = BOUNDARY[name]()
    if name == "nnz_4096":
        assert a[1].size == 4096
    if name == "row_ends_at_4096":
        assert 4096 in a[0].tolist() and a[1].size > 4096
    bad = _check(ctx, a, b, n, cols, name) + _check(ctx, b, a, n, cols, name + " mirrored")
    assert not bad, bad


# ---------------------------------------------------------------- 3. hub rows ----------------------------------------
def test_hub_rows(ctx):
    cols, n = 16384, 6
    rng = np.random.default_rng(9301)
    hub = np.sort(rng.choice(cols, size=10000, replace=False))
    other = np.union1d(hub[::2], np.setdiff1d(np.arange(cols), hub)[:5000])     # half of its columns shared
    three = np.array([hub[0], hub[5000] + 0, cols - 1])
    small = [np.array([1, 5]), np.array([], np.int64)]
    a = _from_rows([small[0], hub, small[1], hub, hub, np.array([7])], n)
    b = _from_rows([np.array([5, 9]), three, small[0], other, small[1], np.array([7])], n)
    bad = _check(ctx, a, b, n, cols, "hub") + _check(ctx, b, a, n, cols, "hub mirrored")
    assert not bad, bad


# ---------------------------------------------------------------- 4. long runs of empty rows -------------------------
def test_long_runs_of_empty_rows(ctx):
    n = 10000
    rng = np.random.default_rng(9401)
    a = _csr(np.concatenate([np.zeros(5000, int), np.full(300, n - 1)]),
             np.concatenate([rng.choice(n, 5000, replace=False), rng.choice(n, 300, replace=False)]), n)
    b = _csr(np.concatenate([np.full(4500, 5000), np.full(200, n - 1)]),
             np.concatenate([rng.choice(n, 4500, replace=False), rng.choice(n, 200, replace=False)]), n)
    bad = _check(ctx, a, b, n, n, "empty runs") + _check(ctx, b, a, n, n, "empty runs mirrored")
    assert not bad, bad


# ---------------------------------------------------------------- 5. degenerate shapes -------------------------------
def test_degenerate_shapes(ctx):
    rp, ci, n = gen.uniform(200, 5, 9501)
    empty = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32))
    bad = _check(ctx, empty, (rp, ci), n, n, "A empty") + _check(ctx, (rp, ci), empty, n, n, "B empty")
    bad += _check(ctx, empty, empty, n, n, "both empty")
    none = (np.zeros(1, np.int32), np.zeros(0, np.int32))
    bad += _check(ctx, none, none, 0, 5, "no rows") + _check(ctx, none, none, 0, 0, "no rows, no columns")
    bad += _check(ctx, (np.zeros(2, np.int32), np.zeros(0, np.int32)), (np.zeros(2, np.int32), np.zeros(0, np.int32)), 1, 0,
                  "no columns")
    one_a = _from_rows([[0], [], [0], [0], []], 5)
    one_b = _from_rows([[0], [0], [], [0], []], 5)
    bad += _check(ctx, one_a, one_b, 5, 1, "one column")
    full, hole = _from_rows([[0]], 1), _from_rows([[]], 1)
    for x, y, what in ((full, full, "1x1 both"), (full, hole, "1x1 A"), (hole, full, "1x1 B"), (hole, hole, "1x1 none")):
        bad += _check(ctx, x, y, 1, 1, what)
    assert not bad, bad


@pytest.mark.parametrize("rows,cols", empty_ref.SHAPES, ids=empty_ref.IDS)
def test_setop_of_nothing_is_an_operand(ctx, rows, cols):
    e = empty_ref.csr(rows)
    A, B = ctx.upload(e[0], e[1], cols), ctx.upload(e[0], e[1], cols)
    for op in OPS:
        S = ctx.setop(A, B, op)
        assert _same(S.download(), setop_ref(e[0], e[1], e[0], e[1], rows, cols, op))
        empty_ref.check(ctx, S, rows, cols)
        S.free()
    assert ctx.matrix_equal(A, B)
    if rows == cols:
        for drop in (False, True):
            S = ctx.symmetrize(A, drop_diagonal=drop)
            empty_ref.check(ctx, S, rows, cols)
            S.free()
    A.free()
    B.free()


def test_setop_that_leaves_nothing_is_an_operand(ctx):
    """4 x 4: A \\ A, A ^ A, and A & B of disjoint patterns"""
    n = 4
    a, b = empty_ref.diagonal(n), _from_rows([[1], [2], [3], [0]], n)
    A, B = ctx.upload(a[0], a[1], n), ctx.upload(b[0], b[1], n)
    for X, Y, x, y, op in ((A, A, a, a, "andnot"), (A, A, a, a, "xor"), (A, B, a, b, "and"), (B, A, b, a, "and")):
        S = ctx.setop(X, Y, op)
        assert _same(S.download(), setop_ref(x[0], x[1], y[0], y[1], n, n, op))
        empty_ref.check(ctx, S, n, n)
        S.free()
    S = ctx.symmetrize(A, drop_diagonal=True)
    empty_ref.check(ctx, S, n, n)
    for h in (S, A, B):
        h.free()


# ---------------------------------------------------------------- 6. algebra -----------------------------------------
def test_algebra(ctx):
    rp, ci, n = gen.dups_unsorted(700, 9, 9601)
    canon = canonical_ref(rp, ci, n, n)
    A = ctx.upload(rp, ci, n)
    for op in ("or", "and"):                                 # A op A, one handle
        S = ctx.setop(A, A, op)
        assert _same(S.download(), canon), op
        S.free()
    for op in ("andnot", "xor"):
        S = ctx.setop(A, A, op)
        assert S.nnz == 0 and not S.download()[0].any(), op
        S.free()
    A.free()
    # disjoint column ranges; B a subset of A
    rp2, ci2, _ = gen.uniform(700, 6, 9602)
    bad = _check(ctx, (rp, ci // 2), (rp2, n // 2 + ci2 // 2), n, n, "disjoint")
    sub = ktruss_ref._filter(canon[0], canon[1], np.arange(canon[1].size) % 3 == 0)
    bad += _check(ctx, canon, sub, n, n, "subset") + _check(ctx, sub, canon, n, n, "superset")
    assert not bad, bad
    for seed in (9603, 9604):
        a, b = gen.dups_unsorted(900, 8, seed)[:2], gen.uniform(900, 11, seed + 10)[:2]
        A, B = ctx.upload(a[0], a[1], 900), ctx.upload(b[0], b[1], 900)
        un, both, a_only, b_only, xor = (ctx.setop(A, B, "or"), ctx.setop(A, B, "and"), ctx.setop(A, B, "andnot"),
                                         ctx.setop(B, A, "andnot"), ctx.setop(A, B, "xor"))
        assert un.nnz + both.nnz == canonical_ref(a[0], a[1], 900, 900)[1].size + canonical_ref(b[0], b[1], 900, 900)[1].size
        back = ctx.setop(a_only, both, "or")
        assert _same(back.download(), canonical_ref(a[0], a[1], 900, 900))
        sym = ctx.setop(a_only, b_only, "or")
        assert _same(sym.download(), xor.download()) and xor.nnz > 0 and ctx.matrix_equal(sym, xor)
        for h in (A, B, un, both, a_only, b_only, xor, back, sym):
            h.free()


# ---------------------------------------------------------------- 7. non-canonical inputs ----------------------------
def test_non_canonical_inputs(ctx):
    import torch
    rp, ci, n = gen.rmat(9, 10, SKEW, 9701)
    rp2, ci2, _ = gen.uniform(n, 7, 9702)
    na, nb = _noisy(rp, ci, n, 1), _noisy(rp2, ci2, n, 2)
    assert na[1].size > ci.size
    bad = _check(ctx, na, (rp2, ci2), n, n, "A noisy") + _check(ctx, (rp, ci), nb, n, n, "B noisy")
    bad += _check(ctx, na, nb, n, n, "both noisy")
    # interior-row_ptr uploads
    r0, rows = 100, 300
    A = ctx.upload(na[0], na[1], n, row0=r0, rows=rows)
    B = ctx.upload(rp2, ci2, n, row0=r0, rows=rows)
    sub = lambda p, c: ((p[r0:r0 + rows + 1] - p[r0]).astype(np.int32), c[p[r0]:p[r0 + rows]])
    bad += _check_handles(ctx, A, B, sub(*na), sub(rp2, ci2), rows, n, "interior upload")
    A.free()
    B.free()
    # wrapped device arrays whose col_idx is one int off 16-byte alignment
    keep, wrapped = [], []
    for p, c in ((rp, ci), nb):
        trp = torch.from_numpy(p).cuda()
        buf = torch.zeros(c.size + 4, dtype=torch.int32, device="cuda")
        buf[1:1 + c.size] = torch.from_numpy(c).cuda()
        torch.cuda.synchronize()
        tci = buf[1:]
        assert tci.data_ptr() % 16 == 4
        keep.append((trp, buf))
        wrapped.append(ctx.wrap_device(n, n, c.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf)))
    bad += _check_handles(ctx, wrapped[0], wrapped[1], (rp, ci), nb, n, n, "wrapped, off alignment")
    for h in wrapped:
        h.free()
    assert not bad, bad


# ---------------------------------------------------------------- 8. against the products ----------------------------
def test_cross_check_against_the_products(ctx):
    """OR, AND and ANDNOT the way they could be had before: products through an identity operand"""
    rp, ci, n = gen.rmat(8, 12, SKEW, 9801)
    b = transpose_ref(rp, ci, n, n)
    A, B = ctx.upload(rp, ci, n), ctx.upload(b[0], b[1], n)
    eye = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    cases = (("or", A, B, ctx.multiply_accumulate(eye, B, A)), ("and", A, B, ctx.multiply_masked(eye, B, A)),
             ("andnot", B, A, ctx.multiply_masked(eye, B, A, complement=True)))
    for op, x, y, P in cases:
        M = ctx.matrix_from_result(P, n)
        S = ctx.setop(x, y, op)
        assert S.nnz == M.nnz > 0 and _same(S.download(), M.download()), op
        for h in (P, M, S):
            h.free()
    for h in (A, B, eye):
        h.free()


# ---------------------------------------------------------------- 9. the output is an operand ------------------------
def test_the_output_is_a_real_operand(ctx):
    rp, ci, n = gen.rmat(9, 8, SKEW, 9901)
    rp2, ci2, _ = gen.uniform(n, 5, 9902)
    A, B = ctx.upload(rp, ci, n), ctx.upload(rp2, ci2, n)
    U = ctx.setop(A, B, "or")
    u = setop_ref(rp, ci, rp2, ci2, n, n, "or")
    assert U.uses_blocked_table == -1 and U.uses_padded_rows == -1
    P = ctx.multiply(U, U)
    erp, eci = O.spgemm(u[0], u[1], u[0], u[1], n)
    prp, pci = P.download()
    assert np.array_equal(prp, erp) and np.array_equal(pci, eci)
    T = ctx.transpose(U)
    assert _same(T.download(), transpose_ref(u[0], u[1], n, n))
    L = ctx.select(U, "tril")
    assert _same(L.download(), ktruss_ref.select_ref(u[0], u[1], "tril"))
    X = ctx.setop(U, T, "xor")                                # an earlier setop and a transpose as inputs
    assert _same(X.download(), setop_ref(u[0], u[1], *transpose_ref(u[0], u[1], n, n), n, n, "xor"))
    for h in (A, B, U, P, T, L, X):
        h.free()


# ---------------------------------------------------------------- 10. matrix_equal -----------------------------------
def test_matrix_equal(ctx):
    a, b, n, cols = _boundary_pair(_lengths_summing_to(9000, 5))
    A = ctx.upload(a[0], a[1], cols)
    noisy = _noisy(a[0], a[1], n, 3)
    N = ctx.upload(noisy[0], noisy[1], cols)
    assert ctx.matrix_equal(A, A) and ctx.matrix_equal(A, N) and ctx.matrix_equal(N, A)
    N.free()
    free_col = lambda r: int(np.setdiff1d(np.arange(cols), a[1][a[0][r]:a[0][r + 1]])[0])
    for p in (0, a[1].size - 1, 4095, 4096):                  # one entry differs: first, last, on a tile boundary
        c = a[1].copy()
        c[p] = free_col(int(np.searchsorted(a[0], p, side="right")) - 1)
        D = ctx.upload(a[0], c, cols)                         # equal nnz, different sets (row p no longer ascending)
        assert not ctx.matrix_equal(A, D) and not ctx.matrix_equal(D, A), p
        D.free()
        keep = np.ones(a[1].size, bool)
        keep[p] = False
        M = ctx.upload(*ktruss_ref._filter(a[0], a[1], keep), cols)
        assert not ctx.matrix_equal(A, M) and not ctx.matrix_equal(M, A), p
        M.free()
    W = ctx.upload(a[0], a[1], cols + 1)
    eq = C.c_int(-7)
    L = bspgemm.lib()
    assert L.bspgemm_matrix_equal(ctx._h, A._h, W._h, C.byref(eq)) == ERR_INVALID and eq.value == -7
    assert "bspgemm_matrix_equal" in L.bspgemm_last_error().decode()
    e1, e2 = ctx.upload(np.zeros(4, np.int32), [], 9), ctx.upload(np.zeros(4, np.int32), [], 9)
    assert ctx.matrix_equal(e1, e2)
    for h in (A, W, e1, e2):
        h.free()


# ---------------------------------------------------------------- 11. errors -----------------------------------------
def test_errors(ctx):
    rp, ci, n = gen.uniform(500, 6, 10001)
    A = ctx.upload(rp, ci, n)
    L = bspgemm.lib()
    other = bspgemm.Context(0)
    Ao = other.upload(rp, ci, n)
    fewer_rows = ctx.upload(rp[:-1], ci[:rp[-2]], n)
    more_cols = ctx.upload(rp, ci, n + 1)
    high, low = ci.copy(), ci.copy()
    high[4200 % ci.size] = n
    low[-1] = -1
    Hi, Lo = ctx.upload(rp, high, n), ctx.upload(rp, low, n)

    def refused(x, y, op=1):
        out = C.c_void_p(1)
        ok = L.bspgemm_matrix_setop(ctx._h, x._h, y._h, op, C.byref(out)) == ERR_INVALID and not out.value
        return ok and "bspgemm_matrix_setop" in L.bspgemm_last_error().decode()

    try:
        assert refused(A, fewer_rows) and refused(fewer_rows, A) and refused(A, more_cols)
        assert refused(A, Ao) and refused(Ao, A)
        for op in (0, 5, -1):
            assert refused(A, A, op)
        for op in (1, 2, 3, 4):
            for bad in (Hi, Lo):
                assert refused(A, bad, op) and refused(bad, A, op), op
        assert "column" in L.bspgemm_last_error().decode()
        eq = C.c_int(-7)
        assert L.bspgemm_matrix_equal(ctx._h, A._h, Hi._h, C.byref(eq)) == ERR_INVALID and eq.value == -7
        # the context goes on working
        S = ctx.setop(A, A, "or")
        assert _same(S.download(), canonical_ref(rp, ci, n, n))
        S.free()
    finally:
        for h in (A, fewer_rows, more_cols, Hi, Lo):
            h.free()
        Ao.free()
        other.close()


# ---------------------------------------------------------------- 12. symmetrize -------------------------------------
def test_symmetrize(ctx):
    rp, ci, n = gen.rmat(8, 12, SKEW, 10101)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.any(rows == ci) and not _same(transpose_ref(rp, ci, n, n), (rp, ci))        # directed, with loops
    A = ctx.upload(rp, ci, n)
    L = bspgemm.lib()
    for drop in (False, True):
        S = ctx.symmetrize(A, drop_diagonal=drop)
        assert _same(S.download(), symmetrize_ref(rp, ci, n, drop)), drop
        T = ctx.transpose(S)
        assert ctx.matrix_equal(S, T) and not ctx.matrix_equal(S, A)
        T.free()
        if drop:
            s_rp, s_ci = ktruss_ref.symmetrise(rp, ci, n)
            assert ctx.triangle_count(S) == ktruss_ref.triangles_ref(s_rp, s_ci, n) > 0
            K, it, conv = ctx.ktruss(S, 4)
            (k_rp, k_ci), e_it, e_conv = ktruss_ref.ktruss_ref(s_rp, s_ci, n, 4)
            assert _same(K.download(), (k_rp, k_ci)) and (it, conv) == (e_it, e_conv) and K.nnz > 0
            K.free()
        S.free()
    R = ctx.upload(np.zeros(4, np.int32), [], 5)
    out = C.c_void_p(1)
    assert L.bspgemm_matrix_symmetrize(ctx._h, R._h, 0, C.byref(out)) == ERR_INVALID and not out.value
    assert "bspgemm_matrix_symmetrize" in L.bspgemm_last_error().decode()
    for flags in (2, 3, 0x80000000):
        out = C.c_void_p(1)
        assert L.bspgemm_matrix_symmetrize(ctx._h, A._h, flags, C.byref(out)) == ERR_INVALID and not out.value
    A.free()
    R.free()


# ---------------------------------------------------------------- 13. a random campaign ------------------------------
def test_random_campaign(ctx):
    rng = np.random.default_rng(10201)
    bad = []
    for case in range(20):
        n = int(rng.integers(1, 3001))
        cols = int(rng.integers(1, 4001))
        sides = []
        for _ in range(2):
            deg = rng.integers(0, 41) * rng.random()
            lens = rng.poisson(deg, size=n)
            if rng.random() < 0.3:
                lens[rng.integers(0, n)] = min(cols, int(rng.integers(1000, 6000)))      # a hub row
            lens = np.minimum(lens, cols)
            r = np.repeat(np.arange(n), lens)
            c = rng.integers(0, cols, size=r.size)
            noise = rng.random() < 0.4
            sides.append(_csr(r, c, n, dedup=not noise, sort=not noise))
        op = OPS[int(rng.integers(0, 4))]
        bad += _check(ctx, sides[0], sides[1], n, cols, "case %d (%d x %d)" % (case, n, cols), ops=(op,))
    assert not bad, bad
