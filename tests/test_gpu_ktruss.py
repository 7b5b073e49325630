"""Device-resident triangle count and k-truss (bspgemm_triangle_count, bspgemm_ktruss) against the scipy restatement of
their definitions in ktruss_ref.py (which test_select_abi.py checks against networkx): the truss compared entry for
entry, the number of counted products and the converged flag as well.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
from ktruss_ref import ktruss_ref, symmetrise, triangles_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _graph(kind):
    if kind == "rmat12":
        rp, ci, n = gen.rmat(12, 16, (0.57, 0.19, 0.19, 0.05), 7101)
    elif kind == "powerlaw":
        rp, ci, n = gen.powerlaw(6000, 6, 7102)
    else:
        rp, ci, n = gen.uniform(2500, 12, 7103)
    return symmetrise(rp, ci, n) + (n,)


def _complete(n):
    rows = np.repeat(np.arange(n), n - 1)
    cols = np.concatenate([np.delete(np.arange(n), i) for i in range(n)])
    return gen._csr_from_pairs(rows, cols, n) + (n,)


def _noisy(rp, ci, n, seed):
    """the same graph with self-loops, repeated entries and extra entries above the diagonal, rows unsorted"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), np.diff(rp))
    extra_r = rng.integers(0, n, size=3 * n)
    extra_c = rng.integers(0, n, size=3 * n)
    upper = extra_c > extra_r
    r = np.concatenate([rows, np.arange(n), rows[::3], extra_r[upper]])
    c = np.concatenate([ci, np.arange(n), ci[::3], extra_c[upper]])
    perm = rng.permutation(r.size)
    return gen._csr_from_pairs(r[perm], c[perm], n, dedup=False, sort=False)


def _still_usable(ctx, rp, ci, n):
    """a plain multiply after the loops: its result survives the round trip through an operand"""
    A = ctx.upload(rp, ci, n)
    P = ctx.multiply(A, A)
    M = ctx.matrix_from_result(P, n)
    prp, pci = P.download()
    mrp, mci = M.download()
    assert np.array_equal(prp, mrp) and np.array_equal(pci, mci) and P.nnz > 0
    I = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    Q = ctx.multiply(M, I)
    assert bspgemm.csr_equal(*Q.download(), prp, pci)
    for h in (A, P, M, I, Q):
        h.free()


# ---------------------------------------------------------------- triangles ------------------------------------------
@pytest.mark.parametrize("kind", ["rmat12", "powerlaw"])
def test_triangle_count(ctx, kind):
    rp, ci, n = _graph(kind)
    exp = triangles_ref(rp, ci, n)
    A = ctx.upload(rp, ci, n)
    assert ctx.triangle_count(A) == exp and exp > 0
    st = ctx.stats()                                  # the statistics describe the counted product L .* (L*L)
    assert st["rows"] == n and st["flow"] == 1 and st["nnz_a"] == ci.size // 2
    # self-loops, repeated entries and entries above the diagonal change nothing
    n_rp, n_ci = _noisy(rp, ci, n, 5)
    assert triangles_ref(n_rp, n_ci, n) == exp
    N = ctx.upload(n_rp, n_ci, n)
    assert ctx.triangle_count(N) == exp
    A.free()
    N.free()
    _still_usable(ctx, rp, ci, n)


def test_triangle_count_closed_forms(ctx):
    for n in (3, 4, 65, 300):
        rp, ci, _ = _complete(n)
        K = ctx.upload(rp, ci, n)
        assert ctx.triangle_count(K) == n * (n - 1) * (n - 2) // 6
        K.free()
    # bipartite: no odd cycle
    rng = np.random.default_rng(9)
    left, right = rng.integers(0, 500, size=6000), rng.integers(500, 1300, size=6000)
    rp, ci = symmetrise(*gen._csr_from_pairs(left, right, 1300), 1300)
    B = ctx.upload(rp, ci, 1300)
    assert ctx.triangle_count(B) == 0
    B.free()
    E = ctx.upload(np.zeros(11, np.int32), np.zeros(0, np.int32), 10)
    assert ctx.triangle_count(E) == 0
    E.free()


# ---------------------------------------------------------------- k-truss --------------------------------------------
def _truss(ctx, A, k, max_iter=0):
    T, it, conv = ctx.ktruss(A, k, max_iter)
    got = T.download()
    shape = (T.rows, T.cols, T.nnz)
    T.free()
    return got, it, conv, shape


@pytest.mark.parametrize("kind", ["rmat12", "powerlaw", "uniform"])
def test_ktruss(ctx, kind):
    rp, ci, n = _graph(kind)
    n_rp, n_ci = _noisy(rp, ci, n, 6)
    n_rp, n_ci = symmetrise(n_rp, n_ci, n) if kind == "uniform" else (n_rp, n_ci)
    A = ctx.upload(n_rp, n_ci, n)
    # a k for the empty truss: a count is at most its row's length, so k - 2 above the longest row of S0 keeps nothing
    (s_rp, s_ci), _, _ = ktruss_ref(n_rp, n_ci, n, 2)
    big = int(np.diff(s_rp).max()) + 3
    bad, sizes = [], []
    try:
        for k in (2, 3, 4, 5, 8, big):
            (e_rp, e_ci), e_it, e_conv = ktruss_ref(n_rp, n_ci, n, k)
            (g_rp, g_ci), it, conv, shape = _truss(ctx, A, k)
            sizes.append(e_ci.size)
            if shape != (n, n, e_ci.size) or not bspgemm.csr_equal(g_rp, g_ci, e_rp, e_ci) or (it, conv) != (e_it, e_conv):
                bad.append("k=%d: nnz %d it %d conv %s, expected %d %d %s" % (k, shape[2], it, conv, e_ci.size, e_it, e_conv))
    finally:
        A.free()
    assert not bad, bad
    assert sizes[-1] == 0 and sizes[0] > 0 and sizes == sorted(sizes, reverse=True)
    _still_usable(ctx, rp, ci, n)


def test_ktruss_complete_graph(ctx):
    for n in (5, 40):
        rp, ci, _ = _complete(n)
        K = ctx.upload(rp, ci, n)
        (g_rp, g_ci), it, conv, _ = _truss(ctx, K, n)
        assert bspgemm.csr_equal(g_rp, g_ci, rp, ci) and (it, conv) == (1, True)
        (g_rp, g_ci), it, conv, shape = _truss(ctx, K, n + 1)
        assert shape == (n, n, 0) and not g_rp.any() and (it, conv) == (1, True)
        K.free()


def test_ktruss_iteration_cap(ctx):
    rp, ci, n = _graph("powerlaw")
    k = next(k for k in (4, 5, 6, 8) if ktruss_ref(rp, ci, n, k)[1] > 2)
    A = ctx.upload(rp, ci, n)
    for cap in (1, 2):
        (e_rp, e_ci), e_it, e_conv = ktruss_ref(rp, ci, n, k, max_iter=cap)
        (g_rp, g_ci), it, conv, _ = _truss(ctx, A, k, cap)
        assert (e_it, e_conv) == (cap, False) and (it, conv) == (cap, False)
        assert bspgemm.csr_equal(g_rp, g_ci, e_rp, e_ci)
    # NULL iterations / converged are allowed
    out = C.c_void_p()
    assert bspgemm.lib().bspgemm_ktruss(ctx._h, A._h, k, 0, C.byref(out), None, None) == 0 and out.value
    bspgemm.lib().bspgemm_matrix_free(out)
    A.free()


def test_ktruss_non_symmetric_input(ctx):
    """a directed pattern: T is the fixpoint of the stated iteration, nothing more"""
    rp, ci, n = gen.rmat(11, 24, (0.45, 0.22, 0.22, 0.11), 7301)
    A = ctx.upload(rp, ci, n)
    for k in (2, 3, 4):
        (e_rp, e_ci), e_it, e_conv = ktruss_ref(rp, ci, n, k)
        (g_rp, g_ci), it, conv, _ = _truss(ctx, A, k)
        assert bspgemm.csr_equal(g_rp, g_ci, e_rp, e_ci) and (it, conv) == (e_it, e_conv), k
    assert e_ci.size > 0
    A.free()


def test_errors(ctx):
    L = bspgemm.lib()
    rp, ci = gen.uniform_rect(300, 200, 5, 7401)
    R = ctx.upload(rp, ci, 200)                       # 300 x 200
    s_rp, s_ci, n = _graph("uniform")
    A = ctx.upload(s_rp, s_ci, n)
    other = bspgemm.Context(0)
    Ao = other.upload(s_rp, s_ci, n)
    try:
        for M, k, c in ((R, 3, ctx), (A, 1, ctx), (A, 0, ctx), (A, -3, ctx), (Ao, 3, ctx), (A, 3, other)):
            out, it, conv = C.c_void_p(1), C.c_int(5), C.c_int(5)
            assert L.bspgemm_ktruss(c._h, M._h, k, 0, C.byref(out), C.byref(it), C.byref(conv)) == ERR_INVALID
            assert not out.value
        for M, c in ((R, ctx), (Ao, ctx), (A, other)):
            t = C.c_int64(-9)
            assert L.bspgemm_triangle_count(c._h, M._h, C.byref(t)) == ERR_INVALID and t.value == -9
        with pytest.raises(bspgemm.BspgemmError):
            ctx.ktruss(R, 3)
        with pytest.raises(bspgemm.BspgemmError):
            ctx.triangle_count(R)
        # both contexts go on working
        assert ctx.triangle_count(A) == triangles_ref(s_rp, s_ci, n) == other.triangle_count(Ao)
    finally:
        for h in (R, A):
            h.free()
        Ao.free()
        other.close()
    _still_usable(ctx, s_rp, s_ci, n)
