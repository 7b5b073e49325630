"""The device-resident k-core decomposition (bspgemm_core_numbers, bspgemm_kcore): the core numbers against the numpy
peeling of kcore_ref.py, bit for bit, with the degeneracy and the number of peel launches, and the k-core operand against
the induced subgraph.

What can go wrong is the frontier: the wave-aggregated appends of the scan and of the peel waves (the spiders: 63, 65 and
257 vertices appended at once, by one launch's scan and by as many different peel waves), the one wave that strides over a
frontier vertex's row (the cliques: rows of 63, 64 and 65 entries around a wave's step; the stars: a 5000-entry row, and
5000 atomics on one address), the jump of the level over empty ones (clique_tail, rmat12) and consecutive levels with
nothing to jump (cliques2_40), a long run of two-vertex frontiers (path4099_permuted), and vertex counts that are no
multiple of 4, 64 or 256, the scan's workgroups (the chains) -- each at the smallest size that still has the property.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import gen
import kcore_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(rp, ci, n) of the named graph; computed once"""
    return kcore_ref.GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(core, degeneracy, rounds) of the reference; computed once and read-only"""
    core, top, rounds = kcore_ref.core_numbers(*_graph(name))
    core.setflags(write=False)
    return core, top, rounds


def _check(ctx, A, exp, what=""):
    """run the call on operand A and compare everything; returns (values, degeneracy, rounds)"""
    e_core, e_top, e_rounds = exp
    n = e_core.size
    R, top, rounds = ctx.core_numbers(A)
    try:
        assert (R.rows, R.nnz) == (n, n), what
        rp, ci = R.download()
        assert rp.dtype == np.int64 and np.array_equal(rp, np.arange(n + 1)), what
        assert ci.dtype == np.int32 and np.array_equal(ci, np.arange(n)), what
        core = R.download_values()
        assert core.dtype == np.int32 and np.array_equal(core, e_core), what
        assert (top, rounds) == (e_top, e_rounds), (what, top, rounds, e_top, e_rounds)
        assert R.values_sum() == int(e_core.sum(dtype=np.int64)), what
    finally:
        R.free()
    return core, top, rounds


# ---------------------------------------------------------------- 1. every named graph against the reference ----------
@pytest.mark.parametrize("name", list(kcore_ref.GRAPHS))
def test_core_numbers_equal_the_reference(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        core, top, rounds = _check(ctx, A, _expected(name), name)
        if name.startswith("empty") or name == "self_loop":
            assert not core.any() and (top, rounds) == (0, 0)
    finally:
        A.free()


# ---------------------------------------------------------------- 2. where the operand comes from ----------------------
def test_operand_provenance(ctx):
    """an upload, an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment, the transpose, a product
    turned operand, a select and an already symmetrized operand: the same numbers"""
    import torch
    name = "rmat12"
    rp, ci, n = _graph(name)
    exp = _expected(name)
    A = ctx.upload(rp, ci, n)
    _check(ctx, A, exp, "upload")
    extra = gen.uniform_rect(37, n, 3, 5450)
    tall_rp = np.concatenate([extra[0], extra[0][-1] + rp[1:]]).astype(np.int32)
    tall_ci = np.concatenate([extra[1], ci]).astype(np.int32)
    I = ctx.upload(tall_rp, tall_ci, n, row0=37, rows=n)
    _check(ctx, I, exp, "interior upload")
    trp = torch.from_numpy(rp).cuda()
    buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + ci.size] = torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    tci = buf[1:]
    assert tci.data_ptr() % 16 == 4
    W = ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf))
    _check(ctx, W, exp, "wrapped, col_idx 4 bytes off alignment")
    T = ctx.transpose(A)
    _check(ctx, T, exp, "transpose")
    U = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(U, A)
    M = ctx.matrix_from_result(R, n)
    R.free()
    _check(ctx, M, exp, "matrix_from_result")
    S = ctx.select(A, "offdiag")
    _check(ctx, S, exp, "select")
    Y = ctx.symmetrize(A, drop_diagonal=True)
    _check(ctx, Y, exp, "symmetrized")
    for h in (A, I, W, T, U, M, S, Y):
        h.free()


# ---------------------------------------------------------------- 3. repeatability, statistics -------------------------
def test_two_calls_give_identical_downloads(ctx):
    rp, ci, n = _graph("rmat12")
    A = ctx.upload(rp, ci, n)
    try:
        first = _check(ctx, A, _expected("rmat12"), "first")
        second = _check(ctx, A, _expected("rmat12"), "second")
        assert np.array_equal(first[0], second[0]) and first[1:] == second[1:]
    finally:
        A.free()


def test_multiply_statistics_are_untouched(ctx):
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    try:
        before = ctx.stats()
        _check(ctx, A, _expected("rmat10"), "stats")
        assert ctx.stats() == before and before["rows"] == n
    finally:
        R.free()
        A.free()


# ---------------------------------------------------------------- 4. composition ----------------------------------------
def test_selectors_of_the_core_and_the_shell(ctx):
    rp, ci, n = _graph("rmat10")
    core, top, _ = _expected("rmat10")
    A = ctx.upload(rp, ci, n)
    R, _, _ = ctx.core_numbers(A)
    try:
        E = ctx.matrix_from_result(R, n)
        e_rp, e_ci = E.download()
        E.free()
        assert np.array_equal(e_rp, np.arange(n + 1)) and np.array_equal(e_ci, np.arange(n))   # the identity
        for cmp, k in ((">=", 0), (">=", 1), (">=", 3), (">=", top), (">=", top + 1), ("==", 0), ("==", 2), ("==", top)):
            D = ctx.matrix_from_result_where(R, n, cmp, k)
            d_rp, d_ci = D.download()
            D.free()
            inside = core >= k if cmp == ">=" else core == k
            assert (D.rows, D.cols) == (n, n) and np.array_equal(d_ci, np.flatnonzero(inside)), (cmp, k)
            assert np.array_equal(np.diff(d_rp), inside.astype(np.int32)), (cmp, k)
    finally:
        R.free()
        A.free()


@pytest.mark.parametrize("name", ["rmat10", "untidy300"])
def test_kcore_equals_the_induced_subgraph(ctx, name):
    rp, ci, n = _graph(name)
    core, top, _ = _expected(name)
    A = ctx.upload(rp, ci, n)
    try:
        for k in sorted({0, 1, 2, max(top // 2, 1), top, top + 1}):
            T, got_top = ctx.kcore(A, k)
            try:
                e_rp, e_ci = kcore_ref.kcore(rp, ci, n, k)
                t_rp, t_ci = T.download()
                assert (T.rows, T.cols, T.nnz, got_top) == (n, n, e_ci.size, top), k
                assert t_rp.dtype == np.int32 and np.array_equal(t_rp, e_rp), k
                assert t_ci.dtype == np.int32 and np.array_equal(t_ci, e_ci), k
                lens = np.diff(t_rp)
                assert (lens[lens > 0] >= k).all(), k
                if k == top + 1:                             # empty, and still an operand
                    assert T.nnz == 0
                    P = ctx.multiply(A, T)
                    Q = ctx.multiply(T, A)
                    assert (P.rows, P.nnz, Q.rows, Q.nnz) == (n, 0, n, 0)
                    P.free()
                    Q.free()
                elif k >= 1:                                 # the core numbers inside T are at least k on T's vertices
                    R, t_top, _ = ctx.core_numbers(T)
                    inner = R.download_values()
                    R.free()
                    assert t_top == top and (inner[lens > 0] >= k).all() and not inner[lens == 0].any(), k
                    assert np.array_equal(inner[core >= k], core[core >= k]), k
            finally:
                T.free()
    finally:
        A.free()


# ---------------------------------------------------------------- 5. errors --------------------------------------------
def test_errors_leave_no_result_and_a_usable_context(ctx):
    import torch
    L = bspgemm.lib()
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                          # 10 x n
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)
    trp = torch.from_numpy(rp).cuda()
    wrapped = []
    for at, col in ((ci.size // 2, n), (ci.size - 1, -1), (0, 2**31 - 1)):   # checked on the device before it indexes
        c = ci.copy()
        c[at] = col
        tci = torch.from_numpy(c).cuda()
        wrapped.append(ctx.wrap_device(n, n, c.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, tci)))
    torch.cuda.synchronize()

    def numbers(a):
        out, top, rounds = C.c_void_p(0x5A5A), C.c_int(7), C.c_int(7)
        st = L.bspgemm_core_numbers(ctx._h, a._h, C.byref(out), C.byref(top), C.byref(rounds))
        return st, out.value, L.bspgemm_last_error().decode()

    def kcore(a, k=2):
        out, top = C.c_void_p(0x5A5A), C.c_int(7)
        st = L.bspgemm_kcore(ctx._h, a._h, k, C.byref(out), C.byref(top))
        return st, out.value, L.bspgemm_last_error().decode()

    try:
        for call, who in ((numbers, "bspgemm_core_numbers"), (kcore, "bspgemm_kcore")):
            st, out, msg = call(rect)
            assert st == ERR_INVALID and not out and who in msg and "square" in msg, msg
            st, out, msg = call(foreign)
            assert st == ERR_INVALID and not out and who in msg and "context" in msg, msg
            for W in wrapped:
                st, out, msg = call(W)
                assert st == ERR_INVALID and not out and "column" in msg, msg
        st, out, msg = kcore(A, -1)
        assert st == ERR_INVALID and not out and "bspgemm_kcore" in msg and "k < 0" in msg, msg
        # the context still multiplies correctly, and still peels
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        _check(ctx, A, _expected("rmat10"), "after the errors")
    finally:
        for h in wrapped:
            h.free()
        foreign.free()
        other.close()
        rect.free()
        A.free()
