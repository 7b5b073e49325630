"""The device-resident graph colouring (bspgemm_graph_coloring): the colours against the numpy model of color_ref.py, bit
for bit, with the number of colours and the number of frontier launches, under all three orders.

What can go wrong is the frontier wave: its 64-entry step over a row (the cliques: rows of 63, 64 and 65 entries), the
wave-aggregated appends (the spiders: 63, 65 and 257 vertices released at once), one wave that releases 5000 vertices and
5000 waves that lower one counter (the stars), a long run of tiny frontiers (the paths), vertex counts that are no multiple
of 4, 64 or 256 (the chains), and the window of 2048 colours of the LDS bitmap: its last bit and the first bit of the next
window (cliques of 2048 and 2060 vertices), a mark above the window and a mark below its base, which must both be ignored,
and the second walk of a row, which must not release anybody again -- each at the smallest size that still has the
property.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import color_ref
import gen
import scc_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
SEED = 11
NAME = "bspgemm_graph_coloring"


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(rp, ci, n) of the named graph; computed once"""
    return (color_ref.GRAPHS.get(name) or color_ref.WINDOW_GRAPHS[name])()


@functools.lru_cache(maxsize=None)
def _expected(name, order, seed=SEED):
    """(colour, ncolors, rounds) of the model; computed once and read-only"""
    colour, ncolors, rounds = color_ref.coloring(*_graph(name), order=order, seed=seed)
    colour.setflags(write=False)
    return colour, ncolors, rounds


def _check(ctx, A, exp, order, seed=SEED, what=""):
    """run the call on operand A and compare everything; returns (colour, ncolors, rounds)"""
    e_colour, e_ncolors, e_rounds = exp
    n = e_colour.size
    P, ncolors, rounds = ctx.graph_coloring(A, order, seed)
    try:
        assert (P.rows, P.cols, P.nnz) == (n, n, n), what
        rp, colour = P.download()
        assert rp.dtype == np.int32 and np.array_equal(rp, np.arange(n + 1)), what
        assert colour.dtype == np.int32 and np.array_equal(colour, e_colour), (what, order, np.flatnonzero(colour != e_colour)[:8])
        assert (ncolors, rounds) == (e_ncolors, e_rounds), (what, order, ncolors, rounds, e_ncolors, e_rounds)
    finally:
        P.free()
    return colour, ncolors, rounds


# ---------------------------------------------------------------- 1. every named graph against the model --------------
@pytest.mark.parametrize("name", color_ref.SMALL)
def test_colours_equal_the_model(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for order in color_ref.ORDERS:
            colour, ncolors, rounds = _check(ctx, A, _expected(name, order), order, what=name)
            if name.startswith("empty") or name == "self_loop":
                assert not colour.any() and (ncolors, rounds) == (min(n, 1), 0)
    finally:
        A.free()


def test_the_stars_and_the_path_take_the_rounds_they_are_built_for(ctx):
    """one wave releases 5000 vertices (the hub first: LARGEST_FIRST), 5000 waves lower one counter (the hub last: NATURAL),
    a run of 200 one-vertex frontiers"""
    assert _expected("star_hub_last", "largest")[1:] == (2, 2) and _expected("star_hub_last", "largest")[0][5000] == 0
    assert _expected("star_hub_last", "natural")[1:] == (2, 2) and _expected("star_hub_last", "natural")[0][5000] == 1
    assert _expected("path200", "natural")[1:] == (2, 200)


# ---------------------------------------------------------------- 2. the window of the bitmap --------------------------
@pytest.mark.parametrize("order", ["natural", "random"])
def test_last_bit_of_window_0_and_first_bit_of_window_1(ctx, order):
    name = "cliques2048_2060"
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        colour, ncolors, rounds = _check(ctx, A, _expected(name, order), order, what=name)
        assert (ncolors, rounds) == (color_ref.CLIQUE, color_ref.CLIQUE)
        assert np.array_equal(np.sort(colour[:color_ref.WINDOW]), np.arange(color_ref.WINDOW))
        assert np.array_equal(np.sort(colour[color_ref.WINDOW:]), np.arange(color_ref.CLIQUE))
    finally:
        A.free()


def test_a_mark_above_the_window_is_ignored(ctx):
    name, K = "window_above", color_ref.CLIQUE
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        colour, ncolors, rounds = _check(ctx, A, _expected(name, "natural"), "natural", what=name)
        assert np.array_equal(colour[:K], np.arange(K)) and colour[K] == 10 and (ncolors, rounds) == (K, K + 1)
    finally:
        A.free()


def test_a_mark_below_the_base_is_ignored_and_the_release_is_not_repeated(ctx):
    name, K, W = "window_below", color_ref.CLIQUE, color_ref.WINDOW
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        colour, ncolors, rounds = _check(ctx, A, _expected(name, "natural"), "natural", what=name)
        assert np.array_equal(colour[:K], np.arange(K)) and colour[K:].tolist() == [10, W, 0]
        assert (ncolors, rounds) == (K, K + 1)
    finally:
        A.free()


# ---------------------------------------------------------------- 3. where the operand comes from ----------------------
def test_operand_provenance(ctx):
    """an upload, an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment, the transpose, a product
    turned operand, a select, an already symmetrized operand and the transposed (in-edge) storage: the same colours"""
    import torch
    name = "rmat12"
    rp, ci, n = _graph(name)
    handles = []

    def both(M, what):
        handles.append(M)
        for order in ("random", "largest"):
            _check(ctx, M, _expected(name, order), order, what=what)

    A = ctx.upload(rp, ci, n)
    both(A, "upload")
    extra = gen.uniform_rect(37, n, 3, 5450)
    tall_rp = np.concatenate([extra[0], extra[0][-1] + rp[1:]]).astype(np.int32)
    tall_ci = np.concatenate([extra[1], ci]).astype(np.int32)
    both(ctx.upload(tall_rp, tall_ci, n, row0=37, rows=n), "interior upload")
    trp = torch.from_numpy(rp).cuda()
    buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + ci.size] = torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    tci = buf[1:]
    assert tci.data_ptr() % 16 == 4
    both(ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf)), "wrapped, col_idx 4 bytes off alignment")
    both(ctx.transpose(A), "transpose")
    U = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(U, A)
    both(ctx.matrix_from_result(R, n), "matrix_from_result")
    R.free()
    both(ctx.select(A, "offdiag"), "select")
    both(ctx.symmetrize(A, drop_diagonal=True), "symmetrized")
    t_rp, t_ci, _ = scc_ref.transposed(rp, ci, n)
    both(ctx.upload(t_rp, t_ci, n), "in-edge storage")
    for h in handles + [U]:
        h.free()


# ---------------------------------------------------------------- 4. through the library's own calls -------------------
def test_the_classes_through_transpose_and_products(ctx):
    name, order = "rmat12", "random"
    rp, ci, n = _graph(name)
    e_colour, e_ncolors, _ = _expected(name, order)
    srp, sci = color_ref.simple(rp, ci, n)
    A = ctx.upload(rp, ci, n)
    P, ncolors, _ = ctx.graph_coloring(A, order, SEED)
    S = ctx.symmetrize(A, drop_diagonal=True)
    T = ctx.transpose(P)
    R1 = ctx.multiply(T, S)
    M1 = ctx.matrix_from_result(R1, n)
    R2 = ctx.multiply(M1, P)
    try:
        # P^T * S * P: the class-adjacency matrix, with an empty diagonal
        q_rp, q_ci = R2.download()
        rows = np.repeat(np.arange(n), np.diff(q_rp))
        assert q_ci.size > 0 and not (rows == q_ci).any()
        assert not np.diff(q_rp)[ncolors:].any() and q_ci.max() < ncolors
        # transpose(P): the classes, ascending
        t_rp, t_ci = T.download()
        assert np.array_equal(np.diff(t_rp), np.bincount(e_colour, minlength=n))
        assert np.array_equal(t_ci, np.argsort(e_colour, kind="stable"))
        # row 0: independent and maximal
        mis = np.zeros(n, bool)
        mis[t_ci[t_rp[0]:t_rp[1]]] = True
        s_rows = np.repeat(np.arange(n), np.diff(srp))
        assert not (mis[s_rows] & mis[sci]).any()
        assert (mis | (np.bincount(s_rows[mis[sci]], minlength=n) > 0)).all()
    finally:
        for h in (R2, M1, R1, T, S, P, A):
            h.free()


# ---------------------------------------------------------------- 5. seeds, repeatability, statistics ------------------
def test_seeds_and_repeatability(ctx):
    name = "rmat12"
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for order in ("random", "largest"):
            a = _check(ctx, A, _expected(name, order, 1), order, seed=1, what="seed 1")
            b = _check(ctx, A, _expected(name, order, 2), order, seed=2, what="seed 2")
            assert not np.array_equal(a[0], b[0]), order
        big = _check(ctx, A, _expected(name, "random", 0xFFFFFFFF), "random", seed=0xFFFFFFFF, what="seed 2^32 - 1")
        assert not np.array_equal(big[0], _expected(name, "random", 1)[0])
        x = _check(ctx, A, _expected(name, "natural"), "natural", seed=1, what="natural, seed 1")
        y = _check(ctx, A, _expected(name, "natural"), "natural", seed=99, what="natural, seed 99")
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]
        first = _check(ctx, A, _expected(name, "random"), "random", what="first")
        second = _check(ctx, A, _expected(name, "random"), "random", what="second")
        assert np.array_equal(first[0], second[0]) and first[1:] == second[1:]
    finally:
        A.free()


def test_optional_outputs_may_be_null(ctx):
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    out = C.c_void_p()
    try:
        assert bspgemm.lib().bspgemm_graph_coloring(ctx._h, A._h, 2, SEED, C.byref(out), None, None) == 0
        colour = np.zeros(n, np.int32)
        assert bspgemm.lib().bspgemm_matrix_download(ctx._h, out, None, colour.ctypes.data) == 0
        assert np.array_equal(colour, _expected("rmat10", "random")[0])
    finally:
        bspgemm.lib().bspgemm_matrix_free(out)
        A.free()


def test_multiply_statistics_are_untouched(ctx):
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    try:
        before = ctx.stats()
        _check(ctx, A, _expected("rmat10", "random"), "random", what="stats")
        assert ctx.stats() == before and before["rows"] == n
    finally:
        R.free()
        A.free()


# ---------------------------------------------------------------- 6. errors --------------------------------------------
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

    def call(a, order=2):
        out, colors, rounds = C.c_void_p(0x5A5A), C.c_int(7), C.c_int(7)
        st = L.bspgemm_graph_coloring(ctx._h, a._h, order, SEED, C.byref(out), C.byref(colors), C.byref(rounds))
        return st, out.value, L.bspgemm_last_error().decode(), (colors.value, rounds.value)

    try:
        st, out, msg, counts = call(rect)
        assert st == ERR_INVALID and not out and NAME in msg and "square" in msg and counts == (0, 0), msg
        st, out, msg, counts = call(foreign)
        assert st == ERR_INVALID and not out and NAME in msg and "context" in msg and counts == (0, 0), msg
        for order in (0, 4, -3):
            st, out, msg, counts = call(A, order)
            assert st == ERR_INVALID and not out and NAME in msg and "order" in msg and counts == (0, 0), msg
        for W in wrapped:
            st, out, msg, counts = call(W)
            assert st == ERR_INVALID and not out and "column" in msg and counts == (0, 0), msg
        with pytest.raises(ValueError):
            ctx.graph_coloring(A, "smallest-last")
        # the context still multiplies correctly, and still colours
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        _check(ctx, A, _expected("rmat10", "random"), "random", what="after the errors")
    finally:
        for h in wrapped:
            h.free()
        foreign.free()
        other.close()
        rect.free()
        A.free()
