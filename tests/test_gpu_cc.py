"""The device-resident connected components (bspgemm_connected_components): the label array against scipy's weak
components relabelled to the smallest vertex id (cc_ref.py), bit for bit, and the component count.

What can go wrong is the hook, which works in tiles of 4096 stored entries, four per lane, whatever rows they belong to,
and the chains it builds, which the jump has to flatten.  So the shapes are long chains in good and bad id order, entry
counts on both sides of one and two tiles, hub rows that span tiles, a tile whose rows are too many to stage, edges stored
in one direction only, and untidy rows -- each at the smallest size that still has the property.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import cc_ref
import empty_ref
import gen

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
SKEW = (0.57, 0.19, 0.19, 0.05)

GRAPHS = {
    "path200": lambda: cc_ref.path(200),
    "path200_reversed": lambda: cc_ref.path(200, np.arange(200)[::-1]),
    "path4099_permuted": lambda: cc_ref.path_permuted(4099, 5410),
    "cycle200": lambda: cc_ref.cycle(200),
    "paths_4095": lambda: cc_ref.short_paths(4095, 5500 + 4095),
    "paths_4096": lambda: cc_ref.short_paths(4096, 5500 + 4096),
    "paths_4097": lambda: cc_ref.short_paths(4097, 5500 + 4097),
    "paths_8195": lambda: cc_ref.short_paths(8195, 5500 + 8195),
    "star_hub_last": lambda: cc_ref.star(5001, 5000, "hub"),
    "star_hub_middle": lambda: cc_ref.star(5001, 2500, "hub"),
    "star_leaf_rows": lambda: cc_ref.star(5001, 5000, "leaves"),
    "sparse_far_rows": lambda: cc_ref.sparse_far_rows(20000, 250, 12, 5420),
    "halves_joined_from_first": lambda: cc_ref.two_halves(150, 5430, "first")[:3],
    "halves_joined_from_second": lambda: cc_ref.two_halves(150, 5430, "second")[:3],
    "untidy300": lambda: cc_ref.untidy(300, 5440),
    "rmat12": lambda: gen.rmat(12, 8, SKEW, 5401),
    "rmat10": lambda: gen.rmat(10, 6, SKEW, 5403),
    "powerlaw": lambda: gen.powerlaw(6000, 3, 5402),
    "uniform300": lambda: gen.uniform(300, 2, 5404),
    "empty0": lambda: (np.zeros(1, np.int32), np.zeros(0, np.int32), 0),
    "empty1": lambda: (np.zeros(2, np.int32), np.zeros(0, np.int32), 1),
    "empty4": lambda: (np.zeros(5, np.int32), np.zeros(0, np.int32), 4),
    "empty1000": lambda: (np.zeros(1001, np.int32), np.zeros(0, np.int32), 1000),
    "self_loop": lambda: (np.array([0, 1], np.int32), np.zeros(1, np.int32), 1),
}
COMPONENTS = {"path200": 1, "path200_reversed": 1, "path4099_permuted": 1, "cycle200": 1, "star_hub_last": 1,
              "star_hub_middle": 1, "star_leaf_rows": 1, "halves_joined_from_first": 1, "halves_joined_from_second": 1,
              "rmat12": 1131, "rmat10": 258, "empty0": 0, "empty1": 1, "empty4": 4, "empty1000": 1000, "self_loop": 1}


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(rp, ci, n) of the named graph; computed once"""
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(labels, ncomponents) of the reference; computed once and read-only"""
    label, count = cc_ref.labels(*_graph(name))
    label.setflags(write=False)
    return label, count


def _check(ctx, A, exp, what=""):
    """run the call on operand A and compare everything; returns (labels, ncomponents, rounds)"""
    e_label, e_count = exp
    n = e_label.size
    P, count, rounds = ctx.connected_components(A)
    try:
        assert (P.rows, P.cols, P.nnz) == (n, n, n), what
        rp, label = P.download()
        assert rp.dtype == np.int32 and np.array_equal(rp, np.arange(n + 1)), what
        assert label.dtype == np.int32 and np.array_equal(label, e_label), what
        assert count == e_count, what
        if A.nnz == 0:
            assert rounds == 0, what
        else:
            assert 1 <= rounds <= n + 1, (what, rounds)
    finally:
        P.free()
    return label, count, rounds


def _run_named(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        return _check(ctx, A, _expected(name), name)
    finally:
        A.free()


# ---------------------------------------------------------------- 1. every shape against the reference -----------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_labels_equal_the_reference(ctx, name):
    rp, ci, n = _graph(name)
    if name in COMPONENTS:
        assert _expected(name)[1] == COMPONENTS[name]
    if name.startswith("paths_"):
        assert ci.size == int(name[6:]) and n % 4 != 0
    if name.startswith("star_"):
        assert ci.size == 5000 > cc_ref.K_SEL_TILE
    label, count, rounds = _run_named(ctx, name)
    if name.startswith("empty"):
        assert np.array_equal(label, np.arange(n)) and count == n


@pytest.mark.parametrize("rows,cols", empty_ref.SHAPES, ids=empty_ref.IDS)
def test_graph_without_edges(ctx, rows, cols):
    """0 x 0: P is an operand without entries; 4 x 4: P is the identity, and works at once as B and as A of a product;
    not square: refused, as it always was"""
    A = ctx.upload(*empty_ref.csr(rows), cols)
    try:
        if rows != cols:
            out = C.c_void_p(0x5A5A)
            st = bspgemm.lib().bspgemm_connected_components(ctx._h, A._h, C.byref(out), None, None)
            assert st == ERR_INVALID and not out.value
            return
        P, count, rounds = ctx.connected_components(A)
        assert (count, rounds) == (rows, 0) == (cc_ref.labels(*empty_ref.csr(rows), rows)[1], 0)
        if rows == 0:
            empty_ref.check(ctx, P, 0, 0)
        else:
            G = empty_ref.gather_all(ctx, rows)
            eye = empty_ref.diagonal(rows)
            assert all(np.array_equal(g, e) for g, e in zip(P.download(), eye))
            for X, x in ((G, G.download()), (P, eye)):
                R = ctx.multiply(X, P)
                erp, eci = gen.small_reference(x[0], x[1], eye[0], eye[1])
                grp, gci = R.download()
                assert np.array_equal(grp, erp) and np.array_equal(gci, eci)
                R.free()
            G.free()
        P.free()
    finally:
        A.free()


def test_sizes_that_are_no_multiple_of_the_vertex_tiles(ctx):
    """n % 4, n % 64 and n % 256 all non-zero, with components that straddle the 256-vertex workgroups of the jump"""
    for n in (257, 1023, 4099):
        rp, ci, _ = cc_ref.csr(np.arange(n - 3), np.arange(3, n), n)        # three interleaved chains: v -> v + 3
        assert n % 4 and n % 64 and n % 256
        exp = cc_ref.labels(rp, ci, n)
        assert exp[1] == 3 and np.array_equal(exp[0], np.arange(n) % 3)
        A = ctx.upload(rp, ci, n)
        try:
            _check(ctx, A, exp, "chains of n = %d" % n)
        finally:
            A.free()


# ---------------------------------------------------------------- 2. where the operand comes from ----------------------
def test_operand_provenance(ctx):
    """an upload, an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment, a transpose's output and
    a product turned operand: the same labels (the transpose's too: weak connectivity ignores direction)"""
    import torch
    name = "rmat12"
    rp, ci, n = _graph(name)
    exp = _expected(name)
    A = ctx.upload(rp, ci, n)
    _check(ctx, A, exp, "upload")
    # the same rows inside a taller host CSR: absolute row_ptr values, col_idx from its start
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
    # a product turned operand: I * A, the same graph with its rows sorted and duplicate-free
    U = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(U, A)
    M = ctx.matrix_from_result(R, n)
    R.free()
    assert M.nnz == ci.size
    _check(ctx, M, exp, "matrix_from_result")
    S = ctx.select(A, "offdiag")
    _check(ctx, S, exp, "select")
    Y = ctx.symmetrize(A)
    _check(ctx, Y, exp, "setop (symmetrize)")
    for h in (A, I, W, T, U, M, S, Y):
        h.free()


def test_two_calls_give_identical_downloads(ctx):
    rp, ci, n = _graph("rmat12")
    A = ctx.upload(rp, ci, n)
    try:
        first = _check(ctx, A, _expected("rmat12"), "first")
        second = _check(ctx, A, _expected("rmat12"), "second")
        assert np.array_equal(first[0], second[0]) and first[1] == second[1]
    finally:
        A.free()


# ---------------------------------------------------------------- 3. composition ----------------------------------------
def test_transpose_of_the_assignment_lists_the_members(ctx):
    name = "rmat10"
    rp, ci, n = _graph(name)
    label, _ = _expected(name)
    A = ctx.upload(rp, ci, n)
    P, count, _ = ctx.connected_components(A)
    T = ctx.transpose(P)
    try:
        t_rp, t_ci = T.download()
        e_rp, e_ci = cc_ref.members(label)
        assert np.array_equal(t_rp, e_rp) and np.array_equal(t_ci, e_ci)
        assert int((np.diff(t_rp) > 0).sum()) == count
    finally:
        for h in (T, P, A):
            h.free()


def test_bfs_reaches_exactly_the_component(ctx):
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    Y = ctx.symmetrize(A)
    P, _, _ = ctx.connected_components(Y)
    label = P.download()[1]
    assert np.array_equal(label, _expected("rmat10")[0])
    sources = [int(s) for s in np.random.default_rng(12).choice(n, size=8, replace=False)]
    R, _, complete = ctx.bfs(Y, sources)
    try:
        r_rp, r_ci = R.download()
        assert complete
        for s, src in enumerate(sources):
            assert np.array_equal(r_ci[r_rp[s]:r_rp[s + 1]], np.flatnonzero(label == label[src])), src
    finally:
        for h in (R, P, Y, A):
            h.free()


def _quotient_equals_scipy(ctx, rp, ci, n):
    """P^T * A * P by two multiplies against scipy's pattern of the same triple product; returns its entries"""
    from scipy.sparse import csr_matrix
    label, count = cc_ref.labels(rp, ci, n)
    A = ctx.upload(rp, ci, n)
    P, got_count, _ = ctx.connected_components(A)
    PT = ctx.transpose(P)
    X = ctx.multiply(PT, A)
    Xm = ctx.matrix_from_result(X, n)
    Q = ctx.multiply(Xm, P)
    try:
        assert got_count == count
        q_rp, q_ci = Q.download()
        Pm = csr_matrix((np.ones(n), label, np.arange(n + 1)), shape=(n, n))
        Am = csr_matrix((np.ones(ci.size), ci, rp), shape=(n, n))
        E = (Pm.T @ Am @ Pm).tocsr()
        E.sum_duplicates()
        E.sort_indices()
        assert np.array_equal(q_rp, E.indptr) and np.array_equal(q_ci, E.indices)
        # entries of A stay inside components: the quotient is the diagonal at the labels that have an entry
        has_entry = np.unique(label[np.repeat(np.arange(n), np.diff(rp))])
        assert np.array_equal(q_ci, has_entry) and np.array_equal(np.flatnonzero(np.diff(q_rp)), has_entry)
        return q_ci.size
    finally:
        for h in (Q, Xm, X, PT, P, A):
            h.free()


def test_quotient_graph_by_two_multiplies(ctx):
    rp, ci, n = _graph("uniform300")
    assert _quotient_equals_scipy(ctx, rp, ci, n) == 1                   # one component: the entry (0, 0)
    # the same graph cut into pieces -- only the entries inside blocks of 50 vertices -- so that the quotient has several
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = rows // 50 == ci // 50
    b_rp, b_ci, _ = cc_ref.csr(rows[keep], ci[keep], n)
    assert _quotient_equals_scipy(ctx, b_rp, b_ci, n) >= 6


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


# ---------------------------------------------------------------- 4. errors --------------------------------------------
def test_errors_leave_no_operand_and_a_usable_context(ctx):
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

    def call(a):
        out, count, rounds = C.c_void_p(0x5A5A), C.c_int(7), C.c_int(7)
        st = L.bspgemm_connected_components(ctx._h, a._h, C.byref(out), C.byref(count), C.byref(rounds))
        return st, out.value, L.bspgemm_last_error().decode()

    try:
        st, out, msg = call(rect)
        assert st == ERR_INVALID and not out and "bspgemm_connected_components" in msg and "square" in msg, msg
        st, out, msg = call(foreign)
        assert st == ERR_INVALID and not out and "bspgemm_connected_components" in msg and "context" in msg, msg
        for W in wrapped:
            st, out, msg = call(W)
            assert st == ERR_INVALID and not out and "bspgemm_connected_components" in msg, msg
            assert "column" in msg and "outside [0, %d)" % n in msg, msg
        # the context still multiplies correctly, and still labels
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
