"""The device-resident strongly connected components (bspgemm_strongly_connected_components): the label array against
scipy's strong components relabelled to the smallest vertex id (scc_ref.py), bit for bit, the component count, the
assignment operand's row_ptr and the number of colouring rounds.

What can go wrong is the three entry-parallel sweeps, which work in tiles of 4096 stored entries, four per lane, whatever
rows they belong to, the trimming that has to reach its fixpoint before and after every round, the backward step that must
stay inside its own component, and the vertex passes in workgroups of 256.  So the shapes are long cycles and paths in good
and bad id order, chains of components that share a colour, entry counts on both sides of one and two tiles, hub rows that
span tiles, a tile whose rows are too many to stage, and untidy rows -- each at the smallest size that still has the
property.  The component counts, largest components and rounds below come from a host model of the sweeps in which every
load of a launch sees the launch boundary.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import cc_ref
import gen
import scc_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
NAME = "bspgemm_strongly_connected_components"
SKEW = (0.57, 0.19, 0.19, 0.05)

GRAPHS = {
    "cycle200": lambda: scc_ref.cycle(200),
    "cycle200_reversed": lambda: scc_ref.cycle_reversed(200),
    "path200": lambda: scc_ref.path(200),
    "path4099_permuted": lambda: scc_ref.path_permuted(4099, 5410),
    "two_cycles_down": lambda: scc_ref.two_cycles(50, "down"),
    "two_cycles_up": lambda: scc_ref.two_cycles(50, "up"),
    "ladder_down": lambda: scc_ref.ladder(100, "down"),
    "ladder_up": lambda: scc_ref.ladder(100, "up"),
    "tails": lambda: scc_ref.tails(),
    "rmat12": lambda: gen.rmat(12, 8, SKEW, 5401),
    "rmat10": lambda: gen.rmat(10, 6, SKEW, 5403),
    "powerlaw": lambda: gen.powerlaw(6000, 3, 5402),
    "uniform300": lambda: gen.uniform(300, 2, 5404),
    "cycles_4095": lambda: scc_ref.four_cycles(4095, 5600 + 4095)[:3],
    "cycles_4096": lambda: scc_ref.four_cycles(4096, 5600 + 4096)[:3],
    "cycles_4097": lambda: scc_ref.four_cycles(4097, 5600 + 4097)[:3],
    "cycles_8195": lambda: scc_ref.four_cycles(8195, 5600 + 8195)[:3],
    "star_out_hub_last": lambda: scc_ref.star(5001, 5000, "hub"),
    "star_out_hub_middle": lambda: scc_ref.star(5001, 2500, "hub"),
    "star_both_hub_last": lambda: scc_ref.star_both(5001, 5000),
    "star_both_hub_middle": lambda: scc_ref.star_both(5001, 2500),
    "sparse_far_rows": lambda: scc_ref.sparse_far_rows(20000, 250, 12, 5420),
    "untidy300": lambda: scc_ref.untidy(300, 5440),
    "untidy300_singletons": lambda: cc_ref.untidy(300, 5440),
    "empty0": lambda: (np.zeros(1, np.int32), np.zeros(0, np.int32), 0),
    "empty1": lambda: (np.zeros(2, np.int32), np.zeros(0, np.int32), 1),
    "empty4": lambda: (np.zeros(5, np.int32), np.zeros(0, np.int32), 4),
    "empty1000": lambda: (np.zeros(1001, np.int32), np.zeros(0, np.int32), 1000),
    "self_loop": lambda: (np.array([0, 1], np.int32), np.zeros(1, np.int32), 1),
}
# name: (components, largest component, colouring rounds)
SHAPE = {
    "cycle200": (1, 200, 1), "cycle200_reversed": (1, 200, 1), "path200": (200, 1, 0), "path4099_permuted": (4099, 1, 0),
    "two_cycles_down": (2, 50, 2), "two_cycles_up": (2, 50, 1), "ladder_down": (100, 2, 100), "ladder_up": (100, 2, 1),
    "tails": (42, 30, 1), "rmat12": (1986, 2111, 1), "rmat10": (490, 535, 1), "powerlaw": (3758, 2243, 1),
    "uniform300": (74, 227, 1), "star_out_hub_last": (5001, 1, 0), "star_out_hub_middle": (5001, 1, 0),
    "star_both_hub_last": (1, 5001, 1), "star_both_hub_middle": (1, 5001, 1), "untidy300_singletons": (300, 1, 0),
    "empty0": (0, 0, 0), "empty1": (1, 1, 0), "empty4": (4, 1, 0), "empty1000": (1000, 1, 0), "self_loop": (1, 1, 0),
}


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
    label, count = scc_ref.labels(*_graph(name))
    label.setflags(write=False)
    return label, count


def _check(ctx, A, exp, what="", rounds_exp=None):
    """run the call on operand A and compare everything; returns (labels, ncomponents, rounds, sweeps)"""
    e_label, e_count = exp
    n = e_label.size
    P, count, rounds, sweeps = ctx.strongly_connected_components(A)
    try:
        assert (P.rows, P.cols, P.nnz) == (n, n, n), what
        rp, label = P.download()
        assert rp.dtype == np.int32 and np.array_equal(rp, np.arange(n + 1)), what
        assert label.dtype == np.int32 and np.array_equal(label, e_label), what
        assert count == e_count, what
        if rounds_exp is not None:
            assert rounds == rounds_exp, (what, rounds)
        if A.nnz == 0:
            assert (rounds, sweeps) == (0, 0), what
        else:
            # the caps: n rounds, n + 2 repetitions of the trim loop in front of every round and behind the last one, and
            # of the forward and the backward loop of every round
            assert 0 <= rounds <= n and 1 <= sweeps <= (3 * rounds + 1) * (n + 2), (what, rounds, sweeps)
    finally:
        P.free()
    return label, count, rounds, sweeps


def _run_named(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        return _check(ctx, A, _expected(name), name, SHAPE[name][2] if name in SHAPE else None)
    finally:
        A.free()


# ---------------------------------------------------------------- 1. every shape against the reference -----------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_labels_equal_the_reference(ctx, name):
    rp, ci, n = _graph(name)
    e_label, e_count = _expected(name)
    if name in SHAPE:
        assert (e_count, scc_ref.largest(e_label)) == SHAPE[name][:2]
    if name.startswith("cycles_"):
        assert ci.size == int(name[7:]) and n % 4 != 0
    if name.startswith("star_"):
        assert ci.size in (5000, 10000) and int(np.diff(rp).max()) == 5000 > scc_ref.K_SEL_TILE
    if name == "untidy300":
        assert scc_ref.largest(e_label) >= 10
    label, count, rounds, sweeps = _run_named(ctx, name)
    if name.startswith("empty"):
        assert np.array_equal(label, np.arange(n)) and count == n
    if name == "self_loop":
        assert sweeps >= 1                                               # the column check alone costs one sweep


def test_sizes_that_are_no_multiple_of_the_vertex_tiles(ctx):
    """n % 4, n % 64 and n % 256 all non-zero, with components that straddle the 256-vertex workgroups of the vertex passes"""
    for n in (257, 1023, 4099):
        rp, ci, _ = scc_ref.three_cycles(n)
        assert n % 4 and n % 64 and n % 256
        exp = scc_ref.labels(rp, ci, n)
        assert exp[1] == 3 and np.array_equal(exp[0], np.arange(n) % 3)
        A = ctx.upload(rp, ci, n)
        try:
            _check(ctx, A, exp, "three cycles of n = %d" % n, 1)
        finally:
            A.free()


# ---------------------------------------------------------------- 2. where the operand comes from ----------------------
def test_operand_provenance(ctx):
    """an upload, an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment, a product turned operand,
    a select -- and the transpose: a graph and its transpose have the same strongly connected components"""
    import torch
    name = "rmat12"
    rp, ci, n = _graph(name)
    exp = _expected(name)
    rounds = SHAPE[name][2]
    A = ctx.upload(rp, ci, n)
    _check(ctx, A, exp, "upload", rounds)
    # the same rows inside a taller host CSR: absolute row_ptr values, col_idx from its start
    extra = gen.uniform_rect(37, n, 3, 5450)
    tall_rp = np.concatenate([extra[0], extra[0][-1] + rp[1:]]).astype(np.int32)
    tall_ci = np.concatenate([extra[1], ci]).astype(np.int32)
    I = ctx.upload(tall_rp, tall_ci, n, row0=37, rows=n)
    _check(ctx, I, exp, "interior upload", rounds)
    trp = torch.from_numpy(rp).cuda()
    buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + ci.size] = torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    tci = buf[1:]
    assert tci.data_ptr() % 16 == 4
    W = ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf))
    _check(ctx, W, exp, "wrapped, col_idx 4 bytes off alignment", rounds)
    # a product turned operand: I * A, the same graph with its rows sorted and duplicate-free
    U = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(U, A)
    M = ctx.matrix_from_result(R, n)
    R.free()
    assert M.nnz == ci.size
    _check(ctx, M, exp, "matrix_from_result", rounds)
    S = ctx.select(A, "offdiag")
    _check(ctx, S, exp, "select", rounds)
    T = ctx.transpose(A)
    t_rp, t_ci = T.download()
    e_rp, e_ci, _ = scc_ref.transposed(rp, ci, n)
    assert np.array_equal(t_rp, e_rp) and np.array_equal(t_ci, e_ci) and not np.array_equal(t_ci, ci)
    _check(ctx, T, exp, "transpose", rounds)
    for h in (A, I, W, U, M, S, T):
        h.free()


def test_symmetrized_graph_gives_the_weak_components(ctx):
    """with every edge in both directions strong and weak connectivity coincide: the labels of bspgemm_connected_components,
    bit for bit"""
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    Y = ctx.symmetrize(A)
    Pw, count_w, _ = ctx.connected_components(Y)
    Ps, count_s, rounds, _ = ctx.strongly_connected_components(Y)
    try:
        weak, strong = Pw.download(), Ps.download()
        assert np.array_equal(weak[0], strong[0]) and np.array_equal(weak[1], strong[1]) and count_w == count_s
        assert np.array_equal(strong[1], cc_ref.labels(rp, ci, n)[0]) and 1 < count_s < n
    finally:
        for h in (Ps, Pw, Y, A):
            h.free()


def test_two_calls_give_identical_downloads(ctx):
    rp, ci, n = _graph("rmat12")
    A = ctx.upload(rp, ci, n)
    try:
        first = _check(ctx, A, _expected("rmat12"), "first")
        second = _check(ctx, A, _expected("rmat12"), "second")
        assert np.array_equal(first[0], second[0]) and first[1:3] == second[1:3]
    finally:
        A.free()


# ---------------------------------------------------------------- 3. composition ----------------------------------------
def test_transpose_of_the_assignment_lists_the_members(ctx):
    name = "rmat10"
    rp, ci, n = _graph(name)
    label, _ = _expected(name)
    A = ctx.upload(rp, ci, n)
    P, count, _, _ = ctx.strongly_connected_components(A)
    T = ctx.transpose(P)
    try:
        t_rp, t_ci = T.download()
        e_rp, e_ci = scc_ref.members(label)
        assert np.array_equal(t_rp, e_rp) and np.array_equal(t_ci, e_ci)
        assert int((np.diff(t_rp) > 0).sum()) == count and int(np.diff(t_rp).max()) == SHAPE[name][1]
    finally:
        for h in (T, P, A):
            h.free()


def test_condensation_by_two_multiplies(ctx):
    """P^T * A * P against scipy's pattern of the same triple product; without its diagonal it is a DAG: every strongly
    connected component of it is a single vertex"""
    from scipy.sparse import csr_matrix
    for name in ("uniform300", "rmat10"):
        rp, ci, n = _graph(name)
        label, count = _expected(name)
        A = ctx.upload(rp, ci, n)
        P, got_count, _, _ = ctx.strongly_connected_components(A)
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
            rows = np.repeat(np.arange(n), np.diff(q_rp))
            off = rows != q_ci
            assert off.sum() > 0 and np.isin(rows, label).all() and np.isin(q_ci, label).all()
            d_rp, d_ci, _ = cc_ref.csr(rows[off], q_ci[off], n)
            assert scc_ref.labels(d_rp, d_ci, n)[1] == n
        finally:
            for h in (Q, Xm, X, PT, P, A):
                h.free()


def test_mutual_reachability_equals_the_closure(ctx):
    """T = A* by bspgemm_closure: T and T^T is the pattern of "u reaches v and v reaches u", which is P * P^T -- what a user
    had to compute, with its quadratic output, before this call"""
    L = bspgemm.lib()
    name = "uniform300"
    rp, ci, n = _graph(name)
    label, _ = _expected(name)
    A = ctx.upload(rp, ci, n)
    P, _, _, _ = ctx.strongly_connected_components(A)
    R, _ = ctx.closure(A)
    T = ctx.matrix_from_result(R, n)
    TT = ctx.transpose(T)
    both = ctx.setop(T, TT, "and")
    PT = ctx.transpose(P)
    X = ctx.multiply(P, PT)
    PPT = ctx.matrix_from_result(X, n)
    try:
        eq = C.c_int(-1)
        assert L.bspgemm_matrix_equal(ctx._h, both._h, PPT._h, C.byref(eq)) == 0 and eq.value == 1
        assert both.nnz == int((np.bincount(label) ** 2).sum()) > n
    finally:
        for h in (PPT, X, PT, both, TT, T, R, P, A):
            h.free()


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
    fn = getattr(L, NAME)
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
        out, count, rounds, sweeps = C.c_void_p(0x5A5A), C.c_int(7), C.c_int(7), C.c_int(7)
        st = fn(ctx._h, a._h, C.byref(out), C.byref(count), C.byref(rounds), C.byref(sweeps))
        return st, out.value, L.bspgemm_last_error().decode()

    try:
        st, out, msg = call(rect)
        assert st == ERR_INVALID and not out and NAME in msg and "square" in msg, msg
        st, out, msg = call(foreign)
        assert st == ERR_INVALID and not out and NAME in msg and "context" in msg, msg
        for W in wrapped:
            st, out, msg = call(W)
            assert st == ERR_INVALID and not out and NAME in msg, msg
            assert "column" in msg and "outside [0, %d)" % n in msg, msg
        # the context still multiplies correctly, and still labels
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        _check(ctx, A, _expected("rmat10"), "after the errors", SHAPE["rmat10"][2])
    finally:
        for h in wrapped:
            h.free()
        foreign.free()
        other.close()
        rect.free()
        A.free()
