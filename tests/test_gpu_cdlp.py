"""The device-resident label propagation (bspgemm_label_propagation): labels, iterations, converged, changed and
communities against the numpy model of cdlp_ref.py, bit for bit.

What can go wrong is the mode of a gathered multiset, which none of the other sweeps computes, in four kernels that must
agree: the lane's register compare (rows of 1 .. 8 entries), the wave's and the workgroup's sort in LDS (the pads of a
row that is no power of two, the 64-entry step, the run that ends at the row's last element, the tie between two runs),
and the hubs' open-addressing tables (label 0 against the empty slot, colliding probe sequences that wrap, one counter
that takes every addition) -- each at the degrees just below, at and above the cap between two classes, and all of them
against each other through BSPGEMM_OPT_LP_MIN_CLASS.  Beside it: the synchronous update (the paths and stars oscillate, so
an iteration that read a label of its own iteration shows at once), both parities of the iteration count (the result lies
in one of two arrays), ids near n, and isolated vertices, which nobody owns.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import cdlp_ref
import gen
import scc_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
NAME = "bspgemm_label_propagation"
SKEW = (0.57, 0.19, 0.19, 0.05)


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.set_option("lp_min_class", 0)
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    return cdlp_ref.GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def _expected(name, max_iter):
    """the model's five; computed once and read-only"""
    exp = cdlp_ref.label_propagation(*_graph(name), max_iter)
    exp[0].setflags(write=False)
    return exp


@functools.lru_cache(maxsize=None)
def _stars(n_total=None, high=False):
    """the star union, the model's five after one iteration, and class_vertices under every LP_MIN_CLASS"""
    rp, ci, n, initial, hubs, mode = cdlp_ref.star_union(n_total, high=high)
    exp = cdlp_ref.label_propagation(rp, ci, n, 1, initial)
    for a in (initial, exp[0], mode):
        a.setflags(write=False)
    return rp, ci, n, initial, hubs, mode, exp, [cdlp_ref.class_vertices(rp, ci, n, k) for k in range(4)]


def _check(ctx, A, exp, max_iter, initial=None, what=""):
    """run the call on operand A and compare everything; returns (labels, info)"""
    e_labels, e_iterations, e_converged, e_changed, e_communities = exp
    n = e_labels.size
    P, info = ctx.label_propagation(A, max_iter, initial)
    try:
        assert (P.rows, P.cols, P.nnz) == (n, n, n), what
        rp, labels = P.download()
        assert rp.dtype == np.int32 and np.array_equal(rp, np.arange(n + 1)), what
        assert labels.dtype == np.int32 and np.array_equal(labels, e_labels), (what, max_iter, np.flatnonzero(labels != e_labels)[:8])
        got = (info["iterations"], info["converged"], info["changed"], info["communities"])
        assert got == (e_iterations, e_converged, e_changed, e_communities), (what, max_iter, got, exp[1:])
    finally:
        P.free()
    return labels, info


# ---------------------------------------------------------------- 1. every named graph against the model --------------
@pytest.mark.parametrize("name", list(cdlp_ref.GRAPHS))
def test_labels_equal_the_model(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for max_iter in (1, 2, 3, 10):                     # odd and even: the oscillators in both phases, both label arrays
            labels, info = _check(ctx, A, _expected(name, max_iter), max_iter, what=name)
            assert info["class_vertices"] == cdlp_ref.class_vertices(rp, ci, n), name
            if name.startswith("empty") or name == "self_loop":
                assert np.array_equal(labels, np.arange(n)) and (info["iterations"], info["converged"]) == (0, 1)
    finally:
        A.free()


def test_the_named_graphs_do_what_they_are_there_for():
    assert _expected("uniform4096_d8", 10)[1:] == (8, 1, 0, 1) and _expected("cliques64_66", 10)[1:] == (3, 1, 0, 3)
    assert _expected("rmat10", 10)[1:4] == (10, 0, 4)
    for name in ("star_hub_last", "spider257", "path200", "chains4099"):      # every label moves in every iteration
        n = _graph(name)[2]
        assert _expected(name, 3)[1:4] == (3, 0, n) and _expected(name, 10)[1:4] == (10, 0, n)
        assert not np.array_equal(_expected(name, 2)[0], _expected(name, 3)[0])
    assert cdlp_ref.class_vertices(*_graph("star_hub_last"))[3] == 1          # a hub of 5000 entries
    for name in ("chains257", "chains1023", "chains4099"):                    # no multiple of 4, 64 or 256
        assert all(_graph(name)[2] % k for k in (4, 64, 256))


# ---------------------------------------------------------------- 2. the mode, one class boundary at a time ------------
def test_the_mode_at_every_class_boundary(ctx):
    rp, ci, n, initial, hubs, mode, exp, classes = _stars()
    A = ctx.upload(rp, ci, n)
    try:
        labels, info = _check(ctx, A, exp, 1, initial, what="stars")
        assert np.array_equal(labels[hubs], mode)                             # the multisets' modes, from a Counter
        assert info["class_vertices"] == classes[0] and all(c > 0 for c in classes[0])
    finally:
        A.free()


# ---------------------------------------------------------------- 3. the four kernels against each other ---------------
@pytest.mark.parametrize("min_class", [0, 1, 2, 3])
def test_every_class_computes_the_same_function(ctx, min_class):
    rp, ci, n, initial, hubs, mode, exp, classes = _stars()
    assert sum(classes[min_class][:min_class]) == 0 and sum(classes[min_class]) == sum(classes[0])
    A = ctx.upload(rp, ci, n)
    ctx.set_option("lp_min_class", min_class)
    try:
        assert ctx.get_option("lp_min_class") == min_class
        labels, info = _check(ctx, A, exp, 1, initial, what="stars, LP_MIN_CLASS %d" % min_class)
        assert np.array_equal(labels[hubs], mode)
        assert info["class_vertices"] == classes[min_class], (info["class_vertices"], classes[min_class])
        name = "rmat12"                                                       # and a graph that iterates
        B = ctx.upload(*_graph(name))
        try:
            _, info = _check(ctx, B, _expected(name, 3), 3, what="%s, LP_MIN_CLASS %d" % (name, min_class))
            assert info["class_vertices"] == cdlp_ref.class_vertices(*_graph(name), min_class)
        finally:
            B.free()
    finally:
        ctx.set_option("lp_min_class", 0)
        A.free()


def test_the_knob_refuses_what_it_does_not_know(ctx):
    for bad in (-1, 4):
        with pytest.raises(bspgemm.BspgemmError):
            ctx.set_option("lp_min_class", bad)
    assert ctx.get_option("lp_min_class") == 0


# ---------------------------------------------------------------- 4. large ids, isolated vertices ----------------------
@pytest.mark.parametrize("min_class", [0, 3])
def test_large_ids_and_isolated_vertices(ctx, min_class):
    rp, ci, n, initial, hubs, mode, exp, classes = _stars(200_000, True)
    alone = np.flatnonzero(np.diff(rp) == 0)
    alone = alone[alone > hubs.max() + 4097]                                  # behind the last star: nobody's neighbour
    assert n == 200_000 and alone.size > 90_000 and np.unique(initial[alone]).size > 50_000 and mode.max() > n - 100
    A = ctx.upload(rp, ci, n)
    ctx.set_option("lp_min_class", min_class)
    try:
        for max_iter in (1, 2):                                               # the result in the workspace array, and in P's own
            e = exp if max_iter == 1 else cdlp_ref.label_propagation(rp, ci, n, 2, initial)
            labels, info = _check(ctx, A, e, max_iter, initial, what="padded stars")
            assert np.array_equal(labels[alone], initial[alone])              # a caller's label on an isolated vertex stays
            assert info["class_vertices"] == classes[min_class]
        assert np.array_equal(exp[0][hubs], mode)
    finally:
        ctx.set_option("lp_min_class", 0)
        A.free()


# ---------------------------------------------------------------- 6. where the operand comes from ----------------------
def test_operand_provenance(ctx):
    """an upload, an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment, the transpose, a product
    turned operand, a select, an already symmetrized operand and the transposed (in-edge) storage: the same labels"""
    import torch
    name = "rmat12"
    rp, ci, n = _graph(name)
    handles = []

    def both(M, what):
        handles.append(M)
        for max_iter in (2, 3):
            _check(ctx, M, _expected(name, max_iter), max_iter, what=what)

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


def test_the_communities_through_transpose_and_products(ctx):
    name = "cliques64_66"
    rp, ci, n = _graph(name)
    e_labels, _, converged, _, communities = _expected(name, 10)
    assert communities == 3 and converged
    A = ctx.upload(rp, ci, n)
    P, info = ctx.label_propagation(A, 10)
    S = ctx.symmetrize(A, drop_diagonal=True)
    T = ctx.transpose(P)
    R1 = ctx.multiply(T, S)
    M1 = ctx.matrix_from_result(R1, n)
    R2 = ctx.multiply(M1, P)
    try:
        t_rp, t_ci = T.download()                                             # transpose(P): the members, ascending
        assert np.array_equal(np.diff(t_rp), np.bincount(e_labels, minlength=n))
        assert np.array_equal(t_ci, np.argsort(e_labels, kind="stable"))
        q_rp, q_ci = R2.download()                                            # P^T * S * P: the cliques do not touch
        rows = np.repeat(np.arange(n), np.diff(q_rp))
        assert q_ci.size == communities and np.array_equal(rows, q_ci)
    finally:
        for h in (R2, M1, R1, T, S, P, A):
            h.free()


def test_statistics_optional_outputs_and_repeatability(ctx):
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    out = C.c_void_p()
    try:
        before = ctx.stats()
        first = _check(ctx, A, _expected("rmat10", 3), 3, what="first")
        second = _check(ctx, A, _expected("rmat10", 3), 3, what="second")
        assert np.array_equal(first[0], second[0]) and first[1] == second[1]
        assert ctx.stats() == before and before["rows"] == n
        assert bspgemm.lib().bspgemm_label_propagation(ctx._h, A._h, None, 3, C.byref(out), None) == 0
        labels = np.zeros(n, np.int32)
        assert bspgemm.lib().bspgemm_matrix_download(ctx._h, out, None, labels.ctypes.data) == 0
        assert np.array_equal(labels, _expected("rmat10", 3)[0])
    finally:
        bspgemm.lib().bspgemm_matrix_free(out)
        R.free()
        A.free()


# ---------------------------------------------------------------- 7. errors --------------------------------------------
def test_errors_leave_no_result_and_a_usable_context(ctx):
    L = bspgemm.lib()
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                          # 10 x n
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)

    def call(a, initial=None, max_iter=3):
        out, info = C.c_void_p(0x5A5A), bspgemm.LpInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = L.bspgemm_label_propagation(ctx._h, a._h, initial.ctypes.data if initial is not None else None, max_iter,
                                         C.byref(out), C.byref(info))
        return st, out.value, L.bspgemm_last_error().decode(), bytes(info) == bytes(C.sizeof(info))

    try:
        st, out, msg, zeroed = call(rect)
        assert st == ERR_INVALID and not out and NAME in msg and "square" in msg and zeroed, msg
        st, out, msg, zeroed = call(foreign)
        assert st == ERR_INVALID and not out and NAME in msg and "context" in msg and zeroed, msg
        st, out, msg, zeroed = call(A, max_iter=-1)
        assert st == ERR_INVALID and not out and NAME in msg and "max_iter" in msg and zeroed, msg
        for at, value in ((0, n), (0, -1), (n - 1, n), (n - 1, 2**31 - 1), (n // 2, -2**31)):   # refused by index, on the host
            initial = np.arange(n, dtype=np.int32)
            initial[at] = value
            st, out, msg, zeroed = call(A, initial)
            assert st == ERR_INVALID and not out and NAME in msg and "initial_labels[%d]" % at in msg and zeroed, msg
        with pytest.raises(ValueError):
            ctx.label_propagation(A, 3, np.zeros(n - 1, np.int32))
        # the context still multiplies correctly, and still propagates
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        _check(ctx, A, _expected("rmat10", 3), 3, what="after the errors")
    finally:
        foreign.free()
        other.close()
        rect.free()
        A.free()


# ---------------------------------------------------------------- 8. max_iter == 0 --------------------------------------
def test_no_iteration(ctx):
    rng = np.random.default_rng(5462)
    for name in ("rmat10", "empty4", "star_hub_last"):
        rp, ci, n = _graph(name)
        A = ctx.upload(rp, ci, n)
        try:
            for initial in (None, rng.integers(0, n, size=n).astype(np.int32)):
                exp = cdlp_ref.label_propagation(rp, ci, n, 0, initial)
                first = np.arange(n) if initial is None else initial
                assert np.array_equal(exp[0], first) and exp[1:4] == (0, int(name == "empty4"), 0)
                labels, info = _check(ctx, A, exp, 0, initial, what=name)
                assert info["communities"] == np.unique(first).size
        finally:
            A.free()


# ---------------------------------------------------------------- 9. a seeded random campaign ---------------------------
def _campaign_case(i):
    rng = np.random.default_rng(5470 + i)
    kind = ("rmat", "powerlaw", "uniform", "dups_unsorted")[i % 4]
    if kind == "rmat":
        rp, ci, n = gen.rmat(int(rng.integers(6, 13)), int(rng.integers(2, 12)), SKEW, 5500 + i)
    elif kind == "powerlaw":
        rp, ci, n = gen.powerlaw(int(rng.integers(100, 5001)), int(rng.integers(2, 6)), 5500 + i)
    elif kind == "uniform":
        rp, ci, n = gen.uniform(int(rng.integers(50, 5001)), int(rng.integers(1, 10)), 5500 + i)
    else:
        rp, ci, n = gen.dups_unsorted(int(rng.integers(50, 5001)), int(rng.integers(1, 8)), 5500 + i)
    max_iter = int(rng.integers(0, 7))
    initial = rng.integers(0, n, size=n).astype(np.int32) if i % 2 else None   # half of the cases
    return kind, rp, ci, n, max_iter, initial, int(rng.integers(0, 4))


@pytest.mark.parametrize("i", range(20))
def test_random_campaign(ctx, i):
    kind, rp, ci, n, max_iter, initial, min_class = _campaign_case(i)
    assert n <= 5000 and max_iter <= 6
    exp = cdlp_ref.label_propagation(rp, ci, n, max_iter, initial)
    A = ctx.upload(rp, ci, n)
    ctx.set_option("lp_min_class", min_class)
    try:
        _, info = _check(ctx, A, exp, max_iter, initial, what="case %d: %s n %d max_iter %d LP_MIN_CLASS %d" % (i, kind, n, max_iter, min_class))
        assert info["class_vertices"] == cdlp_ref.class_vertices(rp, ci, n, min_class)
    finally:
        ctx.set_option("lp_min_class", 0)
        A.free()
