"""bspgemm_pagerank on the GPU against the numpy model of its definition (pagerank_ref.py): the fixed-point ranks, the doubles'
bytes and every counter are EQUAL to the model's under PULL and PUSH, for every iteration count and damping of the issue, at
every in-degree class boundary and under every PR_MIN_CLASS, for every form of the operands, with and without a tolerance,
with every output NULL, twice in a row and after other calls; the multiply statistics stay what they were; every refused
argument leaves a usable context.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
import pagerank_ref as P

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
METHODS = (P.PR_PULL, P.PR_PUSH)


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _check(got, exp, method, what):
    fixed, rank, info = got
    assert fixed.dtype == np.uint64 and np.array_equal(fixed, exp["fixed"]), what
    assert rank.tobytes() == exp["rank"].tobytes(), what
    for k in ("mass", "delta", "dangling", "iterations", "converged"):
        assert info[k] == exp[k], (what, k, info[k], exp[k])
    assert info["method"] == (P.PR_PUSH if method == P.PR_PUSH else P.PR_PULL), what
    return fixed.tobytes()


def _operands(ctx, name):
    rp, ci, n = P.graph(name)
    A = ctx.upload(rp, ci, n)
    t_rp, t_ci, _ = P.transposed(rp, ci, n)
    return A, ctx.upload(t_rp, t_ci, n)


@pytest.mark.parametrize("name", sorted(P.GRAPHS))
def test_equals_the_model(ctx, name):
    """every method x max_iter x damping of the issue; AT given"""
    rp, ci, n = P.graph(name)
    A, AT = _operands(ctx, name)
    try:
        for damping in P.DAMPINGS:
            rs, deltas, _ = P.cached_trajectory(name, damping)
            for it in P.ITERATIONS:
                exp = P.result(rs, deltas, False, rp, ci, n, at=it)
                for method in METHODS:
                    what = "%s, method %d, %d iterations, damping %r" % (name, method, it, damping)
                    _, _, info = got = ctx.pagerank(A, AT, method, damping, it)
                    _check(got, exp, method, what)
                    assert info["transposed"] == 0, what
                    assert info["canonicalised"] == (0 if P.is_canonical(rp, ci, n) else 1), what
    finally:
        AT.free()
        A.free()


@pytest.mark.parametrize("name", ["sink_star_8", "sink_star_256", "sink_star_4096", "hub_chunks", "rmat11", "all_dangling",
                                  "n_4097", "empty1"])
def test_every_min_class_gives_the_same_bits(ctx, name):
    rp, ci, n = P.graph(name)
    A, AT = _operands(ctx, name)
    exp = P.result(*P.cached_trajectory(name, 0.85)[:2], False, rp, ci, n, at=20)
    try:
        for min_class in (0, 1, 2, 3):
            ctx.set_option("pr_min_class", min_class)
            for at in (AT, None):
                _, _, info = got = ctx.pagerank(A, at, P.PR_PULL, 0.85, 20)
                _check(got, exp, P.PR_PULL, (name, min_class))
                assert info["class_vertices"] == P.class_vertices(rp, ci, n, min_class), (name, min_class, info)
            if min_class == 3:
                assert info["class_vertices"] == [0, 0, 0, n]
            _, _, info = got = ctx.pagerank(A, AT, P.PR_PUSH, 0.85, 20)      # PUSH has no classes
            _check(got, exp, P.PR_PUSH, (name, min_class, "push"))
            assert info["class_vertices"] == [0, 0, 0, 0]
    finally:
        ctx.set_option("pr_min_class", 0)
        AT.free()
        A.free()
    with pytest.raises(bspgemm.BspgemmError):
        ctx.set_option("pr_min_class", 4)
    assert ctx.get_option("pr_min_class") == 0


def test_operands_in_every_form(ctx):
    import torch
    name = "rmat11"
    rp, ci, n = P.graph(name)
    assert P.is_canonical(rp, ci, n)
    exp = P.result(*P.cached_trajectory(name, 0.85)[:2], False, rp, ci, n, at=20)
    A, AT = _operands(ctx, name)
    T = ctx.transpose(A)
    I = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(I, A)
    M = ctx.matrix_from_result(R, n)
    R.free()
    # an unsorted AT with repeats, built by hand on the device: the rows of the transpose reversed, the first entry twice
    t_rp, t_ci, _ = P.transposed(rp, ci, n)
    rows = [t_ci[t_rp[v]:t_rp[v + 1]][::-1] for v in range(n)]
    rows = [np.concatenate([r, r[:1]]) for r in rows]
    u_rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    u_ci = np.concatenate(rows).astype(np.int32)
    d_rp, d_ci = torch.from_numpy(u_rp).cuda(), torch.from_numpy(u_ci).cuda()
    torch.cuda.synchronize()
    W = ctx.wrap_device(n, n, u_ci.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci))
    U = ctx.upload(u_rp, u_ci, n)
    # another graph's transpose: memory safety only
    o_rp, o_ci, _ = P.transposed(*gen.uniform(n, 9, 5801))
    wrong = ctx.upload(o_rp, o_ci, n)
    try:
        seen = set()
        for what, a, at, transposed, canon in (("AT given", A, AT, 0, 0), ("AT NULL", A, None, 1, 0),
                                               ("AT from transpose", A, T, 0, 0), ("A from a result", M, AT, 0, 0),
                                               ("A from a result, AT NULL", M, None, 1, 0),
                                               ("unsorted AT, wrapped", A, W, 0, 2), ("unsorted AT, uploaded", A, U, 0, 2)):
            _, _, info = got = ctx.pagerank(A=a, AT=at, method=P.PR_PULL)
            seen.add(_check(got, exp, P.PR_PULL, what))
            assert (info["transposed"], info["canonicalised"]) == (transposed, canon), (what, info)
        for a in (A, M):
            seen.add(_check(ctx.pagerank(a, None, P.PR_PUSH), exp, P.PR_PUSH, "push"))
            seen.add(_check(ctx.pagerank(a, None, P.PR_AUTO), exp, P.PR_AUTO, "auto"))
        assert len(seen) == 1
        fixed, rank, info = ctx.pagerank(A, wrong, P.PR_PULL)              # some result, memory-safely
        assert info["iterations"] == 20 and info["mass"] == int(fixed.sum(dtype=np.uint64))   # (modulo 2^64: mass is not kept)
        _check(ctx.pagerank(A, AT, P.PR_PULL), exp, P.PR_PULL, "after a wrong AT")
    finally:
        for h in (wrong, U, W, M, I, T, AT, A):
            h.free()


def test_symmetric_operand_as_its_own_transpose(ctx):
    rp, ci, n = P.graph("symmetric_rmat9")
    exp = P.result(*P.cached_trajectory("symmetric_rmat9", 0.85)[:2], False, rp, ci, n, at=20)
    A = ctx.upload(rp, ci, n)
    try:
        _, _, info = got = ctx.pagerank(A, A, P.PR_PULL)
        _check(got, exp, P.PR_PULL, "AT == A")
        assert info["transposed"] == 0 and info["canonicalised"] == 0
    finally:
        A.free()


@pytest.mark.parametrize("name", ["dups_unsorted", "untidy"])
def test_non_canonical_operand_is_brought_to_form(ctx, name):
    rp, ci, n = P.graph(name)
    exp = P.result(*P.cached_trajectory(name, 0.85)[:2], False, rp, ci, n, at=20)
    A = ctx.upload(rp, ci, n)
    try:
        for method, at_null_transposed in ((P.PR_PULL, 1), (P.PR_PUSH, 0)):
            _, _, info = got = ctx.pagerank(A, None, method)
            _check(got, exp, method, name)
            assert info["canonicalised"] == 1 and info["transposed"] == at_null_transposed, info
        fixed, _, info = ctx.pagerank(A, A, P.PR_PULL)                     # the one untidy handle as both: some result
        assert info["canonicalised"] == 3 and info["mass"] == int(fixed.sum(dtype=np.uint64))
    finally:
        A.free()


def test_tolerance(ctx):
    name = "rmat11"
    rp, ci, n = P.graph(name)
    A, AT = _operands(ctx, name)
    try:
        for tolerance in (1e-6, 1e-12):
            rs, deltas, conv = P.trajectory(rp, ci, n, 0.85, 200, tolerance)
            exp = P.result(rs, deltas, conv, rp, ci, n)
            assert conv and 3 < exp["iterations"] < 200 and exp["delta"] <= P.threshold(tolerance) < deltas[-2]
            for method in METHODS:
                _check(ctx.pagerank(A, AT, method, 0.85, 200, tolerance), exp, method, (tolerance, method))
            # max_iter ends it first
            cut = P.result(rs, deltas, False, rp, ci, n, at=3)
            _check(ctx.pagerank(A, AT, P.PR_PULL, 0.85, 3, tolerance), cut, P.PR_PULL, (tolerance, "cut"))
        rs, deltas, conv = P.trajectory(rp, ci, n, 0.85, 50)
        for method in METHODS:
            _, _, info = got = ctx.pagerank(A, AT, method, 0.85, 50, 0.0)
            _check(got, P.result(rs, deltas, conv, rp, ci, n), method, "50 iterations")
            assert info["iterations"] == 50 and info["converged"] == 0
        # a tolerance beyond every possible delta ends the loop after one iteration
        exp = P.result(*P.trajectory(rp, ci, n, 0.85, 9, 10.0), rp, ci, n)
        assert exp["iterations"] == 1 and exp["converged"] == 1
        _check(ctx.pagerank(A, AT, P.PR_PUSH, 0.85, 9, 10.0), exp, P.PR_PUSH, "tolerance 10")
    finally:
        AT.free()
        A.free()


def test_null_outputs(ctx):
    L = bspgemm.lib()
    name = "sink_star_256"
    rp, ci, n = P.graph(name)
    exp = P.result(*P.cached_trajectory(name, 0.85)[:2], False, rp, ci, n, at=20)
    A, AT = _operands(ctx, name)
    try:
        for method in METHODS:
            for want_fixed, want_rank, want_info in ((1, 0, 1), (0, 1, 1), (0, 0, 1), (1, 1, 0), (0, 0, 0)):
                fixed, rank, info = np.zeros(n, np.uint64), np.zeros(n, np.float64), bspgemm.PrInfo()
                st = L.bspgemm_pagerank(ctx._h, A._h, AT._h, method, 0.85, 20, 0.0, fixed.ctypes.data if want_fixed else None,
                                        rank.ctypes.data if want_rank else None, C.byref(info) if want_info else None)
                assert st == 0, L.bspgemm_last_error()
                if want_fixed:
                    assert np.array_equal(fixed, exp["fixed"])
                if want_rank:
                    assert rank.tobytes() == exp["rank"].tobytes()
                if want_info:
                    assert info.mass == exp["mass"] and info.delta == exp["delta"] and info.iterations == 20
    finally:
        AT.free()
        A.free()


def test_workspace_reuse(ctx):
    """two calls in a row, and a call after another graph call and a larger PageRank"""
    rp, ci, n = P.graph("rmat11")
    exp = P.result(*P.cached_trajectory("rmat11", 0.85)[:2], False, rp, ci, n, at=20)
    A = ctx.upload(rp, ci, n)
    big = ctx.upload(*P.graph("hub_chunks"))
    try:
        for method in METHODS:
            first = _check(ctx.pagerank(A, None, method), exp, method, "first")
            assert _check(ctx.pagerank(A, None, method), exp, method, "second") == first
            ctx.pagerank(big, None, method, max_iter=2)
            ctx.connected_components(A)[0].free()
            m, _ = ctx.label_propagation(A, 3)
            m.free()
            assert _check(ctx.pagerank(A, None, method), exp, method, "after other calls") == first
    finally:
        big.free()
        A.free()


def test_multiply_statistics_are_untouched(ctx):
    rp, ci, n = P.graph("rmat11")
    exp = P.result(*P.cached_trajectory("rmat11", 0.85)[:2], False, rp, ci, n, at=20)
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    try:
        before = ctx.stats()
        for method in METHODS:
            _check(ctx.pagerank(A, None, method), exp, method, "stats")
        assert ctx.stats() == before and before["rows"] == n
    finally:
        R.free()
        A.free()


def test_errors_leave_a_usable_context(ctx):
    import torch
    L = bspgemm.lib()
    name = "rmat11"
    rp, ci, n = P.graph(name)
    exp = P.result(*P.cached_trajectory(name, 0.85)[:2], False, rp, ci, n, at=20)
    A, AT = _operands(ctx, name)
    t_rp, t_ci, _ = P.transposed(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                              # 10 x n
    small = ctx.upload(np.zeros(n, np.int32), np.zeros(0, np.int32), n - 1)  # (n - 1) x (n - 1)
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)
    bad = []
    for base_rp, base_ci, at, col in ((rp, ci, ci.size // 2, n), (rp, ci, ci.size - 1, -1), (t_rp, t_ci, t_ci.size // 3, n)):
        c = base_ci.copy()
        c[at] = col
        d_rp, d_ci = torch.from_numpy(base_rp.copy()).cuda(), torch.from_numpy(c).cuda()
        bad.append(ctx.wrap_device(n, n, c.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci)))
    torch.cuda.synchronize()
    bad_a, bad_at = bad[:2], bad[2:]

    def call(a, at, method, context=ctx):
        info = bspgemm.PrInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        fixed = np.zeros(n, np.uint64)
        st = L.bspgemm_pagerank(context._h, a._h, at._h if at is not None else None, method, 0.85, 20, 0.0, fixed.ctypes.data,
                                None, C.byref(info))
        msg = L.bspgemm_last_error().decode()
        assert st != 0 and bytes(info) == bytes(C.sizeof(info)) and "bspgemm_pagerank" in msg, (st, msg)
        return st, msg

    def good(what):
        for method in METHODS:
            _check(ctx.pagerank(A, AT, method), exp, method, what)

    try:
        for method in (0, 1, 2):
            st, msg = call(rect, None, method)
            assert st == ERR_INVALID and "square" in msg, msg
            st, msg = call(foreign, None, method)
            assert st == ERR_INVALID and "context" in msg, msg
            for W in bad_a:
                for at in (None, AT):
                    st, msg = call(W, at, method)
                    assert st == ERR_INVALID and "column" in msg and "operand A" in msg, msg
                good("after a bad column of A")
        for method in (0, 1):                                                # (under PUSH, AT is ignored)
            for W in (small, rect):
                st, msg = call(A, W, method)
                assert st == ERR_INVALID and "AT is" in msg, msg
            st, msg = call(A, foreign, method)
            assert st == ERR_INVALID and "context" in msg, msg
            for W in bad_at:
                st, msg = call(A, W, method)
                assert st == ERR_INVALID and "column" in msg and "operand AT" in msg, msg
            good("after a bad column of AT")
        for W in bad_at + [small, rect, foreign]:
            _check(ctx.pagerank(A, W, P.PR_PUSH), exp, P.PR_PUSH, "PUSH ignores AT")
        R = ctx.multiply(A, A)                                              # the context still multiplies correctly
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        good("after the errors")
    finally:
        for h in bad:
            h.free()
        foreign.free()
        other.close()
        for h in (small, rect, AT, A):
            h.free()
