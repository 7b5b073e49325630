"""The single-source direction-optimising BFS (bspgemm_bfs_tree): row_ptr, parents and levels against the numpy search of
bfs_tree_ref.py, bit for bit, under PUSH, PULL and AUTO, with the info block against the host model of the direction rule.

What can go wrong is the frontier and the parent: the wave-aggregated append of more than a wave and one group walking a
long row (the stars), thousands of atomicMin on one address (the stars reversed), groups of unequal trip counts in one wave
(rows of W - 1, W, W + 1 entries under every lane count), two candidate parents and back edges (layered), the hand-over of
a lane's in-row to the wave in the pull kernel (in-rows around kBfsPullLight with the only frontier member first, last or
absent), reached sets that cross the read-out's flag words (vertex counts 257, 1023, 4099), many levels and the depth cap
(the path), and degenerate inputs -- each at the smallest size that still has the property.
"""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import bfs_tree_ref as ref
import bspgemm
import gen

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
DIRECTIONS = ("push", "pull", "auto")
INFO_KEYS = ("reached", "edges_pushed", "pull_mask", "depth", "complete", "push_levels", "pull_levels")


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _run(ctx, A, AT, source, direction, exp, what, max_depth=0):
    """one call compared with the expected (row_ptr, parents, levels); returns (downloaded bytes, info)"""
    e_rp, e_parent, e_level = exp
    R, info = ctx.bfs_tree(A, AT, source, direction, max_depth)
    try:
        assert (R.rows, R.nnz) == (e_rp.size - 1, e_parent.size), (what, R.rows, R.nnz)
        rp, parent = R.download()
        level = R.download_values()
        assert rp.dtype == np.int64 and np.array_equal(rp, e_rp), what
        assert parent.dtype == np.int32 and np.array_equal(parent, e_parent), what
        assert level.dtype == np.int32 and np.array_equal(level, e_level), what
        assert R.values_sum() == int(e_level.sum(dtype=np.int64)), what
        assert info["reached"] == e_parent.size, what
    finally:
        R.free()
    return rp.tobytes() + parent.tobytes() + level.tobytes(), info


def _model(name, direction, **kw):
    return ref.model(*ref.graph(name), direction=direction, **kw)


def _same(info, model, what):
    assert {k: info[k] for k in INFO_KEYS} == model, (what, info, model)


# ---------------------------------------------------------------- 1. every named graph, every direction ---------------
@pytest.mark.parametrize("name", list(ref.GRAPHS))
def test_tree_equals_the_reference_in_every_direction(ctx, name):
    rp, ci, n, source = ref.graph(name)
    exp = ref.expected(name)
    A = ctx.upload(rp, ci, n)
    AT = ctx.transpose(A)
    try:
        seen = set()
        for direction in DIRECTIONS:
            what = "%s, %s" % (name, direction)
            got, info = _run(ctx, A, AT, source, direction, exp, what)
            seen.add(got)
            _same(info, _model(name, direction), what)
            assert (info["transposed"], info["canonicalised"]) == (0, 0), what
        assert len(seen) == 1
        ref.tree_check(rp, ci, n, source, *exp)
    finally:
        AT.free()
        A.free()


@pytest.mark.parametrize("name", list(ref.GRAPHS))
def test_reached_set_and_levels_equal_bspgemm_bfs(ctx, name):
    rp, ci, n, source = ref.graph(name)
    A = ctx.upload(rp, ci, n)
    L, depth, complete = ctx.bfs(A, [source])
    R, info = ctx.bfs_tree(A, None, source, "auto")
    try:
        l_rp, l_ci = L.download()
        l_v = L.download_values()
        t_rp, _ = R.download()
        assert l_rp.tolist() == [0, l_ci.size]
        assert np.array_equal(np.flatnonzero(np.diff(t_rp)), l_ci)
        assert np.array_equal(R.download_values(), l_v)
        assert info["depth"] == depth and info["complete"] == 1 and complete
    finally:
        R.free()
        L.free()
        A.free()


# ---------------------------------------------------------------- 2. the knobs ----------------------------------------
@pytest.mark.parametrize("lanes", [4, 16, 64, 0])
def test_every_lane_count_of_the_push_kernel(ctx, lanes):
    default = ctx.get_option("bfs_push_lanes")
    assert default == 0
    try:
        ctx.set_option("bfs_push_lanes", lanes)
        assert ctx.get_option("bfs_push_lanes") == lanes
        for name in ("rows_around4", "rows_around16", "rows_around64", "star_out65", "star_out5000", "star_in5000", "layered",
                     "rmat12_directed"):
            rp, ci, n, source = ref.graph(name)
            A = ctx.upload(rp, ci, n)
            try:
                what = "%s, %d lanes" % (name, lanes)
                _, info = _run(ctx, A, None, source, "push", ref.expected(name), what)
                _same(info, _model(name, "push"), what)
            finally:
                A.free()
    finally:
        ctx.set_option("bfs_push_lanes", default)
    for bad in (-1, 1, 8, 32, 128):
        with pytest.raises(bspgemm.BspgemmError):
            ctx.set_option("bfs_push_lanes", bad)
    assert ctx.get_option("bfs_push_lanes") == default


@pytest.mark.parametrize("alpha,beta", [(15, 18), (1, 1), (2**20, 2**20)])
def test_direction_follows_the_host_model(ctx, alpha, beta):
    assert (ctx.get_option("bfs_alpha"), ctx.get_option("bfs_beta")) == (15, 18)
    try:
        ctx.set_option("bfs_alpha", alpha)
        ctx.set_option("bfs_beta", beta)
        for name in ("rmat12", "rmat12_directed", "powerlaw", "layered", "star_in5000", "path300"):
            rp, ci, n, source = ref.graph(name)
            A = ctx.upload(rp, ci, n)
            AT = ctx.transpose(A)
            try:
                what = "%s, alpha %d, beta %d" % (name, alpha, beta)
                _, info = _run(ctx, A, AT, source, "auto", ref.expected(name), what)
                model = _model(name, "auto", alpha=alpha, beta=beta)
                _same(info, model, what)
                if name == "rmat12" and (alpha, beta) == (15, 18):   # push, pull, ..., push: both switches were taken
                    kinds = [(info["pull_mask"] >> d) & 1 for d in range(info["push_levels"] + info["pull_levels"])]
                    assert kinds[0] == 0 and kinds[-1] == 0 and 1 in kinds, kinds
            finally:
                AT.free()
                A.free()
    finally:
        ctx.set_option("bfs_alpha", 15)
        ctx.set_option("bfs_beta", 18)
    for name in ("bfs_alpha", "bfs_beta"):
        with pytest.raises(bspgemm.BspgemmError):
            ctx.set_option(name, 0)


@pytest.mark.parametrize("max_depth,complete,depth", [(1, 0, 1), (150, 0, 150), (400, 1, 299)])
def test_depth_cap_on_the_path(ctx, max_depth, complete, depth):
    rp, ci, n, source = ref.graph("path300")
    exp = ref.expected("path300", max_depth)
    assert exp[1].size == depth + 1
    A = ctx.upload(rp, ci, n)
    AT = ctx.transpose(A)
    try:
        for direction in DIRECTIONS:
            _, info = _run(ctx, A, AT, source, direction, exp, direction, max_depth)
            _same(info, _model("path300", direction, max_depth=max_depth), direction)
            assert (info["complete"], info["depth"]) == (complete, depth)
    finally:
        AT.free()
        A.free()


# ---------------------------------------------------------------- 3. AT, provenance, repeatability --------------------
def _untidy_transpose(rp, ci, n, seed):
    """the transpose with every row shuffled and a fifth of the entries stored twice"""
    rng = np.random.default_rng(seed)
    T = csr_matrix((np.ones(ci.size, np.int8), ci.copy(), rp.copy()), shape=(n, n)).T.tocoo()
    r, c = T.row.astype(np.int64), T.col.astype(np.int64)
    again = rng.random(r.size) < 0.2
    r, c = np.concatenate([r, r[again]]), np.concatenate([c, c[again]])
    o = rng.permutation(r.size)
    r, c = r[o], c[o]
    o = np.argsort(r, kind="stable")
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return t_rp, c[o].astype(np.int32)


def test_every_form_of_AT_gives_the_same_tree(ctx):
    name = "rmat12_directed"
    rp, ci, n, source = ref.graph(name)
    exp = ref.expected(name)
    A = ctx.upload(rp, ci, n)
    AT = ctx.transpose(A)
    u_rp, u_ci = _untidy_transpose(rp, ci, n, 5530)
    assert u_ci.size > AT.nnz and (np.diff(u_ci) < 0).sum() > n          # repeats, and rows out of order
    U = ctx.upload(u_rp, u_ci, n)
    try:
        seen = set()
        for direction in DIRECTIONS:
            pulls = _model(name, direction)["pull_levels"]
            assert pulls > 0 or direction == "push"
            for what, at, transposed, canonicalised in (("NULL", None, int(pulls > 0), 0), ("transpose", AT, 0, 0),
                                                        ("untidy", U, 0, int(direction != "push"))):
                got, info = _run(ctx, A, at, source, direction, exp, "%s, AT %s" % (direction, what))
                seen.add(got)
                _same(info, _model(name, direction), (direction, what))
                assert (info["transposed"], info["canonicalised"]) == (transposed, canonicalised), (direction, what, info)
        assert len(seen) == 1
    finally:
        U.free()
        AT.free()
        A.free()
    # a symmetric canonical A is its own transpose: the same handle
    rp, ci, n, source = ref.graph("rmat12")
    S = ctx.upload(rp, ci, n)
    try:
        for direction in DIRECTIONS:
            _, info = _run(ctx, S, S, source, direction, ref.expected("rmat12"), "A as AT, " + direction)
            _same(info, _model("rmat12", direction), direction)
            assert (info["transposed"], info["canonicalised"]) == (0, 0)
    finally:
        S.free()


def test_operand_provenance(ctx):
    """an upload, an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment, the transpose of the
    symmetric graph, a product turned operand, a select and a symmetrized operand: the same tree"""
    import torch
    name = "rmat12"
    rp, ci, n, source = ref.graph(name)
    exp = ref.expected(name)
    A = ctx.upload(rp, ci, n)
    extra = gen.uniform_rect(37, n, 3, 5450)
    tall_rp = np.concatenate([extra[0], extra[0][-1] + rp[1:]]).astype(np.int32)
    tall_ci = np.concatenate([extra[1], ci]).astype(np.int32)
    I = ctx.upload(tall_rp, tall_ci, n, row0=37, rows=n)
    trp = torch.from_numpy(rp.copy()).cuda()
    buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + ci.size] = torch.from_numpy(ci.copy()).cuda()
    torch.cuda.synchronize()
    tci = buf[1:]
    assert tci.data_ptr() % 16 == 4
    W = ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf))
    T = ctx.transpose(A)
    U = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(U, A)
    M = ctx.matrix_from_result(R, n)
    R.free()
    S = ctx.select(A, "offdiag")
    Y = ctx.symmetrize(A, drop_diagonal=True)
    try:
        seen = set()
        for what, X in (("upload", A), ("interior upload", I), ("wrapped, col_idx 4 bytes off alignment", W), ("transpose", T),
                        ("matrix_from_result", M), ("select", S), ("symmetrized", Y)):
            for direction in DIRECTIONS:
                seen.add(_run(ctx, X, X, source, direction, exp, "%s, %s" % (what, direction))[0])
            seen.add(_run(ctx, X, None, source, "auto", exp, what + ", AT NULL")[0])
        assert len(seen) == 1
    finally:
        for h in (A, I, W, T, U, M, S, Y):
            h.free()


def test_two_calls_give_identical_bytes(ctx):
    name = "powerlaw"
    rp, ci, n, source = ref.graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for direction in DIRECTIONS:
            first = _run(ctx, A, None, source, direction, ref.expected(name), "first")
            second = _run(ctx, A, None, source, direction, ref.expected(name), "second")
            assert first == second
    finally:
        A.free()


def test_composition_with_the_result_functions(ctx):
    """the tree as a child -> parent operand, its transpose the children lists, and the vertices of one level"""
    name = "layered"
    rp, ci, n, source = ref.graph(name)
    level, parent, _, _ = ref.search(rp, ci, n, source)
    A = ctx.upload(rp, ci, n)
    R, info = ctx.bfs_tree(A, None, source)
    try:
        up = ctx.matrix_from_result(R, n)
        down = ctx.transpose(up)
        d_rp, d_ci = down.download()
        reached = np.flatnonzero(level >= 0)
        order = np.lexsort((reached, parent[reached]))
        assert np.array_equal(d_ci, reached[order]) and np.array_equal(np.diff(d_rp), np.bincount(parent[reached], minlength=n))
        for d in (0, 3, info["depth"], info["depth"] + 1):
            D = ctx.matrix_from_result_where(R, n, "==", d)
            q_rp, q_ci = D.download()
            D.free()
            assert np.array_equal(np.flatnonzero(np.diff(q_rp)), np.flatnonzero(level == d)), d
            assert np.array_equal(q_ci, parent[level == d]), d
        down.free()
        up.free()
    finally:
        R.free()
        A.free()


def test_multiply_statistics_are_untouched(ctx):
    rp, ci, n, source = ref.graph("rmat12_directed")
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    try:
        before = ctx.stats()
        for direction in DIRECTIONS:
            _run(ctx, A, None, source, direction, ref.expected("rmat12_directed"), "stats")
        assert ctx.stats() == before and before["rows"] == n
    finally:
        R.free()
        A.free()


# ---------------------------------------------------------------- 4. errors --------------------------------------------
def test_errors_leave_no_result_and_a_usable_context(ctx):
    import torch
    L = bspgemm.lib()
    name = "rmat12_directed"
    rp, ci, n, source = ref.graph(name)
    exp = ref.expected(name)
    level = ref.search(rp, ci, n, source)[0]
    A = ctx.upload(rp, ci, n)
    AT = ctx.transpose(A)
    t_rp, t_ci = AT.download()
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                          # 10 x n
    small = ctx.upload(np.zeros(n, np.int32), np.zeros(0, np.int32), n - 1)   # (n - 1) x (n - 1)
    none = ctx.upload(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)   # n == 0
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)
    # one bad column each, on a row that the search walks: checked on the device before it indexes
    rows = np.repeat(np.arange(n), np.diff(rp))
    walked = np.flatnonzero(level[rows] >= 0)
    keep, bad_a, bad_at = [], [], []
    for at, col in ((int(walked[walked.size // 2]), n), (int(walked[-1]), -1), (int(walked[0]), 2**31 - 1)):
        c = ci.copy()
        c[at] = col
        d_rp, d_ci = torch.from_numpy(rp.copy()).cuda(), torch.from_numpy(c).cuda()
        keep.append((d_rp, d_ci))
        bad_a.append(ctx.wrap_device(n, n, c.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci)))
    for at, col in ((t_ci.size // 2, n), (0, -1)):
        c = t_ci.copy()
        c[at] = col
        d_rp, d_ci = torch.from_numpy(t_rp.copy()).cuda(), torch.from_numpy(c).cuda()
        keep.append((d_rp, d_ci))
        bad_at.append(ctx.wrap_device(n, n, c.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci)))
    torch.cuda.synchronize()

    def call(a, at, src=source, direction=0, context=ctx):
        out, info = C.c_void_p(0x5A5A), bspgemm.BfsTreeInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = L.bspgemm_bfs_tree(context._h, a._h, at._h if at is not None else None, src, direction, 0, C.byref(out),
                                C.byref(info))
        msg = L.bspgemm_last_error().decode()
        assert st != 0 and not out.value and bytes(info) == bytes(C.sizeof(info)), (st, msg)
        assert "bspgemm_bfs_tree" in msg, msg
        return st, msg

    try:
        for direction in (0, 1, 2):
            st, msg = call(rect, None, direction=direction)
            assert st == ERR_INVALID and "square" in msg, msg
            st, msg = call(foreign, None, direction=direction)
            assert st == ERR_INVALID and "context" in msg, msg
            for src in (-1, n, 2**31 - 1):
                st, msg = call(A, AT, src=src, direction=direction)
                assert st == ERR_INVALID and "source" in msg, msg
            st, msg = call(none, None, src=0, direction=direction)
            assert st == ERR_INVALID and "source" in msg, msg
            for W in bad_a:
                for at in (None, AT):
                    st, msg = call(W, at, direction=direction)
                    assert st == ERR_INVALID and "column" in msg, msg
                    _run(ctx, A, AT, source, {0: "auto", 1: "push", 2: "pull"}[direction], exp, "after a bad column of A")   # exact at once
        for direction in (0, 2):                             # (under PUSH, AT is ignored)
            st, msg = call(A, small, direction=direction)
            assert st == ERR_INVALID and "AT is" in msg, msg
            st, msg = call(A, rect, direction=direction)
            assert st == ERR_INVALID and "AT is" in msg, msg
            st, msg = call(A, foreign, direction=direction)
            assert st == ERR_INVALID and "context" in msg, msg
            for W in bad_at:
                st, msg = call(A, W, direction=direction)
                assert st == ERR_INVALID and "column" in msg and "AT" in msg, msg
        for W in bad_at + [small, rect, foreign]:
            _run(ctx, A, W, source, "push", exp, "PUSH ignores AT")
        for direction in (-1, 3, 7):
            st, msg = call(A, AT, direction=direction)
            assert st == ERR_INVALID and "direction" in msg, msg
        # the context still multiplies correctly, and still searches
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        for direction in DIRECTIONS:
            _run(ctx, A, AT, source, direction, exp, "after the errors")
    finally:
        for h in bad_a + bad_at:
            h.free()
        foreign.free()
        other.close()
        for h in (none, small, rect, AT, A):
            h.free()
