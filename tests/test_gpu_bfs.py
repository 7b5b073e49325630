"""The device-resident multi-source BFS (bspgemm_bfs): pattern, levels, depth and completion against scipy's shortest
paths (bfs_ref.py), bit for bit.

What can go wrong is the merge of the visited set with each new frontier: it works in tiles of 4096 entries, four per
lane, whatever rows they belong to, searches every entry in the other operand's row and places it without a scan.  So the
shapes put many tiles on both sides of one merge, rows that are empty on one side, row and tile boundaries everywhere
(|V| crossing 64, 4096 and 4097 entries from one level to the next), and sizes that are no multiple of four.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bfs_ref
import bspgemm
import gen

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
SKEW = (0.57, 0.19, 0.19, 0.05)
LAYERS = [1, 62, 1, 1, 4030, 1, 1, 3, 4095]          # |V| = 1, 63, 64, 65, 4095, 4096, 4097, 4100, 8195 level by level


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(rp, ci, n) of the named graph; computed once"""
    if name == "rmat12":
        return gen.rmat(12, 8, SKEW, 5401)
    if name == "powerlaw":
        return gen.powerlaw(6000, 3, 5402)
    if name == "rmat10":
        return gen.rmat(10, 6, SKEW, 5403)
    if name == "uniform300":
        return gen.uniform(300, 2, 5404)
    if name == "layered":
        return bfs_ref.layered(LAYERS, 2, 11)[:3]
    return {"path": bfs_ref.path, "cycle": bfs_ref.cycle, "star": bfs_ref.star}[name](200)


@functools.lru_cache(maxsize=None)
def _dist(name, sources):
    rp, ci, n = _graph(name)
    d = bfs_ref.distances(rp, ci, n, list(sources))
    d.setflags(write=False)
    return d


def _sources(name, count):
    n = _graph(name)[2]
    return tuple(int(x) for x in np.random.default_rng(9).choice(n, size=count, replace=False))


def _expected(name, sources, max_depth=0):
    """((row_ptr, col_idx, values), depth, complete) from the shared reference distances"""
    dist = _dist(name, tuple(sources))
    full_depth = int(dist.max())
    csr = bfs_ref.levels_csr(dist, max_depth)
    complete = 1 if max_depth <= 0 or max_depth > full_depth else int(csr[1].size == dist.size)
    return csr, int(csr[2].max()), complete


def _download(R):
    rp, ci = R.download()
    return rp, ci, R.download_values()


def _check(ctx, A, sources, exp, max_depth=0, what=""):
    """run the search and compare everything; returns the downloaded result"""
    (e_rp, e_ci, e_v), e_depth, e_complete = exp
    R, depth, complete = ctx.bfs(A, sources, max_depth)
    try:
        got = _download(R)
        assert R.rows == len(sources) and R.nnz == e_ci.size, what
        assert got[0].dtype == np.int64 and np.array_equal(got[0], e_rp), what
        assert np.array_equal(got[1], e_ci), what
        assert got[2].dtype == np.int32 and np.array_equal(got[2], e_v), what
        assert (depth, int(complete)) == (e_depth, e_complete), what
        at_source = np.array([got[2][got[0][s] + np.searchsorted(got[1][got[0][s]:got[0][s + 1]], src)]
                              for s, src in enumerate(sources)])
        assert (at_source == 0).all(), what
        assert R.values_sum() == int(e_v.astype(np.int64).sum()), what
    finally:
        R.free()
    return got


def _run_named(ctx, name, sources, max_depth=0):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        return _check(ctx, A, list(sources), _expected(name, sources, max_depth), max_depth, name)
    finally:
        A.free()


# ---------------------------------------------------------------- 1. the inputs of the host-loop test ------------------
@pytest.mark.parametrize("name,depth", [("rmat12", 5), ("powerlaw", 9)])
def test_existing_inputs_eight_sources(ctx, name, depth):
    sources = _sources(name, 8)
    rp, ci, n = _graph(name)
    if name == "rmat12":          # a one-entry row of V against an empty row of N
        assert int((np.diff(rp)[list(sources)] == 0).sum()) == 5
    exp = _expected(name, sources)
    assert exp[1:] == (depth, 1)
    _run_named(ctx, name, sources)


# ---------------------------------------------------------------- 2. many tiles on both sides --------------------------
@pytest.mark.parametrize("name", ["rmat12", "powerlaw"])
def test_sixty_four_sources_many_tiles(ctx, name):
    sources = _sources(name, 64)
    rp, ci, n = _graph(name)
    dist = _dist(name, sources)
    sizes = bfs_ref.frontier_sizes(dist)
    if name == "rmat12":
        assert sizes == [64, 396, 18647, 56603, 19787, 1073, 23] and sum(sizes) == 96593
        assert int((np.diff(rp)[list(sources)] == 0).sum()) == 26
        assert int(np.diff(rp).max()) == 641 and int((np.diff(rp) == 0).sum()) == 1555
    else:
        assert len(sizes) - 1 == 12 and sum(sizes) == 143595
    before = np.cumsum(sizes)[:-1]                     # |V| when level d is merged in, |N| = sizes[d]
    assert any(v >= 3 * bfs_ref.K_SEL_TILE and m >= 3 * bfs_ref.K_SEL_TILE for v, m in zip(before, sizes[1:]))
    _run_named(ctx, name, sources)


# ---------------------------------------------------------------- 3. tile, word and alignment edges -------------------
@pytest.mark.parametrize("name", ["path", "cycle", "star"])
def test_path_cycle_star(ctx, name):
    sources = (0, 199, 100, 1)
    exp = _expected(name, sources)
    assert exp[1:] == ({"path": 199, "cycle": 199, "star": 1}[name], 1)
    _run_named(ctx, name, sources)


def test_complete_digraph_ends_by_the_full_set(ctx):
    rp, ci, n = bfs_ref.complete(65)
    sources = np.arange(n)
    A = ctx.upload(rp, ci, n)
    try:
        exp = bfs_ref.bfs_ref(rp, ci, n, sources)
        assert exp[0][1].size == n * n and exp[1:] == (1, 1)
        _check(ctx, A, sources, exp, what="complete 65")
        # the cap at the depth: the set is full, so the search still ended by itself
        _check(ctx, A, sources, bfs_ref.bfs_ref(rp, ci, n, sources, 1), 1, "complete 65 capped")
        assert ctx.stats()["rows"] == n
        # one product ran, and none after the visited set was full
        R, depth, complete = ctx.bfs(A, sources[:3])
        assert (R.nnz, depth, complete) == (3 * n, 1, True)
        R.free()
    finally:
        A.free()


def test_visited_set_crosses_64_4096_4097(ctx):
    rp, ci, n, ids = bfs_ref.layered(LAYERS, 2, 11)
    assert n % 4 == 1
    lost = int(np.setdiff1d(np.arange(n), np.concatenate(ids))[0])
    one = (int(ids[0][0]),)
    assert np.cumsum(bfs_ref.frontier_sizes(_dist("layered", one))).tolist() == [1, 63, 64, 65, 4095, 4096, 4097, 4100, 8195]
    _run_named(ctx, "layered", one)
    # rows of very different lengths: tiles that start and end inside rows, a row that stays short, a repeated source
    several = (int(ids[0][0]), int(ids[4][7]), lost, int(ids[8][0]), int(ids[0][0]), int(ids[2][0]))
    _run_named(ctx, "layered", several)


# ---------------------------------------------------------------- 4. arguments and composition ------------------------
def test_repeated_sources_give_equal_rows(ctx):
    sources = _sources("rmat10", 3)
    twice = sources + sources[::-1] + (sources[0],)
    rp, ci, v = _run_named(ctx, "rmat10", twice)
    rows = [(ci[rp[s]:rp[s + 1]].tolist(), v[rp[s]:rp[s + 1]].tolist()) for s in range(len(twice))]
    for s, src in enumerate(twice):
        assert rows[s] == rows[twice.index(src)]


def test_one_source_and_a_source_without_out_edges(ctx):
    rp, ci, n = _graph("rmat12")
    empty = int(np.flatnonzero(np.diff(rp) == 0)[3])
    busy = int(np.argmax(np.diff(rp)))
    A = ctx.upload(rp, ci, n)
    try:
        got = _check(ctx, A, [empty], _expected("rmat12", (empty,)), what="empty row")
        assert (got[1].tolist(), got[2].tolist()) == ([empty], [0])
        R, depth, complete = ctx.bfs(A, [empty])
        assert (R.nnz, depth, complete) == (1, 0, True)
        R.free()
        _check(ctx, A, [busy], _expected("rmat12", (busy,)), what="one source")
    finally:
        A.free()


def test_unsorted_rows_with_repeats(ctx):
    rp, ci, n = _graph("rmat10")
    rng = np.random.default_rng(77)
    rows = np.repeat(np.arange(n), np.diff(rp))
    extra = rng.random(rows.size) < 0.3
    r, c = np.concatenate([rows, rows[extra]]), np.concatenate([ci, ci[extra]])
    perm = rng.permutation(r.size)
    n_rp, n_ci = gen._csr_from_pairs(r[perm], c[perm], n, dedup=False, sort=False)
    assert n_ci.size > ci.size
    sources = _sources("rmat10", 16)
    A = ctx.upload(n_rp, n_ci, n)
    try:
        _check(ctx, A, list(sources), _expected("rmat10", sources), what="noisy")
    finally:
        A.free()


@pytest.mark.parametrize("name", ["rmat12", "powerlaw"])
def test_depth_cap(ctx, name):
    sources = _sources(name, 8)
    depth = _expected(name, sources)[1]
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for cap in sorted({1, 2, depth - 1}):
            exp = _expected(name, sources, cap)
            assert exp[1:] == (cap, 0)
            _check(ctx, A, list(sources), exp, cap, "%s capped at %d" % (name, cap))
        exp = _expected(name, sources, depth)             # the full result; the cap ended the search all the same
        assert np.array_equal(exp[0][1], _expected(name, sources)[0][1]) and exp[1:] == (depth, 0)
        _check(ctx, A, list(sources), exp, depth, "%s capped at its depth" % name)
        _check(ctx, A, list(sources), _expected(name, sources, depth + 1), depth + 1, "%s cap above its depth" % name)
    finally:
        A.free()


def test_all_sources_equal_the_closure(ctx):
    rp, ci, n = _graph("uniform300")
    sources = tuple(range(n))
    A = ctx.upload(rp, ci, n)
    try:
        R, depth, complete = ctx.bfs(A, sources)
        M = ctx.matrix_from_result(R, n)
        T, _ = ctx.closure(A)
        m_rp, m_ci = M.download()
        t_rp, t_ci = T.download()
        assert complete and depth == int(_dist("uniform300", sources).max())
        assert np.array_equal(m_rp, t_rp) and np.array_equal(m_ci, t_ci) and 0 < m_ci.size < n * n
        for h in (R, M, T):
            h.free()
        _check(ctx, A, list(sources), _expected("uniform300", sources), what="all sources")
    finally:
        A.free()


def test_frontiers_and_neighbourhoods_by_value_select(ctx):
    name = "rmat12"
    sources = _sources(name, 8)
    dist = _dist(name, sources)
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        R, depth, _ = ctx.bfs(A, sources)
        for cmp, of in (("==", lambda d: dist == d), ("<=", lambda d: (dist >= 0) & (dist <= d))):
            for d in range(depth + 2):
                M = ctx.matrix_from_result_where(R, n, cmp, d)
                keep = of(d)
                e_rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
                m_rp, m_ci = M.download()
                assert np.array_equal(m_rp, e_rp) and np.array_equal(m_ci, np.nonzero(keep)[1]), (cmp, d)
                M.free()
        R.free()
    finally:
        A.free()


# ---------------------------------------------------------------- 5. errors and the check option ----------------------
def test_errors_leave_no_result_and_a_usable_context(ctx):
    L = bspgemm.lib()
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                          # 10 x n
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)

    def call(a, sources):
        src = (C.c_int * len(sources))(*sources)
        out, depth, complete = C.c_void_p(0x5A5A), C.c_int(7), C.c_int(7)
        st = L.bspgemm_bfs(ctx._h, a._h, len(sources), src, 0, C.byref(out), C.byref(depth), C.byref(complete))
        return st, out.value, L.bspgemm_last_error().decode()

    try:
        for bad in ([0, 5, n], [3, -1], [n + 7]):
            st, out, msg = call(A, bad)
            where = [i for i, s in enumerate(bad) if not 0 <= s < n][0]
            assert st == ERR_INVALID and not out and "bspgemm_bfs" in msg and "sources[%d]" % where in msg, msg
        st, out, msg = call(rect, [0])
        assert st == ERR_INVALID and not out and "bspgemm_bfs" in msg and "square" in msg, msg
        st, out, msg = call(foreign, [0])
        assert st == ERR_INVALID and not out and "bspgemm_bfs" in msg and "context" in msg, msg
        # the context still multiplies, and still searches
        P = ctx.multiply(A, A)
        assert P.nnz > 0
        P.free()
        sources = _sources("rmat10", 3)
        _check(ctx, A, list(sources), _expected("rmat10", sources), what="after the errors")
    finally:
        foreign.free()
        other.close()
        rect.free()
        A.free()


def test_check_option_changes_nothing():
    c = bspgemm.Context(0)
    try:
        c.set_option("check", 1)
        for name, count in (("rmat12", 64), ("layered", 0)):
            sources = _sources(name, count) if count else (int(bfs_ref.layered(LAYERS, 2, 11)[3][0][0]),)
            _run_named(c, name, sources)
        assert c.stats()["checked"] == 1
    finally:
        c.close()


# ---------------------------------------------------------------- 6. knobs ---------------------------------------------
@pytest.mark.parametrize("option,value", [("class_streams", 1), ("class_streams", 3), ("padded_rows", 1)])
def test_knobs_change_no_result(option, value):
    c = bspgemm.Context(0)
    try:
        c.set_option(option, value)
        sources = _sources("rmat12", 64)
        _run_named(c, "rmat12", sources)
        st = c.stats()
        assert st["class_streams" if option == "class_streams" else "padded_rows"] == value
    finally:
        c.close()
