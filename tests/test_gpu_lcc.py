"""The device-resident local clustering coefficient (bspgemm_local_clustering): counts, degrees and the coefficients' bits
against the scipy model of lcc_ref.py, info.triangles against bspgemm_triangle_count, undirected and directed.

What can go wrong is the crediting of a triangle that is walked once to its three corners: the per-hit atomic on the lowest
corner (a hub's counter takes one from every wave), the per-entry one, and the credit a lane keeps in a register while it
stays in a row and has to flush when the row ends inside its four entries, at a tile's end or after the walk; the directed
weights, read through the positions of a hit in BOTH rows, whichever of the two is walked; the light / heavy split at every
BSPGEMM_OPT_DOT_LIGHT (0: every entry by a wave, 2^30: every entry by a lane) with rows that straddle the 64-lane step and
the heavy kernel's trips; the per-workgroup credit cache in LDS (a hub that every workgroup credits, vertices beyond its 1024
slots that share a slot); and select's geometry (tiles of kSelTile entries, more than kSelStage empty rows in a tile).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import gen
import kcore_ref
import lcc_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
NAME = "bspgemm_local_clustering"
LIGHTS = (0, lcc_ref.LIGHT_DEFAULT, 2**30)


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.set_option("dot_light", lcc_ref.LIGHT_DEFAULT)
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    return lcc_ref.GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def _expected(name, directed):
    """the model's five, the entries of the walked half and the heavy ones under every LIGHTS; computed once and read-only"""
    rp, ci, n = _graph(name)
    exp = lcc_ref.local_clustering(rp, ci, n, directed)
    for a in exp[:3]:
        a.setflags(write=False)
    return exp + (lcc_ref.half_entries(rp, ci, n), tuple(lcc_ref.heavy_entries(rp, ci, n, t) for t in LIGHTS))


def _check(ctx, A, exp, directed, light=lcc_ref.LIGHT_DEFAULT, what=""):
    """run the call on operand A and compare everything; returns (num, info)"""
    e_num, e_d, e_lcc, e_triangles, e_reciprocal, e_entries, e_heavy = exp
    n = e_num.size
    R, d, lcc, info = ctx.local_clustering(A, directed)
    try:
        assert (R.rows, R.nnz) == (n, n), what
        rp, ci = R.download()
        num = R.download_values()
        print("LCC %-40s directed %d light %10d: info %s" % (what, directed, light, info))
        assert rp.dtype == np.int64 and np.array_equal(rp, np.arange(n + 1)) and np.array_equal(ci, np.arange(n)), what
        assert num.dtype == np.int32 and np.array_equal(num, e_num), (what, directed, light, np.flatnonzero(num != e_num)[:8])
        assert d.dtype == np.int32 and np.array_equal(d, e_d), (what, directed)
        assert lcc.dtype == np.float64 and lcc.tobytes() == e_lcc.tobytes(), (what, directed)       # the bits
        assert R.values_sum() == int(e_num.sum(dtype=np.int64)), what
        assert info["triangles"] == e_triangles and info["entries"] == e_entries and info["reciprocal"] == e_reciprocal, \
            (what, directed, info, exp[3:])
        assert info["heavy_entries"] == e_heavy[LIGHTS.index(light)], (what, directed, light, info, e_heavy)
    finally:
        R.free()
    return num, info


# ---------------------------------------------------------------- 1. every named graph, every split, both modes ---------
@pytest.mark.parametrize("name", list(lcc_ref.GRAPHS))
def test_counts_equal_the_model(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    S = ctx.symmetrize(A, drop_diagonal=True)
    try:
        triangles = ctx.triangle_count(S)
        first = {}
        for light in LIGHTS:
            ctx.set_option("dot_light", light)
            for directed in (False, True):
                exp = _expected(name, directed)
                assert exp[3] == triangles
                num, info = _check(ctx, A, exp, directed, light, what=name)
                first.setdefault(directed, num)
                assert np.array_equal(num, first[directed])               # equal bits under every split
                if light == 0:
                    assert info["heavy_entries"] <= info["entries"]
                if light == 2**30:
                    assert info["heavy_entries"] == 0
    finally:
        ctx.set_option("dot_light", lcc_ref.LIGHT_DEFAULT)
        S.free()
        A.free()


def test_the_named_graphs_do_what_they_are_there_for():
    T = lcc_ref.LIGHT_DEFAULT
    for name in ("k70", "k258", "k258_oriented", "rmat11"):                   # both kernels credit at the default split
        e = _expected(name, True)
        assert 0 < e[6][LIGHTS.index(T)] < e[5], name
    for name in ("friendship_hub_first", "friendship_hub_last"):             # the hub's counter: 3000 triangles, twice each
        num = _expected(name, False)[0]
        assert num.max() == 6000 and _expected(name, False)[5] == 9000 > 2 * lcc_ref.K_SEL_TILE
    for name in ("empty0", "empty1", "empty1000", "self_loops5", "star5000"):
        assert not _expected(name, False)[0].any() and not _expected(name, True)[0].any() and _expected(name, True)[3] == 0
    und, dire = _expected("k258_oriented", False), _expected("k258_oriented", True)
    assert (und[0] == 257 * 256).all() and (und[2] == 1.0).all() and (dire[0] < und[0]).all() and dire[4] > 5000


# ---------------------------------------------------------------- 2. where the operand comes from ----------------------
def test_operand_provenance(ctx):
    """an upload, wrapped device arrays one int off 16-byte alignment, the transpose (the loader's in-edges), a select and
    an already symmetrized operand: the same counts (the symmetrized one: the undirected counts in both modes)"""
    import torch
    name = "rmat11"
    rp, ci, n = _graph(name)
    handles = []

    def both(M, what, symmetric=False):
        handles.append(M)
        for directed in (False, True):
            exp = _expected(name, directed)
            if symmetric and directed:
                und = _expected(name, False)
                exp = und[:4] + (und[5],) + und[5:]                           # every edge both ways: reciprocal = entries
            _check(ctx, M, exp, directed, what=what)

    A = ctx.upload(rp, ci, n)
    both(A, "upload")
    trp = torch.from_numpy(rp).cuda()
    buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + ci.size] = torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    tci = buf[1:]
    assert tci.data_ptr() % 16 == 4
    both(ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf)), "wrapped, col_idx 4 bytes off alignment")
    both(ctx.transpose(A), "transpose")
    both(ctx.select(A, "offdiag"), "select")
    both(ctx.symmetrize(A, drop_diagonal=True), "symmetrized", symmetric=True)
    for h in handles:
        h.free()


# ---------------------------------------------------------------- 3. an independent route on the device ----------------
@pytest.mark.parametrize("name", ["untidy150", "k258_oriented", "rmat11"])
def test_counts_equal_the_row_sums_of_the_masked_dot(ctx, name):
    """num = rowsum(S .* (S * B^T)), the product by bspgemm_multiply_masked_dot and B from public calls: S itself, or the
    off-diagonal entries of A (the masked dot makes them canonical itself)"""
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    S = ctx.symmetrize(A, drop_diagonal=True)
    off = ctx.select(A, "offdiag")
    try:
        for directed in (False, True):
            D, _ = ctx.multiply_masked_dot(S, off if directed else S, S)
            d_rp, _ = D.download()
            vals = D.download_values().astype(np.int64)
            D.free()
            rows = np.repeat(np.arange(n), np.diff(d_rp))
            sums = np.bincount(rows, weights=vals, minlength=n).astype(np.int64)
            R, _, _, _ = ctx.local_clustering(A, directed)
            num = R.download_values()
            R.free()
            assert np.array_equal(num, sums), (name, directed)
            assert np.array_equal(num, _expected(name, directed)[0])
    finally:
        off.free()
        S.free()
        A.free()


# ---------------------------------------------------------------- 4. selectors, statistics, optional outputs -----------
def test_vertex_selectors_statistics_optional_outputs_and_repeatability(ctx):
    name = "rmat11"
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    P = ctx.multiply(A, A)
    out = C.c_void_p()
    try:
        before = ctx.stats()
        first = _check(ctx, A, _expected(name, True), True, what="first")
        second = _check(ctx, A, _expected(name, True), True, what="second")
        assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]          # two runs: equal bits
        assert ctx.stats() == before and before["rows"] == n
        R, _, _, _ = ctx.local_clustering(A)
        e_num = _expected(name, False)[0]
        D = ctx.matrix_from_result_where(R, n, ">=", 100)                     # the vertices in at least 50 triangles
        d_rp, d_ci = D.download()
        assert np.array_equal(d_ci, np.flatnonzero(e_num >= 100)) and 0 < d_ci.size < n
        assert np.array_equal(np.diff(d_rp), (e_num >= 100).astype(np.int32))
        D.free()
        R.free()
        # every optional output NULL
        assert bspgemm.lib().bspgemm_local_clustering(ctx._h, A._h, 1, C.byref(out), None, None, None) == 0
        num = np.zeros(n, np.int32)
        assert bspgemm.lib().bspgemm_result_download_values(ctx._h, out, num.ctypes.data) == 0
        assert np.array_equal(num, _expected(name, True)[0])
    finally:
        bspgemm.lib().bspgemm_result_free(out)
        P.free()
        A.free()


# ---------------------------------------------------------------- 5. errors --------------------------------------------
def test_errors_leave_no_result_and_a_usable_context(ctx):
    L = bspgemm.lib()
    name = "rmat8"
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                          # 10 x n
    import torch
    trp = torch.from_numpy(rp).cuda()
    wrapped = []
    for at, col in ((ci.size // 2, n), (ci.size - 1, -1), (0, 2**31 - 1)):   # checked on the device before it indexes
        c = ci.copy()
        c[at] = col
        tci = torch.from_numpy(c).cuda()
        wrapped.append(ctx.wrap_device(n, n, c.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, tci)))
    torch.cuda.synchronize()
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)

    def call(a, flags=0):
        out, info = C.c_void_p(0x5A5A), bspgemm.LccInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        d, lcc = np.full(n, -7, np.int32), np.full(n, -7.0)
        st = L.bspgemm_local_clustering(ctx._h, a._h, flags, C.byref(out), d.ctypes.data, lcc.ctypes.data, C.byref(info))
        return st, out.value, L.bspgemm_last_error().decode(), bytes(info) == bytes(C.sizeof(info))

    try:
        for flags in (0, 1):
            st, out, msg, zeroed = call(rect, flags)
            assert st == ERR_INVALID and not out and NAME in msg and "square" in msg and zeroed, msg
            st, out, msg, zeroed = call(foreign, flags)
            assert st == ERR_INVALID and not out and NAME in msg and "context" in msg and zeroed, msg
            for W in wrapped:
                st, out, msg, zeroed = call(W, flags)
                assert st == ERR_INVALID and not out and "column" in msg and zeroed, msg
        st, out, msg, zeroed = call(A, 2)
        assert st == ERR_INVALID and not out and NAME in msg and "flag" in msg and zeroed, msg
        # the context still multiplies correctly, and still counts
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        for directed in (False, True):
            _check(ctx, A, _expected(name, directed), directed, what="after the errors")
    finally:
        foreign.free()
        other.close()
        for W in wrapped:
            W.free()
        rect.free()
        A.free()


# ---------------------------------------------------------------- 6. a seeded random campaign ---------------------------
def _campaign_case(i):
    rng = np.random.default_rng(5570 + i)
    kind = ("rmat", "powerlaw", "uniform", "dups_unsorted", "untidy")[i % 5]
    if kind == "rmat":
        rp, ci, n = gen.rmat(int(rng.integers(6, 11)), int(rng.integers(2, 12)), kcore_ref.SKEW, 5600 + i)
    elif kind == "powerlaw":
        rp, ci, n = gen.powerlaw(int(rng.integers(100, 3001)), int(rng.integers(2, 6)), 5600 + i)
    elif kind == "uniform":
        rp, ci, n = gen.uniform(int(rng.integers(50, 2001)), int(rng.integers(1, 10)), 5600 + i)
    elif kind == "dups_unsorted":
        rp, ci, n = gen.dups_unsorted(int(rng.integers(50, 2001)), int(rng.integers(1, 8)), 5600 + i)
    else:
        n = int(rng.integers(30, 400))
        rp, ci, n = lcc_ref.untidy(n, int(rng.integers(2, 12)) * n, 5600 + i)
    return kind, rp, ci, n, bool(i & 1), LIGHTS[int(rng.integers(0, 3))]


@pytest.mark.parametrize("i", range(15))
def test_random_campaign(ctx, i):
    kind, rp, ci, n, directed, light = _campaign_case(i)
    exp = lcc_ref.local_clustering(rp, ci, n, directed)
    exp = exp + (lcc_ref.half_entries(rp, ci, n), tuple(lcc_ref.heavy_entries(rp, ci, n, t) for t in LIGHTS))
    A = ctx.upload(rp, ci, n)
    ctx.set_option("dot_light", light)
    try:
        _check(ctx, A, exp, directed, light, what="case %d: %s n %d" % (i, kind, n))
    finally:
        ctx.set_option("dot_light", lcc_ref.LIGHT_DEFAULT)
        A.free()
