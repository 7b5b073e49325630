"""The on-device submatrix extraction (bspgemm_matrix_extract, bspgemm_matrix_extract_rows_of): row_ptr and col_idx of the
downloaded operand and every info field are EQUAL to the model's (extract_ref.py), on the edge graphs whose claims
test_extract_shapes.py checks on the host -- the lane groups, the hub chunks, the sort classes -- under every EXTRACT_LANES,
on every form of operand, against the routes that exist already (the two-product route, bspgemm_kcore, the triangle count,
the oracle's product), with the lists read on the device, and through every error of the device path.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import gen
import extract_ref as X

pytestmark = pytest.mark.gpu
ERR_INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _model(key, keep):
    """the model of a named case, computed once and read-only"""
    rp, ci, rows, cols, I, J = _CASES[key]()
    m = X.model(rp, ci, rows, cols, I, J, keep)
    for k in ("rp", "ci"):
        m[k].setflags(write=False)
    return m


def _compare(S, info, m, what, lanes=0):
    try:
        assert (S.rows, S.cols) == tuple(m["shape"]) and S.nnz == m["kept"], (what, S.rows, S.cols, S.nnz)
        rp, ci = S.download()
        assert rp.dtype == np.int32 and np.array_equal(rp, m["rp"]), what
        assert ci.dtype == np.int32 and np.array_equal(ci, m["ci"]), what
        assert {k: info[k] for k in X.INFO} == {k: m[k] for k in X.INFO}, (what, info)
        assert info["lanes"] == (lanes if lanes else X.lanes_auto(m["scanned"], m["walked"])), (what, info)
    finally:
        S.free()


def _check(ctx, A, src, I=None, J=None, keep=False, what="", lanes=0, m=None):
    """the host-list call on operand A against the model of the host arrays src = (rp, ci, rows, cols)"""
    m = X.model(*src, I, J, keep) if m is None else m
    S, info = ctx.extract(A, I, J, keep_shape=keep)
    _compare(S, info, m, what, lanes)
    return m


def _every_width(ctx, fn):
    try:
        for lanes in X.LANES:
            ctx.set_option("extract_lanes", lanes)
            fn(lanes)
    finally:
        ctx.set_option("extract_lanes", 0)


def _reversed_lane():
    rp, ci, rows, cols, I, J = X.lane_case()
    return rp, ci, rows, cols, I, J[::-1].copy()


_CASES = {"lane": X.lane_case, "lane_reversed": _reversed_lane, "hub": X.hub_case}


# ---------------------------------------------------------------- 1. lane groups, hubs, sort classes -------------------
def test_extract_lanes_option(ctx):
    for bad in (-1, 1, 8, 32, 128):
        with pytest.raises(bspgemm.BspgemmError):
            ctx.set_option("extract_lanes", bad)
    assert ctx.get_option("extract_lanes") == 0
    ctx.set_option("extract_lanes", 16)
    assert ctx.get_option("extract_lanes") == 16
    ctx.set_option("extract_lanes", 0)


@pytest.mark.parametrize("case", ["lane", "lane_reversed"])
@pytest.mark.parametrize("keep", [False, True])
def test_lane_groups_under_every_width(ctx, case, keep):
    rp, ci, rows, cols, I, J = _CASES[case]()
    A = ctx.upload(rp, ci, cols)
    try:
        m = _model(case, keep)
        assert m["sorted_by"] == (1 if case == "lane_reversed" and not keep else 0)
        _every_width(ctx, lambda lanes: _check(ctx, A, None, I, J, keep, "%s lanes %d" % (case, lanes), lanes, m))
    finally:
        A.free()


@pytest.mark.parametrize("keep", [False, True])
def test_hubs_under_every_width(ctx, keep):
    rp, ci, rows, cols, I, J = X.hub_case()
    A = ctx.upload(rp, ci, cols)
    try:
        m = _model("hub", keep)
        assert m["hub_chunks"] == (14 if keep else 17) and m["sorted_by"] == 0
        _every_width(ctx, lambda lanes: _check(ctx, A, None, I, J, keep, "hub lanes %d" % lanes, lanes, m))
        # the same rows under a column list that is not ascending: the hubs' out rows pass the workgroup cap
        m2 = _check(ctx, A, (rp, ci, rows, cols), I, J[::-1].copy(), keep, "hub, reversed J")
        assert m2["sorted_by"] == (0 if keep else 2) and m2["kept_rows"].max() > X.SORT_BLOCK
    finally:
        A.free()


def test_sort_classes(ctx):
    rng = np.random.default_rng(11)
    for fallback in (False, True):
        rp, ci, rows, cols = X.sort_case(fallback)
        A = ctx.upload(rp, ci, cols)
        try:
            for name, J in (("reversed", np.arange(cols, dtype=np.int32)[::-1].copy()), ("permuted", rng.permutation(cols).astype(np.int32))):
                m = _check(ctx, A, (rp, ci, rows, cols), None, J, False, "sort %s fallback %d" % (name, fallback))
                assert m["sorted_by"] == (2 if fallback else 1) and m["cols_monotone"] == 0
            m = _check(ctx, A, (rp, ci, rows, cols), None, np.arange(0, cols, 7, dtype=np.int32), False, "monotone, skipping")
            assert m["cols_monotone"] == 1 and m["sorted_by"] == 0
        finally:
            A.free()


# ---------------------------------------------------------------- 2. shapes and forms ----------------------------------
def test_shapes_and_forms(ctx):
    import torch
    rp, ci, n = gen.rmat(11, 8, (0.45, 0.22, 0.22, 0.11), seed=31)
    src = (rp, ci, n, n)
    rng = np.random.default_rng(32)
    I, J = rng.integers(0, n, 700).astype(np.int32), rng.permutation(n)[:900].astype(np.int32)
    A = ctx.upload(rp, ci, n)
    T = ctx.transpose(A)
    TT = ctx.transpose(T)
    S, info = ctx.extract(A)                                     # both lists NULL: the double transpose
    assert ctx.matrix_equal(S, TT) and np.array_equal(S.download()[1], TT.download()[1]) and info["kept"] == TT.nnz
    S.free()
    for keep in (False, True):
        _check(ctx, A, src, I, J, keep, "rmat11")
        _check(ctx, A, src, np.zeros(0, np.int32), J, keep, "ni = 0")
        _check(ctx, A, src, I, np.zeros(0, np.int32), keep, "nj = 0")
        _check(ctx, A, src, None, J, keep, "I NULL")
        _check(ctx, A, src, I, None, keep, "J NULL")
    # A with no rows, A with no entries, a rectangular operand
    E0 = ctx.upload(np.zeros(1, np.int32), np.zeros(0, np.int32), 50)
    E1 = ctx.upload(np.zeros(41, np.int32), np.zeros(0, np.int32), 50)
    for keep in (False, True):
        _check(ctx, E0, (np.zeros(1, np.int32), np.zeros(0, np.int32), 0, 50), None, [3, 1], keep, "no rows")
        _check(ctx, E1, (np.zeros(41, np.int32), np.zeros(0, np.int32), 40, 50), [5, 5, 39], [49, 0], keep, "no entries")
    rrp, rci = gen.uniform_rect(300, 200, 5, seed=3)
    Rm = ctx.upload(rrp, rci, 200)
    for keep in (False, True):
        _check(ctx, Rm, (rrp, rci, 300, 200), rng.integers(0, 300, 120), rng.permutation(200)[:77], keep, "300 x 200")
    # an interior-row_ptr upload, wrapped device arrays one int off 16-byte alignment
    extra = gen.uniform_rect(37, n, 3, 5450)
    tall_rp = np.concatenate([extra[0], extra[0][-1] + rp[1:]]).astype(np.int32)
    tall_ci = np.concatenate([extra[1], ci]).astype(np.int32)
    In = ctx.upload(tall_rp, tall_ci, n, row0=37, rows=n)
    trp = torch.from_numpy(rp).cuda()
    buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + ci.size] = torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    assert buf[1:].data_ptr() % 16 == 4
    W = ctx.wrap_device(n, n, ci.size, trp.data_ptr(), buf[1:].data_ptr(), keep=(trp, buf))
    for keep in (False, True):
        _check(ctx, In, src, I, J, keep, "interior upload")
        _check(ctx, W, src, I, J, keep, "wrapped, 4 bytes off alignment")
    # an untidy operand
    urp, uci, un = gen.dups_unsorted(500, 6, seed=9)
    U = ctx.upload(urp, uci, un)
    p = rng.permutation(un).astype(np.int32)
    for keep in (False, True):
        m = _check(ctx, U, (urp, uci, un, un), p, p, keep, "untidy")
        assert m["canonicalised"] == 1
    m = _check(ctx, U, (urp, uci, un, un), None, None, False, "untidy, both NULL")
    assert m["canonicalised"] == 1 and m["kept"] < uci.size
    for h in (A, T, TT, E0, E1, Rm, In, W, U):
        h.free()


# ---------------------------------------------------------------- 3. against the code that exists ----------------------
def _diag(ctx, n, members):
    """the diagonal selector D: (v, v) for v in members"""
    on = np.zeros(n, bool)
    on[np.asarray(members, np.int64)] = True
    rp = np.concatenate([[0], np.cumsum(on)]).astype(np.int32)
    return ctx.upload(rp, np.flatnonzero(on).astype(np.int32), n)


def test_keep_shape_equals_the_product_route(ctx):
    rp, ci, n = gen.rmat(11, 8, (0.45, 0.22, 0.22, 0.11), seed=33)
    rng = np.random.default_rng(34)
    I, J = rng.integers(0, n, 900).astype(np.int32), rng.integers(0, n, 1100).astype(np.int32)
    A, DI, DJ = ctx.upload(rp, ci, n), _diag(ctx, n, I), _diag(ctx, n, J)
    R1 = ctx.multiply(DI, A)
    M1 = ctx.matrix_from_result(R1, n)
    R2 = ctx.multiply(M1, DJ)
    M2 = ctx.matrix_from_result(R2, n)
    S, info = ctx.extract(A, I, J, keep_shape=True)
    assert ctx.matrix_equal(S, M2)
    (srp, sci), (mrp, mci) = S.download(), M2.download()
    assert np.array_equal(srp, mrp) and np.array_equal(sci, mci) and info["kept"] == M2.nnz
    for h in (R1, R2):
        h.free()
    for h in (A, DI, DJ, M1, M2, S):
        h.free()


def test_keep_shape_on_the_core_vertices_equals_kcore(ctx):
    rp, ci, n = gen.rmat(11, 8, (0.45, 0.22, 0.22, 0.11), seed=35)
    A = ctx.upload(rp, ci, n)
    Sy = ctx.symmetrize(A, drop_diagonal=True)
    cores, top, _ = ctx.core_numbers(A)
    core = cores.download_values()
    assert top >= 4
    for k in (0, top // 2, top + 1):
        K, _ = ctx.kcore(A, k)
        V = np.flatnonzero(core >= k).astype(np.int32)
        S, info = ctx.extract(Sy, V, V, keep_shape=True)
        sel = ctx.matrix_from_result_where(cores, n, ">=", k)
        S2, info2 = ctx.extract_rows_of(Sy, sel, -1, sel, -1, keep_shape=True)
        krp, kci = K.download()
        for got, what in ((S, "host lists"), (S2, "device lists")):
            assert ctx.matrix_equal(got, K), (k, what)
            grp, gci = got.download()
            assert np.array_equal(grp, krp) and np.array_equal(gci, kci), (k, what)
        assert info == info2 and info["kept"] == K.nnz, (k, info, info2)
        assert (K.nnz == 0) == (k == top + 1)
        for h in (K, S, S2, sel):
            h.free()
    cores.free()
    Sy.free()
    A.free()


def test_permutation_round_trip_and_triangles(ctx):
    rp, ci, n = gen.rmat(11, 8, (0.45, 0.22, 0.22, 0.11), seed=37)
    A0 = ctx.upload(rp, ci, n)
    A = ctx.symmetrize(A0, drop_diagonal=True)
    arp, aci = A.download()
    deg = np.diff(arp)
    p = np.argsort(-deg, kind="stable").astype(np.int32)          # the degree-descending relabelling
    inv = np.empty(n, np.int32)
    inv[p] = np.arange(n, dtype=np.int32)
    B, info = ctx.extract(A, p, p)
    assert info["cols_monotone"] == 0 and info["sorted_by"] in (1, 2) and info["kept"] == A.nnz
    brp, bci = B.download()
    m = X.model(arp, aci, n, n, p, p)
    assert np.array_equal(brp, m["rp"]) and np.array_equal(bci, m["ci"]) and info["sorted_by"] == m["sorted_by"]
    assert np.array_equal(np.diff(brp), deg[p])
    Bk, _ = ctx.extract(B, inv, inv)
    assert ctx.matrix_equal(Bk, A)
    krp, kci = Bk.download()
    assert np.array_equal(krp, arp) and np.array_equal(kci, aci)
    assert ctx.triangle_count(B) == ctx.triangle_count(A) > 0
    for h in (A0, A, B, Bk):
        h.free()


def test_the_extracted_operand_in_a_product(ctx):
    from oracle import oracle as O
    rp, ci, n = gen.rmat(10, 8, (0.45, 0.22, 0.22, 0.11), seed=39)
    rng = np.random.default_rng(40)
    V = rng.permutation(n)[:600].astype(np.int32)
    A = ctx.upload(rp, ci, n)
    S, _ = ctx.extract(A, V, V)
    m = X.model(rp, ci, n, n, V, V)
    erp, eci = O.spgemm(m["rp"], m["ci"], m["rp"], m["ci"], V.size)
    R = ctx.multiply(S, S)                                       # as A and as B
    crp, cci = R.download()
    assert np.array_equal(crp, erp) and np.array_equal(cci, eci)
    R.free()
    S.free()
    A.free()


# ---------------------------------------------------------------- 4. device lists --------------------------------------
def test_rows_of_equals_the_host_lists(ctx):
    # a few components: disjoint blocks of an R-MAT, vertices interleaved so that the member lists are not ranges
    rp0, ci0, n0 = gen.rmat(9, 6, (0.45, 0.22, 0.22, 0.11), seed=41)
    parts, n = 5, 5 * n0
    rows = np.repeat(np.arange(n0), np.diff(rp0))
    r = np.concatenate([rows * parts + q for q in range(parts)])
    c = np.concatenate([ci0.astype(np.int64) * parts + q for q in range(parts)])
    rp, ci = gen._csr_from_pairs(r, c, n)
    A = ctx.upload(rp, ci, n)
    P, ncomp, _ = ctx.connected_components(A)
    PT = ctx.transpose(P)
    label = P.download()[1]
    assert ncomp >= parts
    big = [int(x) for x in np.unique(label) if np.count_nonzero(label == x) > 1]
    assert len(big) >= parts
    for keep in (False, True):
        for lab in big + [int(np.flatnonzero(np.bincount(label, minlength=n) == 1)[0])]:
            members = np.flatnonzero(label == lab).astype(np.int32)
            S1, i1 = ctx.extract(A, members, members, keep_shape=keep)
            S2, i2 = ctx.extract_rows_of(A, PT, lab, PT, lab, keep_shape=keep)
            m = X.model(rp, ci, n, n, members, members, keep)
            (r1, c1), (r2, c2) = S1.download(), S2.download()
            assert np.array_equal(r1, r2) and np.array_equal(c1, c2) and i1 == i2, (lab, keep)
            assert np.array_equal(r1, m["rp"]) and np.array_equal(c1, m["ci"]) and i1["kept"] == m["kept"]
            S1.free()
            S2.free()
        # one list on the device, the other "all"
        lab = big[0]
        members = np.flatnonzero(label == lab).astype(np.int32)
        S2, i2 = ctx.extract_rows_of(A, PT, lab, None, -1, keep_shape=keep)
        _compare(S2, i2, X.model(rp, ci, n, n, members, None, keep), "MJ NULL")
        S2, i2 = ctx.extract_rows_of(A, None, 0, PT, lab, keep_shape=keep)
        _compare(S2, i2, X.model(rp, ci, n, n, None, members, keep), "MI NULL")
    # an empty row of PT: a vertex that labels no component
    empty = int(np.flatnonzero(np.bincount(label, minlength=n) == 0)[0])
    S2, i2 = ctx.extract_rows_of(A, PT, empty, PT, empty)
    _compare(S2, i2, X.model(rp, ci, n, n, [], []), "empty lists")
    for h in (A, P, PT):
        h.free()


# ---------------------------------------------------------------- 5. errors --------------------------------------------
def _raw(ctx, fn, *args):
    """(status, out handle value, info bytes, message) of a raw call"""
    L = bspgemm.lib()
    info, out = bspgemm.ExtractInfo(), C.c_void_p(77)
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    st = getattr(L, fn)(ctx._h, *args, C.byref(out), C.byref(info))
    return st, out.value, bytes(info), L.bspgemm_last_error().decode(errors="replace")


def test_errors_on_the_device_path(ctx):
    rp, ci, n = gen.rmat(10, 8, (0.45, 0.22, 0.22, 0.11), seed=43)
    src = (rp, ci, n, n)
    A = ctx.upload(rp, ci, n)
    good = np.array([5, 900, 17], np.int32)
    one = np.array([0, 3], np.int32)
    beyond = ctx.upload(one, np.array([4, n + 2, 9], np.int32), n + 10)        # an entry outside [0, n)
    twice = ctx.upload(one, np.array([8, 2, 8], np.int32), n)                 # a column named twice
    narrow = ctx.upload(rp, ci, int(ci.max()))                                  # a column of A outside [0, A.cols)
    fine = ctx.upload(one, good, n)
    NAME = "bspgemm_matrix_extract_rows_of"
    zero = bytes(C.sizeof(bspgemm.ExtractInfo))

    def refused(args, *words):
        st, out, info, msg = _raw(ctx, NAME, *args)
        assert st == ERR_INVALID and out is None and info == zero, (st, out, msg)
        assert NAME in msg and all(w in msg for w in words), msg
        _check(ctx, A, src, good, good, False, "after " + msg)               # the context stays usable

    refused((A._h, beyond._h, 0, fine._h, 0, 0), "row list MI", "outside")
    refused((A._h, fine._h, 0, beyond._h, 0, 0), "column list MJ", "outside")
    refused((A._h, fine._h, 0, beyond._h, -1, 1), "column list MJ", "outside")
    refused((A._h, fine._h, 0, twice._h, 0, 0), "twice", "MJ")
    refused((narrow._h, fine._h, 0, fine._h, 0, 0), "column index outside", "operand A")
    refused((A._h, fine._h, 1, fine._h, 0, 0), "row 1 of MI")
    refused((A._h, fine._h, 0, fine._h, -2, 0), "row -2 of MJ")
    S, info = ctx.extract_rows_of(A, fine, 0, twice, 0, keep_shape=True)       # repeats are harmless under KEEP_SHAPE
    _compare(S, info, X.model(rp, ci, n, n, good, [8, 2, 8], True), "repeats, KEEP_SHAPE")
    other = bspgemm.Context(0)
    try:
        B = other.upload(rp, ci, n)
        st, out, info, msg = _raw(ctx, NAME, B._h, None, -1, None, -1, 0)
        assert st == ERR_INVALID and out is None and "another context" in msg and NAME in msg
        st, out, info, msg = _raw(ctx, NAME, A._h, B._h, 0, None, -1, 0)
        assert st == ERR_INVALID and out is None and "another context" in msg
        B.free()
    finally:
        other.close()
    for h in (A, beyond, twice, narrow, fine):
        h.free()


def test_errors_of_the_host_lists(ctx):
    rp, ci, n = gen.rmat(10, 8, (0.45, 0.22, 0.22, 0.11), seed=43)
    A = ctx.upload(rp, ci, n)
    NAME = "bspgemm_matrix_extract"
    zero = bytes(C.sizeof(bspgemm.ExtractInfo))

    def refused(I, J, flags, *words):
        I, J = np.asarray(I, np.int32), np.asarray(J, np.int32)
        st, out, info, msg = _raw(ctx, NAME, A._h, I.size, I.ctypes.data, J.size, J.ctypes.data, flags)
        assert st == ERR_INVALID and out is None and info == zero, (st, out, msg)
        assert NAME in msg and all(w in msg for w in words), msg

    refused([0, n, 1], [0, 1], 0, "row list I", "I[1]")
    refused([0, -1], [0, 1], 1, "row list I", "I[1]")
    refused([0, 1], [2, 5, n + 7], 0, "column list J", "J[2]")
    refused([0, 1], [2, 5, 9, 5], 0, "twice", "J[3]")
    S, info = ctx.extract(A, [0, 1], [2, 5, 9, 5], keep_shape=True)
    _compare(S, info, X.model(rp, ci, n, n, [0, 1], [2, 5, 9, 5], True), "repeats, KEEP_SHAPE")
    A.free()


def test_timing_line(capfd, monkeypatch):
    monkeypatch.setenv("BSPGEMM_EXTRACT_TIMING", "1")                            # read once, in bspgemm_create
    timed = bspgemm.Context(0)
    monkeypatch.delenv("BSPGEMM_EXTRACT_TIMING")
    try:
        rp, ci, rows, cols, I, J = X.hub_case()
        A = timed.upload(rp, ci, cols)
        capfd.readouterr()
        _check(timed, A, None, I, J, False, "timed", 0, _model("hub", False))
        err = capfd.readouterr().err
        line = [ln for ln in err.splitlines() if "bspgemm_matrix_extract" in ln]
        assert len(line) == 1, err
        for word in ("kept %d" % _model("hub", False)["kept"], "hub chunks 17", "maps and checks", "count", "hub launches", "scan",
                     "read-back two", "emit", "sort"):
            assert word in line[0], line[0]
        A.free()
    finally:
        timed.close()
