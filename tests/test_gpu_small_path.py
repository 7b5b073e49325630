"""The small-product path (csrc/small.hip, csrc/multiply.hip multiply_small) at its row-size, fit and tile edges.

Every product runs on the path (SMALL_PATH = 1), under the automatic choice (-1), through the general flow (0) and under the
exact flow, which never takes the path; every run must give the reference CSR bit for bit -- gen.small_reference, np.unique
per row, which tests/test_small_path_shapes.py pins to the CPU oracle -- and bspgemm_stats must name the path that
gen.small_expected derives from the shape the way the library decides it: a product that fits and silently went through
the general flow fails.  Where the path ran, rows / nnz_a / products / nnz_c / bytes_alg must equal the general flow's on the
same arguments and rows_per_bin must read as multiply_small fills it.  The shapes come from tests/gen.py; that they hold
the cases they are named for (the lane/wave split at 16 products and at 16 outputs, every padding of the bitonic sort, 32
gather trips, a B row of 2048 entries, the fit limits, the scans' tile edges) is asserted there without a GPU.
"""
import numpy as np
import pytest

import bspgemm
import gen

pytestmark = pytest.mark.gpu

LADDER, FIT, TILE = gen.small_ladder_cases(), gen.small_fit_cases(), gen.small_tile_cases()
# (flow, SMALL_PATH): the general flow first, the others are compared with its statistics
RUNS = (("upper-bound", 0), ("upper-bound", 1), ("auto", -1), ("exact", 1))
SAME_STATS = ("rows", "nnz_a", "products", "nnz_c", "bytes_alg")


@pytest.fixture(scope="module")
def ctx():
    """one context for the whole file: its result cache and its statistics ring carry over from product to product"""
    c = bspgemm.Context(0)
    yield c
    c.close()


def _set(ctx, flow, small):
    ctx.set_flow(flow)
    ctx.set_option("small_path", small)


def _same(got, want, tag):
    rp, ci = got
    assert rp.shape == want[0].shape and np.array_equal(rp, want[0]), "%s: row_ptr differs (first rows %s)" % (
        tag, np.flatnonzero(rp != want[0])[:5] if rp.shape == want[0].shape else "shape")
    assert ci.shape == want[1].shape, "%s: nnz %d, expected %d" % (tag, ci.size, want[1].size)
    assert np.array_equal(ci, want[1]), "%s: col_idx differs (first at %s)" % (tag, np.flatnonzero(ci != want[1])[:5])


def _multiply(ctx, A, B, r0, r1):
    C = ctx.multiply(A, B, r0, r1)
    got, st = C.download(), ctx.stats()
    C.free()
    return got, st


def check_product(ctx, s, A, B, r0=0, r1=None, F=None, want=None, runs=RUNS, must_fit=None):
    """rows [r0, r1) of A*B under every (flow, SMALL_PATH) of `runs`: the CSR, the path that ran, the statistics.
    F, want: the rows' products and the reference CSR where A is not the whole of s (an interior upload)."""
    r1 = A.rows if r1 is None else r1
    R = r1 - r0
    F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], r0, r1) if F is None else F
    want = gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], r0, r1) if want is None else want
    nonempty = int((F > 0).sum())
    general, took = None, {}
    for flow, small in runs:
        tag = "flow=%s small_path=%d rows=[%d,%d)" % (flow, small, r0, r1)
        _set(ctx, flow, small)
        got, st = _multiply(ctx, A, B, r0, r1)
        _same(got, want, tag)
        expect = gen.small_expected(flow, small, R, A.nnz, B.nnz, B.rows, F)
        assert st["small_path"] == int(expect), "%s: small_path %d, the shape says %d" % (tag, st["small_path"], expect)
        took[(flow, small)] = st["small_path"]
        assert st["rows"] == R and st["products"] == F.sum() and st["nnz_c"] == want[1].size, (tag, st)
        if st["small_path"]:
            bins = [0] * gen.NUM_BINS
            bins[0], bins[gen.SMALL_BIN] = R - nonempty, nonempty
            assert st["rows_per_bin"] == bins and sum(bins) == R, "%s: rows per class %s" % (tag, st["rows_per_bin"])
            assert (st["flow"], st["prepass_kernel"], st["padded_rows"], st["checked"], st["class_streams"]) == (1, 2, 0, 0, 1), (tag, st)
            if general is not None:
                assert {k: st[k] for k in SAME_STATS} == {k: general[k] for k in SAME_STATS}, tag
        else:
            assert st["flow"] == (2 if flow == "exact" else 1), (tag, st["flow"])
            assert st["rows_per_bin"] == gen.expected_bins(F, s["ncols"]), "%s: rows per class %s" % (tag, st["rows_per_bin"])
            if small == 0:
                general = st
    if must_fit is not None:                               # no product that fits may pass through the general flow
        assert took[("upper-bound", 1)] == int(must_fit), "SMALL_PATH = 1: small_path %d" % took[("upper-bound", 1)]
    return took


def _upload(ctx, s):
    return ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1), ctx.upload(s["b_rp"], s["b_ci"], s["ncols"])


@pytest.mark.parametrize("name", list(LADDER))
def test_row_ladder(ctx, name):
    """rows of 1, 2, 15 .. 18, 63 .. 65, ... 2047, 2048 products of one content and one split, lane-rows and wave-rows mixed in
    the 64-row batches.  At 2^31 - 1 columns (2^31 - 2 against the sort's ~0u sentinel) the small path alone runs."""
    s = LADDER[name]()
    A, B = _upload(ctx, s)
    try:
        took = check_product(ctx, s, A, B, runs=RUNS[1:2] if s["small_only"] else RUNS, must_fit=True)
        assert took[("upper-bound", 1)] == 1
    finally:
        A.free()
        B.free()


@pytest.mark.parametrize("name", list(FIT))
def test_fit_limits(ctx, name):
    """exactly 65536 products, all distinct (the workspace and C.col_idx full to the last entry), one more (the device
    bails), one fewer; a row of 2048 / 2049 products behind row 8192; the host's limits on nnz(A), R and the automatic
    choice's estimate; the exact flow never takes the path"""
    s = FIT[name]()
    A, B = _upload(ctx, s)
    fits = name in ("fit_total_65536", "fit_total_65535", "fit_row_2048", "fit_auto_at_limit", "fit_auto_above_limit")
    try:
        took = check_product(ctx, s, A, B, must_fit=fits)
        if name.startswith("fit_auto"):
            assert took[("auto", -1)] == int(name == "fit_auto_at_limit")
        assert took[("exact", 1)] == 0 and took[("upper-bound", 0)] == 0
    finally:
        A.free()
        B.free()


@pytest.mark.parametrize("R", gen.SMALL_TILE_ROWS)
def test_tile_edges(ctx, R):
    """non-empty rows at the first and last place of the 32-row, 256-row and 8192-row tiles of the two scans, lists of 63, 64 and
    65 rows, rows whose A-entries all point at empty B rows"""
    s = TILE["tile_rows_%d" % R]()
    A, B = _upload(ctx, s)
    try:
        check_product(ctx, s, A, B, must_fit=True)
    finally:
        A.free()
        B.free()


def test_row_ranges(ctx):
    """interior row ranges that begin inside a 32-row tile, of 1, 33 and 257 rows; an A uploaded from an interior row_ptr;
    an A wrapped from device arrays that begin 4 bytes behind an aligned address"""
    import torch
    s = gen.small_range_case()
    nb = s["b_rp"].size - 1
    A, B = _upload(ctx, s)
    try:
        for r0, r1 in s["ranges"]:
            check_product(ctx, s, A, B, r0, r1, must_fit=True)
        check_product(ctx, s, A, B, must_fit=True)
        A.free()
        r0, r1 = 37, 294
        F = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], r0, r1)
        want = gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], r0, r1)
        A = ctx.upload(s["a_rp"], s["a_ci"], nb, row0=r0, rows=r1 - r0)
        assert A.rows == r1 - r0 and A.nnz == s["a_rp"][r1] - s["a_rp"][r0]
        check_product(ctx, s, A, B, F=F, want=want, must_fit=True)
        check_product(ctx, s, A, B, 5, 38, F=F[5:38], want=(want[0][5:39] - want[0][5], want[1][want[0][5]:want[0][38]]), must_fit=True)
        A.free()
        dev = torch.device("cuda", 0)
        keep = []
        for a in (s["a_rp"], s["a_ci"]):
            buf = torch.zeros(a.size + 1, dtype=torch.int32, device=dev)
            buf[1:].copy_(torch.from_numpy(np.ascontiguousarray(a, np.int32)))
            keep.append(buf)
        torch.cuda.synchronize()
        assert all(t.data_ptr() % 16 == 0 for t in keep)
        A = ctx.wrap_device(s["a_rp"].size - 1, nb, int(s["a_rp"][-1]), keep[0].data_ptr() + 4, keep[1].data_ptr() + 4, keep=tuple(keep))
        check_product(ctx, s, A, B, must_fit=True)
        check_product(ctx, s, A, B, 101, 358, must_fit=True)
    finally:
        A.free()
        B.free()


def _transpose_reference(rp, ci, cols):
    """pattern(C)^T of a CSR with sorted duplicate-free rows"""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    o = np.lexsort((rows, ci))
    return np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=cols))]).astype(np.int32), rows[o].astype(np.int32)


def test_result_as_operand(ctx):
    """the small path's result becomes an operand (matrix_from_result), equals the general flow's as a pattern on the device
    (matrix_equal), is B of another small product and is transposed"""
    s = gen.small_range_case()
    R, cols = s["a_rp"].size - 1, s["ncols"]
    want = gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"])
    x_rp, x_ci = gen.uniform_rect(60, R, 4, seed=2701)
    x_ci = x_ci[::-1].copy()                                # (every row of 4 reversed as a whole: unsorted)
    x_rp = (x_rp[-1] - x_rp[::-1]).astype(np.int32)
    A, B = _upload(ctx, s)
    X = ctx.upload(x_rp, x_ci, R)
    made = []
    try:
        for small in (1, 0):
            _set(ctx, "upper-bound", small)
            C = ctx.multiply(A, B)
            assert ctx.stats()["small_path"] == small
            made.append(ctx.matrix_from_result(C, cols))
            C.free()
        M, M0 = made
        assert (M.rows, M.cols, M.nnz) == (R, cols, want[1].size)
        assert ctx.matrix_equal(M, M0) and ctx.matrix_equal(M0, M)
        got = M.download()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # X * M on the small path, M from the small path
        c_rp = want[0].astype(np.int32)
        sx = dict(a_rp=x_rp, a_ci=x_ci, b_rp=c_rp, b_ci=want[1], ncols=cols)
        check_product(ctx, sx, X, M, must_fit=True)
        t_want = _transpose_reference(want[0], want[1], cols)
        for m in (M, M0):
            T = ctx.transpose(m)
            made.append(T)
            t_got = T.download()
            assert (T.rows, T.cols) == (cols, R)
            assert np.array_equal(t_got[0], t_want[0]) and np.array_equal(t_got[1], t_want[1])
    finally:
        for m in made + [A, B, X]:
            m.free()


def test_dropins_on_unsorted_duplicates():
    """SpGEMM_hip, SpGEMM_hip_bigslice and SpGEMM_hip_mat on an unsorted input with duplicates that their context's automatic
    choice sends down the small path (their context is not the caller's: only the CSR is seen here)"""
    rp, ci, n = gen.dups_unsorted(900, 6, 2801)
    F = gen.row_products(rp, ci, rp, 0, n)
    assert gen.small_expected("auto", -1, n, int(rp[-1]), int(rp[-1]), n, F) and F.max() > gen.SMALL_TINY
    want = gen.small_reference(rp, ci, rp, ci)
    _same(bspgemm.SpGEMM_hip(ci, rp, n, ci, rp, n), (want[0].astype(np.int32), want[1]), "SpGEMM_hip")
    _same(bspgemm.SpGEMM_hip_mat(ci, rp, n, ci, rp, n, want[1].size), (want[0].astype(np.int32), want[1]), "SpGEMM_hip_mat")
    r0, r1 = 101, 777
    F = F[r0:r1]
    assert gen.small_expected("auto", -1, r1 - r0, int(rp[-1]), int(rp[-1]), n, F)
    part = gen.small_reference(rp, ci, rp, ci, r0, r1)
    _same(bspgemm.SpGEMM_hip_bigslice(ci, rp, n, ci, rp, n, r0, r1), (part[0].astype(np.int32), part[1]), "SpGEMM_hip_bigslice")


def test_closure_runs_small_then_bails(ctx):
    """the closure of a 600-node ring with chords: its first squarings fit the small path, the later ones are found too large on
    the device (or by the host), and the result equals the closure computed without the path"""
    n = 600
    rows = [[(i + 1) % n] + ([(i + 37) % n] if i % 5 == 0 else []) for i in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.array([c for r in rows for c in r], np.int32)
    A = ctx.upload(rp, ci, n)
    try:
        _set(ctx, "upper-bound", 1)
        T, it = ctx.closure(A)
        got = T.download()
        T.free()
        assert 3 <= it <= 16
        st = [ctx.stats(age) for age in range(it - 1, -1, -1)]                  # the squarings, first to last
        path = [x["small_path"] for x in st]
        assert path[0] == 1 and path[-1] == 0 and path == sorted(path, reverse=True), path
        assert all(x["rows"] == n for x in st)
        assert [x["nnz_c"] for x in st] == sorted(x["nnz_c"] for x in st)
        bailed = [x for x in st if not x["small_path"] and x["nnz_a"] <= gen.SMALL_MAX_NNZ_A]
        assert bailed and all(x["products"] > gen.SMALL_MAX_PRODUCTS or max(x["rows_per_bin"][17:]) > 0 for x in bailed), path
        _set(ctx, "upper-bound", 0)
        T, it0 = ctx.closure(A)
        want = T.download()
        T.free()
        assert it0 == it and all(ctx.stats(age)["small_path"] == 0 for age in range(it))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[0], n * np.arange(n + 1)) and np.array_equal(got[1], np.tile(np.arange(n, dtype=np.int32), n))
    finally:
        A.free()


def test_result_cache_changes_hands(ctx):
    """40 products, small path and general flow in turn, of differing sizes, each result freed before the next: the small
    path's 65536-entry C.col_idx and the general flow's buffers come from the same cache and every result is compared"""
    cases = [gen.small_range_case(), LADDER["ladder_pairs_holes_6000"](), FIT["fit_auto_at_limit"]()]
    ops = [_upload(ctx, s) for s in cases]
    try:
        for k in range(40):
            s, (A, B) = cases[k % 3], ops[k % 3]
            r0, r1 = (3 * k) % 50, A.rows - (11 * k) % 90
            small = 1 - k % 2
            _set(ctx, "upper-bound", small)
            got, st = _multiply(ctx, A, B, r0, r1)
            assert st["small_path"] == small, (k, st["small_path"])
            _same(got, gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], r0, r1), "product %d rows=[%d,%d) small_path=%d" % (k, r0, r1, small))
    finally:
        for A, B in ops:
            A.free()
            B.free()


def test_stats_ring_counts_a_bailed_product_once(ctx):
    """bspgemm_stats_at: age 0 is the last multiply, 1 the one before.  A small-path attempt that bailed and the general flow that
    then ran are ONE multiply: after P1 (small path), P2 (bails), P3 (small path) the ages 0, 1, 2 describe P3, P2, P1, and
    after 16 products that all bail every age 0 .. 15 answers."""
    s1, s2 = gen.small_range_case(), FIT["fit_row_2049"]()
    F1 = gen.row_products(s1["a_rp"], s1["a_ci"], s1["b_rp"], 0, s1["a_rp"].size - 1)
    F2 = gen.row_products(s2["a_rp"], s2["a_ci"], s2["b_rp"], 0, s2["a_rp"].size - 1)
    R2 = F2.size
    (A1, B1), (A2, B2) = _upload(ctx, s1), _upload(ctx, s2)
    try:
        _set(ctx, "upper-bound", 1)
        for A, B, r0, r1 in ((A1, B1, 37, 70), (A2, B2, 0, R2), (A1, B1, 101, 358)):
            ctx.multiply(A, B, r0, r1).free()
        got = [ctx.stats(age) for age in range(3)]
        seen = [(x["rows"], x["products"], x["small_path"]) for x in got]
        assert seen == [(257, F1[101:358].sum(), 1), (R2, F2.sum(), 0), (33, F1[37:70].sum(), 1)], seen
        assert got[1]["flow"] == 1 and got[1]["rows_per_bin"] == gen.expected_bins(F2, s2["ncols"])
        for k in range(16):
            ctx.multiply(A2, B2, 0, R2 - k).free()
        for age in range(16):
            x = ctx.stats(age)
            assert (x["rows"], x["products"], x["small_path"]) == (R2 - 15 + age, F2[:R2 - 15 + age].sum(), 0), (age, x)
    finally:
        for m in (A1, B1, A2, B2):
            m.free()
