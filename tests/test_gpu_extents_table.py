"""B's blocked extents table (csrc/prepass.hip k_blk16 / blk16_extent / k_row_work_flat): 16 bytes per 16 rows of B, the
group's start and 16 six-bit lengths clamped to 63, five to a word and the 16th in the words' top bits.  Forced on small
operands (BSPGEMM_OPT_BLOCKED_EXTENTS = 1, bspgemm_stats.prepass_kernel says that it ran), at every length and group
offset where the decode takes another turn, compared completely against the oracle and against the same product with
the table forbidden."""
import numpy as np
import pytest

import bspgemm
import gen
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GROUP = 16
B_ROWS = 1003                                   # 62 whole groups and one of 11 rows
NCOLS = 9000
A_ROWS = 700


def _special_lengths(beside_clamp):
    """{B row: length}: every length of `beside_clamp` at group offsets 0, 7 and 15, each in a group of its own whose
    successor is left alone (a clamped row must not reach into the next group); lengths at the offsets where a word of
    five fields ends or begins; one group of nothing but 62s (the largest sums the decode can meet); the partial last
    group with a clamped row at its start and a long one at its end."""
    special = {}
    g = 2
    for L in beside_clamp:
        for off in (0, 7, 15):
            special[GROUP * g + off] = L
            g += 2
    for off in (4, 5, 9, 10, 14):
        special[GROUP * g + off] = 62
    g += 2
    for off in range(GROUP):
        special[GROUP * g + off] = 62
    g += 2
    special[GROUP * g + 3] = 63                 # one clamped row in the middle of three short ones, then a word boundary
    special[GROUP * g + 5] = 1
    assert GROUP * (g + 1) < B_ROWS - 11
    special[B_ROWS - 11] = 63                   # offset 0 of the last group
    special[B_ROWS - 1] = 700                   # its last row, offset 10
    return special


def _case(seed, beside_clamp, max_len):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, size=B_ROWS)
    special = _special_lengths(beside_clamp)
    for r, L in special.items():
        lens[r] = L
    b_rows = np.repeat(np.arange(B_ROWS), lens)
    b_rp, b_ci = gen._csr_from_pairs(b_rows, rng.integers(0, NCOLS, size=b_rows.size), B_ROWS, dedup=False)   # exact lengths
    assert np.array_equal(np.diff(b_rp), lens)
    # A looks up EVERY row of B at least once -- below, at and above each clamped row of its group, and the whole group
    # behind it -- and many of them again at random
    a_rows = np.repeat(np.arange(A_ROWS), rng.integers(0, 30, size=A_ROWS))
    a_rows = np.sort(np.concatenate([a_rows, np.arange(B_ROWS) % A_ROWS]))
    a_cols = rng.integers(0, B_ROWS, size=a_rows.size)
    a_cols[rng.permutation(a_rows.size)[:B_ROWS]] = np.arange(B_ROWS)
    a_rp, a_ci = gen._csr_from_pairs(a_rows, a_cols, A_ROWS)
    assert np.unique(a_ci).size == B_ROWS
    erp, eci = O.spgemm(a_rp, a_ci, b_rp, b_ci, NCOLS)
    # a mask that keeps about half of the product and adds columns that are not in it
    keep = rng.random(eci.size) < 0.5
    f_rows = np.concatenate([np.repeat(np.arange(A_ROWS), np.diff(erp))[keep], rng.integers(0, A_ROWS, size=5000)])
    f_cols = np.concatenate([np.asarray(eci)[keep], rng.integers(0, NCOLS, size=5000)])
    f_rp, f_ci = gen._csr_from_pairs(f_rows, f_cols, A_ROWS)
    mrp, mci = O.spgemm_masked(a_rp, a_ci, b_rp, b_ci, NCOLS, f_rp, f_ci)
    return dict(a=(a_rp, a_ci), b=(b_rp, b_ci), f=(f_rp, f_ci), c=(np.asarray(erp), np.asarray(eci)), m=(mrp, mci))


@pytest.fixture(scope="module")
def boundary_case():
    """rows of 0, 1, 62, 63, 64 and 700 entries: the last unclamped length, the clamp, just above it, far above it"""
    return _case(6161, (0, 1, 62, 63, 64, 700), 40)


@pytest.fixture(scope="module")
def padded_case():
    """the lengths where a padded row takes one more 16-entry unit (15/16/17, 47/48/49) beside the clamp; the other rows
    up to 62 long, so that units of 0 to 4 sixteenths are summed everywhere"""
    return _case(6262, (15, 16, 17, 47, 48, 49, 62, 63, 64), 63)


@pytest.fixture(scope="module", params=["upper-bound", "exact"])
def ctx(request):
    c = bspgemm.Context(0)
    c.set_flow(request.param)
    yield c
    c.close()


def _same(got, want):
    assert np.array_equal(got[0], want[0]), "row_ptr differs (first at %s)" % np.flatnonzero(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), "col_idx differs (first at %s)" % np.flatnonzero(got[1] != want[1])[:5]


def _products(ctx, case, table, padded):
    """the rectangular product, an interior row range of it and the masked product, with the table forced or forbidden"""
    ctx.set_option("blocked_extents", table)
    ctx.set_option("padded_rows", padded)
    A, B, F = ctx.upload(*case["a"], B_ROWS), ctx.upload(*case["b"], NCOLS), ctx.upload(*case["f"], NCOLS)
    out = {}
    try:
        C = ctx.multiply(A, B)
        st = ctx.stats()
        assert st["prepass_kernel"] == table and B.uses_blocked_table == table and st["padded_rows"] == padded
        out["whole"] = C.download()
        C.free()
        C = ctx.multiply(A, B, 123, 600)
        assert ctx.stats()["prepass_kernel"] == table
        out["range"] = C.download()
        C.free()
        M = ctx.multiply_masked(A, B, F)
        assert ctx.stats()["prepass_kernel"] == table
        out["masked"] = M.download()
        M.free()
    finally:
        for h in (A, B, F):
            h.free()
    return out


def _check(ctx, case, padded):
    old = ctx.get_option("blocked_extents"), ctx.get_option("padded_rows")
    try:
        got = {t: _products(ctx, case, t, padded) for t in (1, 0)}
    finally:
        ctx.set_option("blocked_extents", old[0])
        ctx.set_option("padded_rows", old[1])
    erp, eci = case["c"]
    want = {"whole": (erp, eci), "range": (erp[123:601] - erp[123], eci[erp[123]:erp[600]]), "masked": case["m"]}
    for name in want:
        _same(got[1][name], want[name])                           # against the oracle
        _same(got[1][name], got[0][name])                         # against the B.row_ptr prepass


def test_lengths_beside_the_clamp(ctx, boundary_case):
    _check(ctx, boundary_case, 0)


def test_padded_starts_beside_the_clamp(ctx, padded_case):
    """BSPGEMM_OPT_PADDED_ROWS: the table's starts count 16-entry units of the padded copy of B.col_idx"""
    _check(ctx, padded_case, 1)


def test_padded_lengths_without_padding(ctx, padded_case):
    _check(ctx, padded_case, 0)


def test_debug_check_reads_the_table():
    """BSPGEMM_OPT_CHECK verifies the table against B.row_ptr: a correct one passes; after the wrapped row_ptr is rewritten
    in place without invalidate, the stale-table error.  The rewrite moves only the boundary between two rows of more
    than 255 entries, the second of which starts a group: every clamped length stays what it was (the byte lengths of
    the other derived table too), only that group's start is stale."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6363)
    n = 2000
    lens = rng.integers(0, 70, size=n)
    lens[16 * 40 - 1], lens[16 * 40] = 300, 400
    rows = np.repeat(np.arange(n), lens)
    rp1, ci = gen._csr_from_pairs(rows, rng.integers(0, n, size=rows.size), n, dedup=False)
    rp1 = np.asarray(rp1, np.int32)
    rp2 = rp1.copy()
    rp2[16 * 40] += 100                                           # (300, 400) -> (400, 300)
    assert np.array_equal(np.minimum(np.diff(rp1), 255), np.minimum(np.diff(rp2), 255))
    d_rp = torch.from_numpy(rp1).to(dev)
    d_ci = torch.from_numpy(np.asarray(ci, np.int32)).to(dev)
    ctx = bspgemm.Context(0)
    try:
        ctx.set_option("blocked_extents", 1)
        ctx.set_option("padded_rows", 0)
        ctx.set_option("check", 1)
        A = ctx.wrap_device(n, n, int(rp1[-1]), d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci))
        C = ctx.multiply(A, A)
        st = ctx.stats()
        assert st["checked"] == 1 and st["prepass_kernel"] == 1
        _same(C.download(), O.spgemm(rp1, ci, rp1, ci, n))
        C.free()
        d_rp.copy_(torch.from_numpy(rp2))
        torch.cuda.synchronize()
        with pytest.raises(bspgemm.BspgemmError) as e:
            ctx.multiply(A, A)
        assert e.value.status == 1 and "invalidate" in str(e.value)
        A.invalidate()
        C = ctx.multiply(A, A)
        assert ctx.stats()["prepass_kernel"] == 1
        _same(C.download(), O.spgemm(rp2, ci, rp2, ci, n))
        C.free()
        A.free()
    finally:
        ctx.close()
