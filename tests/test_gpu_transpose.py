"""The operand transpose AT = pattern(A)^T on the device (bspgemm_matrix_transpose, Context.transpose) and the operand
read-back (bspgemm_matrix_download, Matrix.download), compared in full against a numpy reference: the unique (k, i)
pairs in lexicographic order as a CSR of A.cols rows.

Cases: every operand of the golden fixtures; rectangular and degenerate shapes; column counts at the 8-bit digit
boundaries with entries in the last column; a hub column in every row, a full row, unsorted rows with duplicates; the
operand sources (interior upload, wrapped torch tensors, a product); the involution; transposed operands in products,
masked products and the closure; out-of-range columns; the stats ring; and Graph500-skew scale 20.

The kernel edges -- tile and thread tails, the staged and unstaged row_ptr window of the first pass, duplicate runs
across threads, waves and tiles, the narrow / wide fills of empty rows -- are pinned one by one in
tests/test_gpu_transpose_edges.py, with the reference (ref_transpose) and a host model in tests/transpose_ref.py.
"""
import glob
import os

import numpy as np
import pytest

import bspgemm
import empty_ref
import gen
from oracle import oracle as O
from transpose_ref import ref_transpose

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def check(ctx, A, rp, ci, cols):
    """transpose the operand A (host CSR rp / ci, `cols` columns) and compare everything; returns AT"""
    AT = ctx.transpose(A)
    erp, eci = ref_transpose(rp, ci, cols)
    assert (AT.rows, AT.cols, AT.nnz) == (cols, A.rows, eci.size)
    grp, gci = AT.download()
    assert np.array_equal(grp, erp)
    assert np.array_equal(gci, eci)
    return AT


def _operands(path):
    """every CSR in a fixture: the pairs <x>_rp / <x>_ci, and row_ptr / col_idx"""
    d = np.load(path)
    for key in d.files:
        if key.endswith("_rp") and key[:-3] + "_ci" in d.files:
            yield key[:-3], d[key], d[key[:-3] + "_ci"]
    if "row_ptr" in d.files and "col_idx" in d.files:
        yield "csr", d["row_ptr"], d["col_idx"]


# (live_reference.npz holds digests only)
GOLDEN = [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))) if any(True for _ in _operands(p))]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_operands(ctx, path):
    seen = 0
    for name, rp, ci in _operands(path):
        rp = rp.astype(np.int32)
        ci = ci.astype(np.int32)
        cols = max(int(ci.max()) + 1 if ci.size else 0, rp.size - 1)
        A = ctx.upload(rp, ci, cols)
        check(ctx, A, rp, ci, cols)
        seen += 1
    assert seen > 0


def random_csr(rows, cols, nnz, seed, sort=False):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, rows, nnz) if rows else np.zeros(0, np.int64)
    c = rng.integers(0, cols, nnz) if cols else np.zeros(0, np.int64)
    return gen._csr_from_pairs(r, c, rows, dedup=False, sort=sort)


@pytest.mark.parametrize("rows,cols,nnz", [(20000, 37, 60000), (37, 20000, 60000), (5000, 1, 4000), (1, 5000, 3000),
                                           (0, 10, 0), (10, 0, 0), (0, 0, 0), (300, 200, 0), (4097, 4099, 9000)])
def test_shapes(ctx, rows, cols, nnz):
    rp, ci = random_csr(rows, cols, nnz, seed=rows * 7 + cols)
    A = ctx.upload(rp, ci, cols)
    AT = check(ctx, A, rp, ci, cols)
    ATT = ctx.transpose(AT)
    assert (ATT.rows, ATT.cols) == (rows, cols)


@pytest.mark.parametrize("rows,cols", empty_ref.SHAPES, ids=empty_ref.IDS)
def test_transpose_of_nothing_is_an_operand(ctx, rows, cols):
    rp, ci = empty_ref.csr(rows)
    A = ctx.upload(rp, ci, cols)
    AT = check(ctx, A, rp, ci, cols)
    empty_ref.check(ctx, AT, cols, rows)
    ATT = ctx.transpose(AT)
    empty_ref.check(ctx, ATT, rows, cols)
    for h in (ATT, AT, A):
        h.free()


@pytest.mark.parametrize("cols", [255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1])
def test_digit_boundaries(ctx, cols):
    rows = 3000
    rp, ci = random_csr(rows, cols, 20000, seed=cols)
    ci = ci.copy()
    ci[::97] = cols - 1                          # the last column, many times (and some first ones)
    ci[5::211] = 0
    A = ctx.upload(rp, ci, cols)
    check(ctx, A, rp, ci, cols)


def test_hub_column_full_row_and_duplicates(ctx):
    n = 1 << 20
    rng = np.random.default_rng(5)
    r = np.concatenate([np.arange(n), rng.integers(0, n, 3 * n)])
    c = np.concatenate([np.full(n, 12345), rng.integers(0, n, 3 * n)])
    rp, ci = gen._csr_from_pairs(r, c, n, dedup=False, sort=False)
    AT = check(ctx, ctx.upload(rp, ci, n), rp, ci, n)
    grp, _ = AT.download()
    assert grp[12346] - grp[12345] == n          # the hub row of AT holds every row of A
    m = 70000                                     # one full row of 70000 columns in a matrix of mostly empty rows
    rp = np.zeros(1001, np.int32)
    rp[501:] = m
    ci = np.arange(m, dtype=np.int32)[::-1].copy()
    check(ctx, ctx.upload(rp, ci, m), rp, ci, m)
    rp, ci, n = gen.dups_unsorted(3000, 40, seed=9)
    check(ctx, ctx.upload(rp, ci, n), rp, ci, n)


def test_operand_sources(ctx):
    import torch
    rp, ci, n = gen.rmat(12, 8, (0.57, 0.19, 0.19, 0.05), seed=3)
    r0, rows = 1000, 2000                          # interior upload: rows [1000, 3000)
    A = ctx.upload(rp, ci, n, row0=r0, rows=rows)
    sub_rp = (rp[r0:r0 + rows + 1] - rp[r0]).astype(np.int32)
    sub_ci = ci[rp[r0]:rp[r0 + rows]]
    check(ctx, A, sub_rp, sub_ci, n)
    trp = torch.from_numpy(rp).cuda()
    tci = torch.from_numpy(ci).cuda()
    W = ctx.wrap_device(n, n, ci.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, tci))
    check(ctx, W, rp, ci, n)
    B = ctx.upload(rp, ci, n)
    C = ctx.multiply(B, B)
    crp, cci = C.download()
    P = ctx.matrix_from_result(C, n)
    check(ctx, P, crp, cci, n)


def test_involution(ctx):
    rp, ci, n = gen.dups_unsorted(2000, 30, seed=4)
    A = ctx.upload(rp, ci, n)
    ATT = ctx.transpose(ctx.transpose(A))
    trp, tci = ref_transpose(rp, ci, n)
    erp, eci = ref_transpose(trp, tci, n)          # canonical A: rows sorted, duplicates dropped
    grp, gci = ATT.download()
    assert np.array_equal(grp, erp) and np.array_equal(gci, eci)


def test_transposed_operand_in_products(ctx):
    # multiply(transpose(A), B) against the oracle on host-transposed inputs (rectangular)
    a_rp, a_ci = random_csr(3000, 2000, 30000, seed=11)
    b_rp, b_ci = random_csr(3000, 2500, 30000, seed=12)
    AT = ctx.transpose(ctx.upload(a_rp, a_ci, 2000))
    B = ctx.upload(b_rp, b_ci, 2500)
    t_rp, t_ci = ref_transpose(a_rp, a_ci, 2000)
    erp, eci = O.spgemm(t_rp, t_ci, b_rp, b_ci, 2500)
    crp, cci = ctx.multiply(AT, B).download()
    assert np.array_equal(crp, erp) and np.array_equal(cci, eci)
    # (A*B)^T == B^T * A^T, bit for bit, on R-MAT scale 16
    rp, ci, n = bspgemm.gen_rmat(16, 16, (0.30, 0.25, 0.25), seed=2)
    rp2, ci2, _ = bspgemm.gen_rmat(16, 16, (0.57, 0.19, 0.19), seed=3)
    A, B = ctx.upload(rp, ci, n), ctx.upload(rp2, ci2, n)
    AB = ctx.matrix_from_result(ctx.multiply(A, B), n)
    left = ctx.transpose(AB).download()
    rrp, rci = ctx.multiply(ctx.transpose(B), ctx.transpose(A)).download()
    assert np.array_equal(left[0], rrp) and np.array_equal(left[1], rci)
    # a masked product with a transposed mask
    d = np.load(os.path.join(ROOT, "tests", "golden", "masked_n512.npz"))
    n = int(d["n"])
    A = ctx.upload(d["a_rp"], d["a_ci"], n)
    FT = ctx.transpose(ctx.upload(d["f_rp"], d["f_ci"], n))
    f_rp, f_ci = ref_transpose(d["f_rp"], d["f_ci"], n)
    erp, eci = O.spgemm_masked(d["a_rp"], d["a_ci"], d["a_rp"], d["a_ci"], n, f_rp, f_ci)
    crp, cci = ctx.multiply_masked(A, A, FT).download()
    assert np.array_equal(crp, erp) and np.array_equal(cci, eci)


def test_closure_of_transpose(ctx):
    rp, ci, n = gen.rmat(9, 2, (0.57, 0.19, 0.19, 0.05), seed=8)
    A = ctx.upload(rp, ci, n)
    T, _ = ctx.closure(A)
    trp, tci = T.download()
    TT, _ = ctx.closure(ctx.transpose(A))
    grp, gci = TT.download()
    erp, eci = ref_transpose(trp, tci, n)
    assert np.array_equal(grp, erp) and np.array_equal(gci, eci)


@pytest.mark.parametrize("bad", ["cols", "negative"])
def test_out_of_range_column(ctx, bad):
    rp, ci, n = gen.uniform(5000, 6, seed=1)
    ci = ci.copy()
    ci[len(ci) * 3 // 4] = n if bad == "cols" else -3
    A = ctx.upload(rp, ci, n)
    with pytest.raises(bspgemm.BspgemmError) as e:
        ctx.transpose(A)
    assert e.value.status == ERR_INVALID
    assert "column" in str(e.value)
    rp, ci, n = gen.uniform(2048, 8, seed=2)
    G = ctx.upload(rp, ci, n)
    crp, cci = ctx.multiply(G, G).download()        # the context is still usable
    erp, eci = O.spgemm(rp, ci, rp, ci, n)
    assert np.array_equal(crp, erp) and np.array_equal(cci, eci)


def test_stats_untouched(ctx):
    rp, ci, n = gen.uniform(4096, 8, seed=3)
    A = ctx.upload(rp, ci, n)
    ctx.multiply(A, A).free()
    ctx.multiply(A, A).free()
    before = [ctx.stats(age) for age in range(2)]
    ctx.transpose(A).free()
    after = [ctx.stats(age) for age in range(2)]
    assert before == after


def test_download_is_what_was_uploaded(ctx):
    rp, ci, n = gen.dups_unsorted(1500, 20, seed=6)
    r0, rows = 100, 900
    A = ctx.upload(rp, ci, n, row0=r0, rows=rows)
    grp, gci = A.download()
    assert np.array_equal(grp, rp[r0:r0 + rows + 1] - rp[r0])
    assert np.array_equal(gci, ci[rp[r0]:rp[r0 + rows]])
    E = ctx.upload(np.zeros(4, np.int32), np.zeros(0, np.int32), 9)
    grp, gci = E.download()
    assert np.array_equal(grp, np.zeros(4, np.int32)) and gci.size == 0


def test_graph500_skew_scale20(ctx):
    rp, ci, n = bspgemm.gen_rmat(20, 16, (0.57, 0.19, 0.19), seed=1)
    A = ctx.upload(rp, ci, n)
    check(ctx, A, rp, ci, n)
