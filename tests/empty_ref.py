"""Operands without entries, for the tests of the entry points that build an operand on the device (select, the set
operations, transpose, matrix_from_result, connected components): the shapes, and what such a result has to be.  The CPU
reference of every one of them is the all-zero row_ptr; the library is never compared with itself."""
import numpy as np

SHAPES = ((0, 0), (0, 5), (5, 0), (4, 4))          # rows, cols
IDS = ["%dx%d" % s for s in SHAPES]


def csr(rows):
    """(row_ptr, col_idx) of `rows` empty rows"""
    return np.zeros(rows + 1, np.int32), np.zeros(0, np.int32)


def diagonal(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)


def gather_all(ctx, rows):
    """a 3 x rows operand whose every row holds every column: as A of a product it gathers every row of B"""
    return ctx.upload((np.arange(4) * rows).astype(np.int32), np.tile(np.arange(rows, dtype=np.int32), 3), rows)


def check(ctx, M, rows, cols):
    """M, a derived operand, is rows x cols without an entry, and works at once as B (where square: also as A) of a product"""
    assert (M.rows, M.cols, M.nnz) == (rows, cols, 0)
    rp, ci = M.download()
    assert rp.dtype == np.int32 and rp.size == rows + 1 and not rp.any() and ci.size == 0
    A = gather_all(ctx, rows)
    for X in (A, M) if rows == cols else (A,):
        P = ctx.multiply(X, M)
        prp, pci = P.download()
        assert (P.rows, P.nnz) == (X.rows, 0) and not prp.any() and pci.size == 0
        P.free()
    A.free()
