"""The scipy model of bspgemm_multiply_masked_dot, shared by the masked-dot tests.  CSR in as (row_ptr, col_idx) pairs with
explicit shapes, CSR out as (row_ptr int64, col_idx int32, values int32).

A, B and F are deduplicated (counts are taken on patterns), then C = F .* (A1 @ B1.T) with F cut to B.rows columns, zeros
eliminated and indices sorted: C_ij = |pattern(A_i) n pattern(B_j)| for (i, j) in pattern(F), j < B.rows, stored where > 0.
"""
import numpy as np
import scipy.sparse as sp


def pattern(rp, ci, rows, cols):
    """the 0/1 matrix of a CSR pattern: repeats collapsed, indices sorted"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    m = sp.csr_matrix((np.ones(ci.size, np.int64), ci, rp), shape=(rows, cols))
    m.sum_duplicates()
    m.data[:] = 1
    m.sort_indices()
    return m


def csr(rows):
    """(row_ptr int32, col_idx int32) of a list of rows, entries as given"""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.array([c for r in rows for c in r], dtype=np.int32)


def dot_ref(a, b, f, a_rows, b_rows, cols, f_cols):
    """a, b, f: (row_ptr, col_idx); A is a_rows x cols, B is b_rows x cols, F is a_rows x f_cols"""
    A1, B1 = pattern(a[0], a[1], a_rows, cols), pattern(b[0], b[1], b_rows, cols)
    F1 = pattern(f[0], f[1], a_rows, max(f_cols, b_rows, 1)).tocsc()[:, :b_rows].tocsr()
    C = F1.multiply(A1 @ B1.T).tocsr()
    C.eliminate_zeros()
    C.sort_indices()
    return C.indptr.astype(np.int64), C.indices.astype(np.int32), C.data.astype(np.int32)


def heavy_at_zero(a, b, f, a_rows, b_rows, cols, f_cols):
    """mask entries (of the deduplicated F) with j < B.rows whose two (deduplicated) rows are both non-empty: what the
    one-wave-per-entry kernel handles under dot_light = 0; and nnz of the deduplicated F"""
    la = np.diff(pattern(a[0], a[1], a_rows, cols).indptr)
    lb = np.diff(pattern(b[0], b[1], b_rows, cols).indptr)
    F1 = pattern(f[0], f[1], a_rows, max(f_cols, b_rows, 1))
    i = np.repeat(np.arange(a_rows), np.diff(F1.indptr))
    j = F1.indices.astype(np.int64)
    ok = j < b_rows
    return int(np.count_nonzero((la[i[ok]] > 0) & (lb[j[ok]] > 0))), int(F1.nnz)
