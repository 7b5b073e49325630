"""numpy references of the set operations on CSR patterns (bspgemm_matrix_setop, bspgemm_matrix_symmetrize): the entries
as keys row * cols + col, combined by numpy's set routines.  CSR in, sorted duplicate-free CSR out:
(row_ptr int32, col_idx int32).
"""
import numpy as np

SETOPS = {"or": np.union1d, "and": np.intersect1d, "andnot": np.setdiff1d, "xor": np.setxor1d}


def _keys(rp, ci, cols):
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    return rows * max(int(cols), 1) + np.asarray(ci, np.int64)


def _csr(keys, rows, cols):
    c = max(int(cols), 1)
    counts = np.bincount(keys // c, minlength=rows)[:rows] if rows else np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (keys % c).astype(np.int32)


def setop_ref(rpA, ciA, rpB, ciB, rows, cols, op):
    """pattern(A) op pattern(B), op in "or" | "and" | "andnot" | "xor"; the inputs' rows may be unsorted and hold repeats"""
    keys = SETOPS[op](np.unique(_keys(rpA, ciA, cols)), np.unique(_keys(rpB, ciB, cols)))
    return _csr(np.asarray(keys, np.int64), rows, cols)


def canonical_ref(rp, ci, rows, cols):
    """rows sorted, repeats dropped"""
    return setop_ref(rp, ci, rp, ci, rows, cols, "or")


def transpose_ref(rp, ci, rows, cols):
    keys = _keys(rp, ci, cols)
    c = max(int(cols), 1)
    return _csr(np.unique((keys % c) * max(rows, 1) + keys // c), cols, rows)


def symmetrize_ref(rp, ci, n, drop_diagonal=False):
    """A | A^T of an n x n pattern, without the diagonal when drop_diagonal"""
    t_rp, t_ci = transpose_ref(rp, ci, n, n)
    u_rp, u_ci = setop_ref(rp, ci, t_rp, t_ci, n, n, "or")
    if not drop_diagonal:
        return u_rp, u_ci
    d = np.arange(n, dtype=np.int32)
    return setop_ref(u_rp, u_ci, np.arange(n + 1, dtype=np.int32), d, n, n, "andnot")
