"""numpy / scipy references shared by the select, triangle-count and k-truss tests (test_select_abi.py checks them
against networkx where it is installed).  CSR in, CSR out: (row_ptr int32, col_idx int32).
"""
import numpy as np
import scipy.sparse as sp

SELECT_KEEP = {"tril": lambda r, c: c < r, "triu": lambda r, c: c > r, "offdiag": lambda r, c: c != r}
COMPARE = {">=": np.greater_equal, ">": np.greater, "<=": np.less_equal, "<": np.less, "==": np.equal, "!=": np.not_equal}


def _rows_of(rp):
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


def _filter(rp, ci, keep):
    """the kept entries in their stored order, and the row_ptr that goes with them"""
    rows = _rows_of(rp)
    n = np.asarray(rp).size - 1
    counts = np.bincount(rows[keep], minlength=n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), np.asarray(ci, np.int32)[keep]


def select_ref(rp, ci, op):
    """the entries (r, c) with c < r ("tril"), c > r ("triu"), c != r ("offdiag"): a stable filter, repeats kept"""
    return _filter(rp, ci, SELECT_KEEP[op](_rows_of(rp), np.asarray(ci, np.int64)))


def where_ref(rp, ci, values, cmp, threshold):
    """the pattern of the entries whose value satisfies `value cmp threshold`"""
    return _filter(rp, ci, COMPARE[cmp](np.asarray(values, np.int64), int(threshold)))


def dedup_ref(rp, ci, n):
    """rows sorted, repeats dropped"""
    key = np.unique((_rows_of(rp) << 32) | np.asarray(ci, np.int64))
    counts = np.bincount(key >> 32, minlength=n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)


def _ones(rp, ci, n):
    return sp.csr_matrix((np.ones(np.asarray(ci).size, np.int64), np.asarray(ci), np.asarray(rp)), shape=(n, n))


def triangles_ref(rp, ci, n):
    """sum(L .* (L*L)) for L = the strictly lower triangle, repeats counted once"""
    L = _ones(*dedup_ref(*select_ref(rp, ci, "tril"), n), n)
    return int((L @ L).multiply(L).sum())


def ktruss_ref(rp, ci, n, k, max_iter=0):
    """The k-truss iteration as include/bspgemm.h states it: S0 = A off its diagonal, deduplicated; a step keeps the
    entries of S .* (S*S) with a count of k - 2 or more; stop when a step removes nothing or leaves nothing (converged),
    or after max_iter steps (max_iter > 0, not converged).  Returns ((row_ptr, col_idx), iterations, converged)."""
    s_rp, s_ci = dedup_ref(*select_ref(rp, ci, "offdiag"), n)
    if k == 2:
        return (s_rp, s_ci), 0, True
    it = 0
    while True:
        S = _ones(s_rp, s_ci, n)
        C = (S @ S).multiply(S).tocsr()
        C.eliminate_zeros()
        C.sort_indices()
        it += 1
        n_rp, n_ci = where_ref(C.indptr, C.indices, C.data, ">=", k - 2)
        done = n_ci.size == s_ci.size or n_ci.size == 0
        s_rp, s_ci = n_rp, n_ci
        if done:
            return (s_rp, s_ci), it, True
        if max_iter > 0 and it >= max_iter:
            return (s_rp, s_ci), it, False


def symmetrise(rp, ci, n):
    """the undirected simple graph of a pattern: both directions, no diagonal, no repeats"""
    rows = _rows_of(rp)
    ci = np.asarray(ci, np.int64)
    r, c = np.concatenate([rows, ci]), np.concatenate([ci, rows])
    off = r != c
    key = np.unique((r[off] << 32) | c[off])
    counts = np.bincount(key >> 32, minlength=n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)
