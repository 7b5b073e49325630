"""The tests' model of bspgemm_matrix_extract (include/bspgemm.h): scipy's A[I][:, J] with sum_duplicates and sort_indices, the
predictions of every info field but `lanes` under the automatic rule, a naive model of the definition in Python sets that
cross-checks it, and the edge graphs of the GPU tests with what they claim to reach (test_extract_shapes.py checks the
claims on the host).
"""
import numpy as np
import scipy.sparse as sp

HUB_CHUNK = 4096      # csrc/kernels.hpp kExHubChunk
SORT_WAVE = 256       # kExSortWave
SORT_BLOCK = 4096     # kExSortBlock
THREADS = 256         # csrc/extract.hip kExThreads
LANES = (0, 4, 16, 64)   # BSPGEMM_OPT_EXTRACT_LANES
INFO = ("kept", "scanned", "hub_chunks", "cols_monotone", "sorted_by", "canonicalised")   # (lanes: see lanes_auto)


def _csr(rp, ci, rows, cols):
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    return sp.csr_matrix((np.ones(ci.size, np.int64), ci, rp - rp[0]), shape=(rows, cols))


def is_canonical(rp, ci):
    """every row strictly ascending"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    if ci.size < 2:
        return True
    inner = np.ones(ci.size, bool)
    inner[(rp[:-1] - rp[0])[rp[:-1] < rp[-1]]] = False        # the first entry of a row has no predecessor
    return bool(np.all((ci[1:] > ci[:-1]) | ~inner[1:]))


def canonical(rp, ci, rows, cols):
    """(row_ptr, col_idx) int32 of the sorted duplicate-free copy"""
    M = _csr(rp, ci, rows, cols)
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32)


def chunks_of(length):
    length = np.asarray(length, np.int64)
    return np.where(length > HUB_CHUNK, (length + HUB_CHUNK - 1) // HUB_CHUNK, 0)


def lanes_auto(scanned, walked):
    """the automatic lanes per out row: the smallest width at or above a quarter of the mean length of the `walked` rows read"""
    if scanned <= 16 * walked:
        return 4
    return 16 if scanned <= 64 * walked else 64


def model(rp, ci, rows, cols, I=None, J=None, keep_shape=False):
    """dict: rp, ci (int32), shape, every INFO field, and per out row the length read (`read`, 0 for a row that is not
    walked), the entries kept (`kept_rows`) and the number of rows read (`walked`: under keep_shape the distinct ones)"""
    M = _csr(rp, ci, rows, cols)
    canonicalised = 0 if is_canonical(rp, ci) else 1
    M.sum_duplicates()
    M.sort_indices()
    lens = np.diff(M.indptr).astype(np.int64)
    Iv = None if I is None else np.asarray(I, np.int64).reshape(-1)
    Jv = None if J is None else np.asarray(J, np.int64).reshape(-1)
    if keep_shape:
        rmask = np.ones(rows, bool) if Iv is None else np.isin(np.arange(rows), Iv)
        cmask = np.ones(cols, bool) if Jv is None else np.isin(np.arange(cols), Jv)
        coo = M.tocoo()
        sel = rmask[coo.row] & cmask[coo.col]
        S = sp.csr_matrix((np.ones(int(sel.sum()), np.int64), (coo.row[sel], coo.col[sel])), shape=(rows, cols))
        read = np.where(rmask, lens, 0)
        monotone = 1
    else:
        S = M if Iv is None else M[Iv]
        if Jv is not None:
            assert np.unique(Jv).size == Jv.size, "relabelling takes each column once"
            S = S[:, Jv]
        S = sp.csr_matrix(S)
        read = lens if Iv is None else lens[Iv]
        monotone = 1 if Jv is None or Jv.size < 2 or bool(np.all(Jv[1:] >= Jv[:-1])) else 0
    S.sum_duplicates()
    S.sort_indices()
    kept_rows = np.diff(S.indptr).astype(np.int64)
    kept = int(kept_rows.sum())
    sorted_by = 0
    if not monotone and kept > 0:
        sorted_by = 2 if kept_rows.max() > SORT_BLOCK else 1
    return {"rp": S.indptr.astype(np.int32), "ci": S.indices.astype(np.int32), "shape": S.shape, "kept": kept,
            "scanned": int(read.sum()), "hub_chunks": int(chunks_of(read).sum()), "cols_monotone": monotone,
            "sorted_by": sorted_by, "canonicalised": canonicalised, "read": read, "kept_rows": kept_rows,
            "walked": int(rmask.sum()) if keep_shape else int(read.size)}


def naive(rp, ci, rows, cols, I=None, J=None, keep_shape=False):
    """the definition in Python sets: (row_ptr, col_idx) as lists"""
    rp, ci = [int(x) for x in rp], [int(x) for x in ci]
    row = [set(ci[rp[r] - rp[0]:rp[r + 1] - rp[0]]) for r in range(rows)]
    I = list(range(rows)) if I is None else [int(i) for i in I]
    J = list(range(cols)) if J is None else [int(j) for j in J]
    out = []
    if keep_shape:
        si, sj = set(I), set(J)
        for i in range(rows):
            out.append(sorted(j for j in row[i] if j in sj) if i in si else [])
    else:
        for r in range(len(I)):
            out.append(sorted(c for c in range(len(J)) if J[c] in row[I[r]]))
    orp = [0]
    for x in out:
        orp.append(orp[-1] + len(x))
    return orp, [c for x in out for c in x]


def sort_class(kept_row):
    """who sorts an out row of that many entries: 0 nobody, 1 a wave, 2 a workgroup, 3 the two-transpose fallback"""
    if kept_row < 2:
        return 0
    return 1 if kept_row <= SORT_WAVE else (2 if kept_row <= SORT_BLOCK else 3)


# ---------------------------------------------------------------- the edge graphs ------------------------------------
def _rows_to_csr(rows_cols):
    rp = np.zeros(len(rows_cols) + 1, np.int64)
    rp[1:] = np.cumsum([len(x) for x in rows_cols])
    ci = np.concatenate([np.asarray(x, np.int64) for x in rows_cols] + [np.zeros(0, np.int64)])
    return rp.astype(np.int32), ci.astype(np.int32)


LANE_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65)       # 0, 1, W - 1, W, W + 1 for W = 4, 16, 64
LANE_PATTERNS = ("none", "all", "first", "last", "alternating")
LANE_NI = 70          # 70 W threads: the last workgroup has idle waves and, for W < 64, a wave with idle groups
LANE_COLS = 2 * 65


def lane_case():
    """(rp, ci, rows, cols, I, J): every LANE_LENGTHS x LANE_PATTERNS row; entry k of a row is column 2k when it is kept and
    2k + 1 when it is not, J the even columns, I every row and then the first LANE_NI - 55 rows of 65 entries again"""
    rows_cols = []
    for n in LANE_LENGTHS:
        for p in LANE_PATTERNS:
            k = np.arange(n)
            keep = {"none": k < 0, "all": k >= 0, "first": k == 0, "last": k == n - 1, "alternating": k % 2 == 0}[p]
            rows_cols.append(2 * k + np.where(keep, 0, 1))
    rp, ci = _rows_to_csr(rows_cols)
    nrows = len(rows_cols)
    I = np.concatenate([np.arange(nrows), nrows - 1 - np.arange(LANE_NI - nrows)]).astype(np.int32)
    J = np.arange(0, LANE_COLS, 2, dtype=np.int32)
    return rp, ci, nrows, LANE_COLS, I, J


HUB_COLS = 20500
HUB_ROWS = {"len4096": 0, "len4097": 1, "len8192": 2, "len8193": 3, "nothing_kept": 4, "empty_middle_chunk": 5, "short": 6,
            "last_hub": 7}


def hub_case():
    """(rp, ci, rows, cols, I, J).  Rows 0 .. 3: 4096 (no hub), 4097, 8192 and 2 * 4096 + 1 entries, column = position.  J:
    the even columns and the runs [4090, 4102) and [8186, 8200), which straddle the chunk borders.  Row 4: a hub of odd
    columns outside the runs (nothing kept).  Row 5: three chunks, the middle one odd columns (empty).  Row 6: short.  Row 7,
    the last: a hub.  I names row 3 twice and ends with the hub."""
    odd = 8201 + 2 * np.arange(4097)
    rows_cols = [np.arange(4096), np.arange(4097), np.arange(8192), np.arange(8193), odd,
                 np.concatenate([np.arange(4096), odd[:4096], 16392 + np.arange(4096)]), np.array([3, 4091, 9000]),
                 np.arange(100, 100 + 5000)]
    rp, ci = _rows_to_csr(rows_cols)
    J = np.union1d(np.arange(0, HUB_COLS, 2), np.concatenate([np.arange(4090, 4102), np.arange(8186, 8200)])).astype(np.int32)
    I = np.array([0, 1, 2, 3, 4, 5, 6, 3, 7], np.int32)
    return rp, ci, len(rows_cols), HUB_COLS, I, J


SORT_KEPT = (1, 2, 255, 256, 257, 4095, 4096)
SORT_COLS = 5000


def sort_case(fallback=False, seed=5):
    """(rp, ci, rows, cols): rows of SORT_KEPT entries (with fallback one of 4097 more), random distinct columns of SORT_COLS;
    a J that is a permutation of all columns keeps every entry"""
    rng = np.random.default_rng(seed)
    lens = SORT_KEPT + ((SORT_BLOCK + 1,) if fallback else ())
    rows_cols = [np.sort(rng.choice(SORT_COLS, n, replace=False)) for n in lens]
    rp, ci = _rows_to_csr(rows_cols)
    return rp, ci, len(lens), SORT_COLS
