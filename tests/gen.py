"""Seeded numpy generators of small boolean CSR matrices for the tests and golden vectors.
(The product's own C generators live in binary-spgemm_amd/host/csr_gen.c and are tested
separately; these are independent so a generator bug cannot hide behind itself.)

All return int32 arrays: (row_ptr[n+1], col_idx[nnz], n) unless stated.
"""
import numpy as np


def _csr_from_pairs(rows, cols, n, dedup=True, sort=True):
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    if dedup:
        key = np.unique(rows * (1 << 32) + cols)
        rows, cols = key >> 32, key & 0xFFFFFFFF
    elif sort:
        o = np.lexsort((cols, rows))
        rows, cols = rows[o], cols[o]
    else:
        o = np.argsort(rows, kind="stable")
        rows, cols = rows[o], cols[o]
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp)
    return rp.astype(np.int32), cols.astype(np.int32)


def uniform(n, d, seed):
    """each row draws d columns i.i.d. uniform in [0,n); duplicates collapsed (SURVEY 8d cfg 2)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), d)
    cols = rng.integers(0, n, size=n * d)
    rp, ci = _csr_from_pairs(rows, cols, n)
    return rp, ci, n


def uniform_rect(nr, nc, d, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(nr), d)
    cols = rng.integers(0, nc, size=nr * d)
    return _csr_from_pairs(rows, cols, nr)


def rmat(scale, ef, abcd, seed):
    """R-MAT, no vertex permutation, directed, duplicates collapsed (SURVEY 8d cfg 3)"""
    rng = np.random.default_rng(seed)
    n = 1 << scale
    m = n * ef
    a, b, c, _ = abcd
    rows = np.zeros(m, dtype=np.int64)
    cols = np.zeros(m, dtype=np.int64)
    for _lvl in range(scale):
        r = rng.random(m)
        right = ((r >= a) & (r < a + b)) | (r >= a + b + c)
        down = r >= a + b
        rows = (rows << 1) | down
        cols = (cols << 1) | right
    rp, ci = _csr_from_pairs(rows, cols, n)
    return rp, ci, n


def with_special_rows(n, d, seed):
    """uniform, but a third of the rows empty, row 7 completely full, row n-1 with one entry"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), d)
    cols = rng.integers(0, n, size=n * d)
    keep = (rows % 3 != 0) & (rows != 7) & (rows != n - 1)
    rows, cols = rows[keep], cols[keep]
    rows = np.concatenate([rows, np.full(n, 7), [n - 1]])
    cols = np.concatenate([cols, np.arange(n), [n - 1]])
    rp, ci = _csr_from_pairs(rows, cols, n)
    return rp, ci, n


def dups_unsorted(n, d, seed):
    """rows keep duplicate entries and are NOT sorted (readCOO keeps duplicates)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), d)
    cols = rng.integers(0, max(n // 8, 1), size=n * d)      # narrow range -> many duplicates
    rp, ci = _csr_from_pairs(rows, cols, n, dedup=False, sort=False)
    return rp, ci, n


def banded(n, half, seed):
    """band matrix with random holes: products collide heavily inside 64-column words"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for off in range(-half, half + 1):
        r = np.arange(max(0, -off), min(n, n - off))
        keep = rng.random(r.size) < 0.8
        rows.append(r[keep])
        cols.append(r[keep] + off)
    rp, ci = _csr_from_pairs(np.concatenate(rows), np.concatenate(cols), n)
    return rp, ci, n


def powerlaw(n, mean_deg, seed, alpha=2.1, max_deg=None):
    """out-degrees Pareto(alpha) clipped to [1,max_deg] rescaled to mean_deg; columns drawn from
    the same skewed distribution (SURVEY 8d cfg 5)"""
    rng = np.random.default_rng(seed)
    max_deg = max_deg or max(n // 16, 1)
    w = (1.0 - rng.random(n)) ** (-1.0 / (alpha - 1.0))
    deg = np.clip(w * mean_deg / w.mean(), 1, max_deg).astype(np.int64)
    rows = np.repeat(np.arange(n), deg)
    p = w / w.sum()
    cols = rng.choice(n, size=rows.size, p=p)
    rp, ci = _csr_from_pairs(rows, cols, n)
    return rp, ci, n


# ---- shapes shared by test_gpu_parity.py and test_gpu_knobs.py: (a_rp, a_ci, b_rp, b_ci) ----------------------------
def tiny_b_heavy(nnzb, b_cols=(7, 0, 10, 3, 4), nrep=5000):
    """a 3 x 11 B of `nnzb` nonzeros (rows {c0}, {c1, c2}, {c3, c4} cut to the first nnzb) under a 2 x 3 A whose row 0 has
    `nrep` repeated entries (a heavy row once B has two nonzeros) and whose row 1 draws every B row once"""
    b_rows = [0, 1, 1, 2, 2][:nnzb]
    b_rp, b_ci = _csr_from_pairs(b_rows, list(b_cols)[:nnzb], 3)
    rng = np.random.default_rng(900 + nnzb)
    a_rows = np.concatenate([np.zeros(nrep, np.int64), np.ones(3, np.int64)])
    a_cols = np.concatenate([rng.integers(0, 3, size=nrep), [0, 1, 2]])
    a_rp, a_ci = _csr_from_pairs(a_rows, a_cols, 2, dedup=False)
    return a_rp, a_ci, b_rp, b_ci


WAVE_CAPS = [64 * c for c in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32)]   # csrc/kernels.hpp kWaveChunks


def class_boundary_rows(repeat=4, seed=301, n=6000):
    """n x n A and B whose A rows have F_i just below / at / above each wave class cap (WAVE_CAPS), 1, 2 and heavy rows of
    3000 .. 600000 products, every target `repeat` times.  B row j has (j % 97) + 1 entries; A rows keep repeated columns
    (a 6000-column A row could not reach 600000 products without them)."""
    rng = np.random.default_rng(seed)
    b_rows = np.repeat(np.arange(n), (np.arange(n) % 97) + 1)
    b_cols = rng.integers(0, n, size=b_rows.size)
    b_rp, b_ci = _csr_from_pairs(b_rows, b_cols, n)
    blen = np.diff(b_rp)
    targets = ([1, 2] + [t for cap in WAVE_CAPS for t in (cap - 1, cap, cap + 1)] + [3000, 4000, 100000, 280000, 600000]) * repeat
    a_rows, a_cols = [], []
    for i, t in enumerate(targets):
        acc = 0
        while acc < t:
            j = int(rng.integers(0, n))
            if acc + blen[j] <= t + 3:
                a_rows.append(i)
                a_cols.append(j)
                acc += blen[j]
    a_rp, a_ci = _csr_from_pairs(a_rows, a_cols, n, dedup=False)
    return a_rp, a_ci, b_rp, b_ci


def rank_rows(ncols, targets, short_rows=(), ones_rows=(), seed=0, counts=(6000, 2000, 1000)):
    """B of sum(counts) rows over `ncols` columns: counts[0] rows of 1-3 entries, counts[1] of 4-199, counts[2] of 200-1499,
    as dense clusters, tails that include the last column, runs around 2^20-column span boundaries and scattered columns.
    A row i has exactly targets[i] products, drawn from the longer B rows -- from the 1-3-entry rows for i in `short_rows`
    (masked quads), from the one-entry rows for i in `ones_rows` (as many sources as products) -- with repeated entries."""
    rng = np.random.default_rng(seed)
    nb = int(sum(counts))
    lens = np.concatenate([rng.integers(1, 4, counts[0]), rng.integers(4, 200, counts[1]), rng.integers(200, 1500, counts[2])])
    rows, cols = [], []
    for j, L in enumerate(lens):
        kind = j % 4
        if kind == 0:      # a dense cluster somewhere (consecutive columns: whole slots and top words)
            c0 = int(rng.integers(0, ncols - L))
            c = np.arange(c0, c0 + L)
        elif kind == 1:    # the tail of the column range, including the last column
            c = ncols - 1 - rng.choice(min(ncols, 4 * L + 8), size=L, replace=False)
        elif kind == 2 and ncols > (1 << 20):   # around a span boundary
            c = (1 << 20) * int(rng.integers(1, (ncols >> 20) + 1)) - 2 * L + rng.choice(4 * L, size=L, replace=False)
            c = c[c < ncols]
            c = np.concatenate([c, rng.choice(1000, size=L - c.size, replace=False)]) if c.size < L else c
        else:
            c = rng.permutation(np.unique(rng.integers(0, ncols, size=2 * L)))[:L] if ncols > (1 << 21) else rng.choice(ncols, size=L, replace=False)
            c = np.concatenate([c, ncols - 1 - np.arange(L - c.size)]) if c.size < L else rng.permutation(c)
        rows.append(np.full(L, j)); cols.append(c)
    b_rp, b_ci = _csr_from_pairs(np.concatenate(rows), np.concatenate(cols), nb)
    blen = np.diff(b_rp)
    short = np.flatnonzero(blen <= 3); longer = np.flatnonzero(blen > 3)
    ones = np.flatnonzero(blen == 1)
    a_rows, a_cols = [], []
    for i, t in enumerate(targets):
        acc = 0
        pool = ones if i in ones_rows else short if i in short_rows else longer
        while acc < t:
            j = int(pool[rng.integers(0, pool.size)])
            if acc + blen[j] <= t:
                a_rows.append(i); a_cols.append(j); acc += blen[j]
            elif t - acc <= 3:
                j = int(short[np.flatnonzero(blen[short] == t - acc)[0]])
                a_rows.append(i); a_cols.append(j); acc += blen[j]
    a_rp, a_ci = _csr_from_pairs(a_rows, a_cols, len(targets), dedup=False)
    return a_rp, a_ci, b_rp, b_ci
