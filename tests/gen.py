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


WAVE_CHUNKS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32)   # csrc/kernels.hpp kWaveChunks
WAVE_CAPS = [64 * c for c in WAVE_CHUNKS]


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


# ---- capacity classes and the one-wave kernel's launch decisions (csrc/prepass.hip, csrc/wave_rows*.{hip,inc}) ------
NUM_BINS, RANK_BIN, MID_BIN, DENSE_BIN = 20, 17, 18, 19
SPREAD_WAVES = 256 * 8          # launch_cfg kSpreadWaves: a class is spread over at least this many waves
MAX_AMBIGUOUS = 12              # kMaxAmbiguous: the count pass's hash filter settles rows with at most this many
COMPACT_GRAN = 4096             # kCompactGran = kCompactChunkTable: outputs per chunk of the compaction's table path
COMPACT_SPARSE_ROWS = 4096      # kCompactSparseRows: a chunk spanning more rows is searched per output


def row_products(a_rp, a_ci, b_rp, r0, r1):
    """F_i of rows [r0, r1)"""
    per = np.diff(np.asarray(b_rp, np.int64))[np.asarray(a_ci, np.int64)]
    cs = np.concatenate([[0], np.cumsum(per)])
    a_rp = np.asarray(a_rp, np.int64)
    return cs[a_rp[r0 + 1:r1 + 1]] - cs[a_rp[r0:r1]]


def _mid_rank_caps(cols):
    passes = (cols + (1 << 18) - 1) >> 18
    mid_cap = 524288 if passes <= 1 else max(2048, 524288 // passes)
    rank_cap = 6144 if (1 << 18) < cols <= (1 << 24) else 0
    return mid_cap, rank_cap


def row_bins(F, cols):
    """capacity class of every row as csrc/prepass.hip bin_of places it (BSPGEMM_RANK_ROWS at its default)"""
    mid_cap, rank_cap = _mid_rank_caps(cols)
    F = np.asarray(F, np.int64)
    b = np.zeros(F.size, np.int64)
    wave = (F > 0) & (F <= 2048)
    b[wave] = 1 + np.searchsorted(np.array(WAVE_CAPS[:-1]), F[wave], side="left")
    heavy = F > 2048
    b[heavy] = np.where(F[heavy] <= rank_cap, RANK_BIN, np.where(F[heavy] > mid_cap, DENSE_BIN, MID_BIN))
    return b


def expected_bins(F, cols):
    """rows per capacity class (bspgemm_stats.rows_per_bin)"""
    return np.bincount(row_bins(F, cols), minlength=NUM_BINS).tolist()


def expected_bin_caps(cols):
    """bspgemm_stats.bin_cap (csrc/context.hip)"""
    mid_cap, rank_cap = _mid_rank_caps(cols)
    return [0] + WAVE_CAPS + [max(rank_cap, 2048), mid_cap, 0x7fffffff]


def wave_levels(cols):
    """5-bit levels of k_wave_rows for `cols` columns (csrc/kernels.hpp wave_levels_for_cols)"""
    L = next((lv for lv in range(1, 5) if cols <= 256 << (5 * lv)), 5)
    return 3 if L == 4 and cols <= 512 << 15 else L


def wave_top_words(cols):
    """TWP, the top-bitmap words per lane of the k_wave_rows instance (csrc/wave_rows.inc launch_one)"""
    topw = -(-cols // (1 << (5 * wave_levels(cols))))
    return 2 if topw <= 128 else 4 if topw <= 256 else 8


def wave_rpw(n, chunks):
    """rows per wave of a class of n rows (launch_cfg): spread over SPREAD_WAVES waves, capped at 16 (8 from 16 chunks)"""
    return max(1, min(-(-n // SPREAD_WAVES), 8 if chunks >= 16 else 16))


def wave_hash_bits(chunks):
    """HB of the count pass's hash filter: floor_log2(32 * SLOTS), SLOTS = 64 * SW"""
    sw = chunks if chunks <= 2 else (chunks + 3) & ~3
    return (32 * 64 * sw).bit_length() - 1


def wave_hash(c, hb):
    c = np.asarray(c, np.int64)
    return (c ^ (c >> hb) ^ ((c >> (2 * hb)) if 2 * hb < 32 else 0)) & ((1 << hb) - 1)


def wave_filters(cols, chunks):
    """the count instance runs the hash filter (exact flow): LEVELS >= 2 and CHUNKS <= 16"""
    return wave_levels(cols) >= 2 and chunks <= 16


def _seg_ids(lengths):
    return np.repeat(np.arange(lengths.size), lengths)


def _first_of_runs(sorted_keys):
    new = np.ones(sorted_keys.size, bool)
    new[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return new


def wave_model(a_rp, a_ci, b_rp, b_ci, cols, r0=0, r1=None, products=True, stride=1):
    """What k_wave_rows decides, from A and B only, for the product over rows [r0, r1).
    Per row: F, class, alen, the source structure of the gather plan; with `products` also |C_i|, the level-0 slots
    (nslots0), the count filter's ambiguous products (per hash value: multiplicity - 1) and the repeat/collision
    patterns the filter has to settle -- for the rows i % stride == 0 (`analysed`; the others read as without them).
    Per class: rows, rpw, waves, size of the last wave."""
    a_rp = np.asarray(a_rp, np.int64)
    b_rp = np.asarray(b_rp, np.int64)
    r1 = a_rp.size - 1 if r1 is None else r1
    R = r1 - r0
    lo, hi = int(a_rp[r0]), int(a_rp[r1])
    aci = np.asarray(a_ci[lo:hi], np.int64)
    alen = np.diff(a_rp[r0:r1 + 1])
    arow = _seg_ids(alen)
    L = (b_rp[1:] - b_rp[:-1])[aci]
    F = np.bincount(arow, weights=L, minlength=R).astype(np.int64)
    bins = row_bins(F, cols)
    chunks = np.array((0,) + WAVE_CHUNKS + (0, 0, 0))[bins]
    m = dict(R=R, F=F, bins=bins, alen=alen, levels=wave_levels(cols), twp=wave_top_words(cols), cols=cols)
    # ---- per class: the launch
    cls = {}
    for b in range(1, 17):
        n = int((bins == b).sum())
        rpw = wave_rpw(n, WAVE_CHUNKS[b - 1])
        waves = -(-n // rpw)
        cls[b] = dict(n=n, rpw=rpw, waves=waves, last=n - (waves - 1) * rpw if n else 0)
    m["classes"] = cls
    # ---- gather plan: offset of every source in its row
    cs = np.cumsum(L)
    row_start = np.concatenate([[0], np.cumsum(F)])
    off = cs - L - row_start[arow]
    nz = L > 0
    nz_cum = np.cumsum(nz)
    row_nz0 = np.concatenate([[0], nz_cum])[a_rp[r0:r1] - lo]          # nonzero sources before the row
    before = nz_cum - nz - row_nz0[arow]
    after = np.bincount(arow, weights=nz, minlength=R).astype(np.int64)[arow] - before - nz
    nch = -(-F // 64)
    m["multi_trip"] = (alen > 64) & (F > 0)
    m["zero_between"] = np.bincount(arow, weights=(~nz) & (before > 0) & (after > 0), minlength=R) > 0
    m["starts_on_chunk"] = np.bincount(arow, weights=nz & (off > 0) & (off % 64 == 0), minlength=R) > 0
    m["spans_all"] = np.bincount(arow, weights=nz & (off < 64) & (off + L > 64 * (nch[arow] - 1)), minlength=R) > 0
    ones = L == 1
    key = arow[ones] * 64 + off[ones] // 64                               # (row, chunk) of the one-entry sources
    u, cnt = np.unique(key, return_counts=True)
    m["ones_chunk"] = np.zeros(R, bool)
    m["ones_chunk"][u[cnt == 64] // 64] = True
    if not products:
        return m
    # ---- products, in the kernel's order (row, then source, then position in the B row); rows % stride == 0 only
    keep = (np.arange(R) % stride == 0)[arow]
    Ls, arow_s = L[keep], arow[keep]
    cs = np.cumsum(Ls)
    tot = int(cs[-1]) if cs.size else 0
    start = np.repeat(cs - Ls, Ls)
    src = np.repeat(b_rp[:-1][aci[keep]], Ls) - start + np.arange(tot)
    pc = np.asarray(b_ci, np.int64)[src]
    chunk = (np.repeat(off[keep], Ls) - start + np.arange(tot)) // 64
    prow = np.repeat(arow_s, Ls)
    del src, start
    m["analysed"] = np.arange(R) % stride == 0
    # distinct columns and level-0 slots per row
    kc = np.sort((prow << 32) | pc)
    first = _first_of_runs(kc)
    ucol = kc[first]
    run = np.diff(np.append(np.flatnonzero(first), kc.size))            # copies of each (row, column)
    urow = ucol >> 32
    m["nnz_row"] = np.bincount(urow, minlength=R)
    ccol = ucol & 0xFFFFFFFF
    m["dup3"] = np.bincount(urow, weights=run >= 3, minlength=R) > 0
    m["col0"] = np.bincount(urow, weights=ccol == 0, minlength=R) > 0
    m["col_last"] = np.bincount(urow, weights=ccol == cols - 1, minlength=R) > 0
    ks = (urow << 32) | (ccol >> 5)
    fs = _first_of_runs(ks)
    srun = np.diff(np.append(np.flatnonzero(fs), ks.size))
    m["nslots0"] = np.bincount(urow[fs], minlength=R)
    m["full_slot"] = np.bincount(urow[fs], weights=srun == 32, minlength=R) > 0
    del kc, first, ks, fs
    # the hash filter: ambiguous products per row, at the row's class's HB
    hb_of_bin = np.array([11] + [wave_hash_bits(c) for c in WAVE_CHUNKS] + [11, 11, 11])
    hb = hb_of_bin[bins][prow]
    h = (pc ^ (pc >> hb) ^ (pc >> (2 * hb))) & ((1 << hb) - 1)          # (int64: >> 32 of a column is 0)
    kh = np.sort((prow << 32) | h)
    fh = _first_of_runs(kh)
    m["ambiguous"] = np.where(m["analysed"], F - np.bincount(kh[fh] >> 32, minlength=R), -1)
    hrun = np.diff(np.append(np.flatnonzero(fh), kh.size))
    shared = np.repeat(hrun > 1, hrun)                                  # (row, hash) groups of 2+ products
    shared_keys = kh[shared]
    del kh, fh
    # the repeat / collision patterns, on the products whose hash is shared
    sel = np.isin((prow << 32) | h, shared_keys)
    sr, sh, sc, sk = prow[sel], h[sel], pc[sel], chunk[sel]
    o = np.lexsort((sk, sc, sh, sr))
    sr, sh, sc, sk = sr[o], sh[o], sc[o], sk[o]
    g = (sr << 32) | sh                                                 # (row, hash) group
    gc_first = _first_of_runs(g)
    gc_first[1:] |= sc[1:] != sc[:-1]
    gid = np.cumsum(_first_of_runs(g)) - 1
    cid = np.cumsum(gc_first) - 1                                       # (row, hash, column) group
    ncols_g = np.bincount(gid, weights=gc_first).astype(np.int64)
    collide = ncols_g >= 2
    m["collision"] = np.zeros(R, bool)
    m["collision"][(g[_first_of_runs(g)] >> 32)[collide]] = True
    cmin = sk[gc_first]                                                 # chunks sorted within (row, hash, column)
    cmax = np.maximum.reduceat(sk, np.flatnonzero(gc_first)) if sk.size else sk
    gmin = np.minimum.reduceat(cmin, np.flatnonzero(_first_of_runs(gid[gc_first]))) if cmin.size else cmin
    cg = gid[gc_first]
    crow = sr[gc_first]
    # a column first seen after a DIFFERENT column set its hash bit, and repeated in a later chunk: every copy is ambiguous
    late = (cmin > gmin[cg]) & (cmax > cmin)
    m["late_repeat"] = np.bincount(crow, weights=late, minlength=R) > 0
    m["repeat_across"] = np.bincount(crow, weights=cmax > cmin, minlength=R) > 0
    same = np.zeros(sk.size, bool)
    same[1:] = (cid[1:] == cid[:-1]) & (sk[1:] == sk[:-1])
    m["repeat_within"] = np.bincount(sr, weights=same, minlength=R) > 0
    return m


# ---- a generator that drives k_wave_rows into its edges: wave_rows_case -------------------------------------------------
WAVE_KINDS = ("sparse", "pair", "full", "dups", "amb0", "amb12", "amb13")   # column content of a row
WAVE_SPLITS = ("many", "ones64", "edge", "span", "mixed")                    # how the row's products split into B rows
_KIND_MIN_F = {"pair": 2, "amb0": 1, "amb12": 32, "amb13": 32}


def _strata(rng, n, k, lo, hi):
    """k distinct values per row in [lo, hi) (hi - lo >= k), one from each of k equal strata, ascending"""
    e = lo + (np.arange(k + 1, dtype=np.int64) * (hi - lo)) // k
    return e[:-1] + (rng.random((n, k)) * np.diff(e)).astype(np.int64)


def _scramble(rng, x):
    """the same random permutation of every row's positions, each row rotated by its own amount"""
    n, F = x.shape
    idx = (rng.permutation(F)[None, :] + rng.integers(0, F, size=(n, 1))) % F
    return np.take_along_axis(x, idx, 1)


def _hash_col(h, q, hb):
    """the column (q << hb) | low whose wave_hash is h"""
    m = (1 << hb) - 1
    return (q << hb) | ((h ^ (q & m) ^ (q >> hb)) & m)


def _amb_rows(rng, n, F, k, cols, hb):
    """n rows of F products with exactly k ambiguous ones: F - k products of distinct hashes, then k that repeat a hash.
    Among them: a column x whose hash a different column y set in an earlier chunk, x repeated in a later chunk (both
    copies ambiguous, only 'ambiguous and earlier' counts the repeat); a column three times, in one chunk and in the last;
    the others alternate true repeats and collisions of distinct columns.  Returns (columns, |C_i|)."""
    Q = max(1, cols >> hb)                          # high parts available: collisions need two of them
    extras = []                                     # (position, referenced position, 'dup' | 'col')
    if k:
        y, x1, x2 = (0, 64, 128) if F > 128 else (0, 1, 64) if F > 64 else (0, 1, 2)
        z2 = F - 1 if F - 1 != x2 else F - 2
        extras = [(x1, y, "col"), (x2, x1, "dup"), (4, 3, "dup"), (z2, 3, "dup")]
        used = {0, 1, 2, 3, 4, x1, x2, z2}
        pos, ref = F - 2, 5
        for e in range(k - 4):
            while pos in used:
                pos -= 1
            extras.append((pos, ref, "col" if e % 2 == 0 else "dup"))
            used |= {pos, ref}
            pos, ref = pos - 1, ref + 1
    out = np.zeros((n, F), np.int64)
    ex_pos = {p for p, _, _ in extras}
    base = np.array([p for p in range(F) if p not in ex_pos])
    H = min(1 << hb, cols)
    h = _strata(rng, n, base.size, 0, H)[:, rng.permutation(base.size)]
    q = rng.integers(0, Q, size=h.shape) if Q > 1 else np.zeros_like(h)
    out[:, base] = _hash_col(h, q, hb)
    dups = 0
    for p, r, kind in extras:
        if kind == "col" and Q > 1:
            hr = wave_hash(out[:, r], hb)
            qr = out[:, r] >> hb
            out[:, p] = _hash_col(hr, (qr + 1 + rng.integers(0, Q - 1, size=n)) % Q, hb)
        else:
            out[:, p] = out[:, r]
            dups += 1
    return out, F - dups


def _content(rng, kind, n, F, cols, levels, hb):
    """n rows x F product columns of one kind, and |C_i|"""
    nslots = -(-cols // 32)
    if kind in ("sparse", "pair"):
        if levels >= 2:                                 # every product alone in its 32-column slot
            c = np.minimum(_strata(rng, n, F, 0, nslots) * 32 + rng.integers(0, 32, size=(n, F)), cols - 1)
        else:
            c = _strata(rng, n, F, 0, cols)
        c[::2, 0], c[::2, F - 1] = 0, cols - 1          # column 0 and the last column
        if kind == "pair" and levels >= 2:              # two distinct columns share one slot: F - 1 slots
            c[:, F - 1 - F // 3] = c[:, F // 3] ^ 1
        return _scramble(rng, c), F
    if kind == "full":                                  # whole 32-column slots
        s = _strata(rng, n, -(-F // 32), 0, cols // 32)
        c = (s[:, :, None] * 32 + np.arange(32)).reshape(n, -1)[:, :F]
        return _scramble(rng, c), F
    if kind == "dups":                                  # every column about three times
        u = max(1, (F + 2) // 3)
        c = _strata(rng, n, u, 0, cols)[:, np.arange(F) % u]
        return _scramble(rng, c), u
    return _amb_rows(rng, n, F, int(kind[3:]), cols, hb)


def _split(rng, kind, F):
    """source lengths (B rows, 0 = an empty B row) of a row of F products"""
    if kind == "many":                                  # more than 64 A-nonzeros: extents loaded in several trips
        n1 = min(F, 60)
        seq = [x for i in range(n1) for x in ((1, 0) if i % 2 else (1,))]
        pad = [0] * max(0, 70 - len(seq))
        return seq[:len(seq) // 2] + pad + seq[len(seq) // 2:] + ([F - n1] if F > n1 else [])
    if kind == "ones64":                                # a chunk of 64 one-entry sources
        if F < 64:
            return [1] * F
        c = (F // 64) // 2
        return ([64 * c] if c else []) + [1] * 64 + ([F - 64 * (c + 1)] if F > 64 * (c + 1) else [])
    if kind == "edge":                                  # sources (and an empty one) starting on chunk boundaries
        cuts = sorted(set(range(64, F, 64)) | ({min(17, F - 1), F // 2} if F > 1 else set()))
        L = list(np.diff([0] + cuts + [F]))
        return L[:1] + [0] + L[1:] if F > 64 else L
    if kind == "span":                                  # one source over every chunk of the row
        return [1, F - 1] if F > 1 else [F]
    L = []                                              # "mixed": natural lengths, empty rows among them
    while sum(L) < F:
        L.append(min(int(rng.integers(0, 98)), F - sum(L)))
    return L


def _tail_rows():
    """rows laid out from output 0 for the compaction's table path, as (F, |C_i|) -- (0, 0) empty, (0, -1) A-nonzeros on
    empty B rows.  Chunks of 4096 outputs: 0 one shift; 1 a hole inside, ends with a hole row whose last output is 8191;
    2 one shift, its last row a hole row whose last output is 12288; 3 starts in that row, a hole inside, more than 4096
    rows (mostly empty): searched per output"""
    r = [(64, 64)] * 64
    r += [(64, 64)] * 10 + [(64, 40)] + [(64, 64)] * 53 + [(64, 24)]
    r += [(64, 64)] * 63 + [(96, 65)]
    r += [(64, 64)] * 60 + [(64, 32)] + [(0, 0)] * 5000 + [(0, -1)] * 100 + [(64, 64)] * 3 + [(31, 31)]
    return r


def wave_rows_case(cols, plan, seed, residue=(4, 1)):
    """A (R x nB) and B (nB x cols) for k_wave_rows: plan[b] rows in one-wave class b (1..16), every row a mix of a content
    kind (WAVE_KINDS) and a split (WAVE_SPLITS) at the bottom, top or middle of its class, rows of one class interleaved
    with the others'.  Every A row has B rows of its own (none shared), so rows next to each other never agree.
    A starts with _tail_rows() and ends with three 2048-product rows that make nnz(C) % residue[0] == residue[1].
    Returns dict(a_rp, a_ci, b_rp, b_ci, ncols, nnz_c, tail)."""
    rng = np.random.default_rng(seed)
    levels = wave_levels(cols)
    b_lens, b_cols, a_rows = [], [], []             # a_rows: (alen, first B row, |C|) per group, rows consecutive
    nb = [0]

    def add(cols2d, L, nnz):
        n = cols2d.shape[0]
        L = np.asarray(L, np.int64)
        b_lens.append(np.tile(L, n))
        b_cols.append(cols2d.ravel())
        a_rows.append((np.full(n, L.size), nb[0] + L.size * np.arange(n), np.broadcast_to(nnz, n)))
        nb[0] += n * L.size

    def simple(n, F, u):                                 # F products, u distinct columns, one source
        c = _strata(rng, n, u, 0, cols)[:, np.arange(F) % u]
        add(_scramble(rng, c), [F], u)

    empty = nb[0]                                        # empty B rows
    b_lens.append(np.zeros(4, np.int64))
    b_cols.append(np.zeros(0, np.int64))
    nb[0] += 4
    tail = _tail_rows()
    for F, u in tail:
        if F == 0:
            a_rows.append((np.array([0 if u == 0 else 2]), np.array([empty + 1]), np.array([0])))
        else:
            simple(1, F, u)
    n_tail = len(a_rows)
    tail_bins = np.bincount(row_bins([F for F, _ in tail], cols), minlength=NUM_BINS)
    for b in range(1, 17):
        ch = WAVE_CHUNKS[b - 1]
        lo, hi = 64 * (WAVE_CHUNKS[b - 2] if b > 1 else 0) + 1, 64 * ch
        hb = wave_hash_bits(ch)
        n = plan[b] - int(tail_bins[b]) - (3 if b == 16 else 0)
        j = np.arange(n)
        combo = (j % len(WAVE_KINDS), (j // len(WAVE_KINDS)) % len(WAVE_SPLITS), (j // 35) % 3)
        key = np.ravel_multi_index(combo, (len(WAVE_KINDS), len(WAVE_SPLITS), 3))
        mid = int(rng.integers(lo, hi + 1))
        for kk, cnt in zip(*np.unique(key, return_counts=True)):
            ki, si, fi = np.unravel_index(kk, (len(WAVE_KINDS), len(WAVE_SPLITS), 3))
            kind = WAVE_KINDS[ki]
            F = min(hi, max((lo, hi, mid)[fi], _KIND_MIN_F.get(kind, 1)))
            c, nnz = _content(rng, kind, int(cnt), F, cols, levels, hb)
            add(c, _split(rng, WAVE_SPLITS[si], F), nnz)
    alen = np.concatenate([a[0] for a in a_rows])
    first = np.concatenate([a[1] for a in a_rows])
    nnz = np.concatenate([a[2] for a in a_rows]).astype(np.int64)
    order = np.concatenate([np.arange(n_tail), n_tail + rng.permutation(alen.size - n_tail)])
    # three rows of 2048 products (class 16) whose outputs set nnz(C) mod residue[0]
    before = int(nnz.sum())
    mod, res = residue
    T = (res - before) % 4096 if mod == 4096 else 3 + (res - before - 3) % 4
    T += 4096 if T < 3 else 0
    u1 = min(2048, T - 2)
    u2 = min(2048, T - u1 - 1)
    for u in (u1, u2, T - u1 - u2):
        simple(1, 2048, u)
    alen = np.concatenate([alen[order]] + [a[0] for a in a_rows[-3:]])
    first = np.concatenate([first[order]] + [a[1] for a in a_rows[-3:]])
    a_rp = np.concatenate([[0], np.cumsum(alen)])
    a_ci = np.repeat(first - a_rp[:-1], alen) + np.arange(a_rp[-1])
    b_len = np.concatenate(b_lens)
    b_rp = np.concatenate([[0], np.cumsum(b_len)])
    return dict(a_rp=a_rp.astype(np.int32), a_ci=a_ci.astype(np.int32), b_rp=b_rp.astype(np.int32),
                b_ci=np.concatenate(b_cols).astype(np.int32), ncols=cols, nnz_c=before + T, tail=len(tail))
