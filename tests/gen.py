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


def mixed_class_rows(nrows=200, inner=512, ncols=4096, seed=41):
    """a small product that still reaches every row kind of the general flows: B is inner x ncols with 20 draws per row; of
    A's nrows rows every fourth is empty, the others cycle through 1, 5, 12 and 40 entries (about 20, 100, 240 and 800
    products: four one-wave classes), and row 21 has 150 (about 3000 products: a heavy row).  (a_rp, a_ci, b_rp, b_ci)."""
    rng = np.random.default_rng(seed)
    b_rp, b_ci = uniform_rect(inner, ncols, 20, seed + 1)
    deg = np.array([0, 1, 5, 12, 0, 40, 1, 5] * (nrows // 8 + 1))[:nrows]
    deg[21] = 150
    rows = np.repeat(np.arange(nrows), deg)
    cols = rng.integers(0, inner, size=rows.size)
    a_rp, a_ci = _csr_from_pairs(rows, cols, nrows)
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


def row_bins(F, cols, rank_cap=None):
    """capacity class of every row as csrc/prepass.hip bin_of places it (BSPGEMM_RANK_ROWS at its default; rank_cap = 0:
    without the rank class, as the masked products bin their rows)"""
    mid_cap, default_rank_cap = _mid_rank_caps(cols)
    rank_cap = default_rank_cap if rank_cap is None else rank_cap
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


def expected_bin_caps(cols, rank_cap=None):
    """bspgemm_stats.bin_cap (csrc/context.hip); rank_cap = 0: of the masked products, which have no rank class"""
    mid_cap, default_rank_cap = _mid_rank_caps(cols)
    rank_cap = default_rank_cap if rank_cap is None else rank_cap
    return [0] + WAVE_CAPS + [max(rank_cap, 2048), mid_cap, 0x7fffffff]


MASK_WAVE_MAX_PRODUCTS = 8192   # csrc/wave_masked.hip kMaskWaveMaxProducts: rows with more go to the window kernel


def masked_row_bins(products, mask_len, cols):
    """capacity class of every row of the masked products C = F .* (A*B) (csrc/wave_masked.hip k_mask_lengths, then bin_of
    without the rank class): by the mask row's length AS STORED (repeats and columns at or above B.cols count), 0 for a
    row without products, and a heavy class for a row of more than 8192 products whatever its mask"""
    F = np.asarray(products, np.int64)
    m = np.where(F > 0, np.asarray(mask_len, np.int64), 0)
    m = np.where((m > 0) & (m <= WAVE_CAPS[-1]) & (F > MASK_WAVE_MAX_PRODUCTS), WAVE_CAPS[-1] + 1, m)
    return row_bins(m, cols, rank_cap=0)


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


# ---- the small-product path (csrc/small.hip, csrc/multiply.hip multiply_small): limits, host model, shapes ---------------
SMALL_MAX_PRODUCTS, SMALL_MAX_ROW, SMALL_MAX_ROWS, SMALL_MAX_NNZ_A = 65536, 2048, 1 << 17, 32768   # csrc/kernels.hpp kSmall*
SMALL_TINY = 16                 # kSmallTiny: products of a row that one lane handles alone
SMALL_BIN = 16                  # multiply_small counts every non-empty row in class kWaveBins
# the row sizes around the lane/wave split and around every padding N of the bitonic sort; 10116 products
SMALL_LADDER = (1, 2, 15, 16, 17, 18, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
SMALL_CONTENTS = ("distinct", "same", "pairs", "to16", "to17", "edges")
SMALL_SPLITS = ("one", "ones", "s64", "s65", "holes", "repeat", "mixed")


def small_fits(F):
    """the device's fit test (csrc/small.hip k_small_plan)"""
    F = np.asarray(F, np.int64)
    return F.size > 0 and int(F.sum()) <= SMALL_MAX_PRODUCTS and int(F.max()) <= SMALL_MAX_ROW


def small_expected(flow, small, R, nnz_a, nnz_b, b_rows, F):
    """csrc/multiply.hip small_eligible + the device's fit test (csrc/small.hip)"""
    if flow == "exact" or small == 0 or not 0 < R <= SMALL_MAX_ROWS or nnz_a > SMALL_MAX_NNZ_A:
        return False
    mean_b = nnz_b / b_rows if b_rows > 0 else 0.0
    if small == -1 and nnz_a * mean_b > 0.5 * SMALL_MAX_PRODUCTS:
        return False
    return small_fits(F)


def small_model(a_rp, a_ci, b_rp, r0=0, r1=None):
    """What the small path does with rows [r0, r1), from A and B's row_ptr only, the way csrc/small.hip derives it.
    Per row: F, lane (one lane sorts it), wave (the whole wave does), N (the bitonic sort's padded size, 0 for the others),
    steps (trips of the 64-source gather loop, wave-rows only).  list: the non-empty rows in order (k_small_plan).
    Per 32-row tile (k_small_sizes): f32, nz32, mx32; per 256-row tile (k_small_plan's workgroups): f256, nz256, and before256,
    the products before the tile.  plan_trips: trips of k_small_plan's strided loop over the 32-row sums.  fits."""
    a_rp = np.asarray(a_rp, np.int64)
    r1 = a_rp.size - 1 if r1 is None else r1
    R = r1 - r0
    F = row_products(a_rp, a_ci, b_rp, r0, r1)
    alen = np.diff(a_rp[r0:r1 + 1])
    lane = (F > 0) & (F <= SMALL_TINY)
    wave = F > SMALL_TINY
    N = np.where(wave, np.maximum(64, 1 << np.ceil(np.log2(np.maximum(F, 1))).astype(np.int64)), 0)
    assert np.all((N[wave] >= F[wave]) & ((N[wave] == 64) | (N[wave] < 2 * F[wave])))
    steps = np.where(wave, -(-alen // 64), 0)

    def tiles(x, w, op):
        n = -(-R // w)
        pad = np.zeros(n * w, np.int64)
        pad[:R] = x
        return op(pad.reshape(n, w), axis=1)

    f256 = tiles(F, 256, np.sum)
    return dict(R=R, F=F, alen=alen, lane=lane, wave=wave, N=N, steps=steps, list=np.flatnonzero(F > 0),
                f32=tiles(F, 32, np.sum), nz32=tiles(F > 0, 32, np.sum), mx32=tiles(F, 32, np.max),
                f256=f256, nz256=tiles(F > 0, 256, np.sum), before256=np.cumsum(f256) - f256,
                plan_trips=-(-(-(-R // 32)) // 256), fits=small_fits(F))


def small_reference(a_rp, a_ci, b_rp, b_ci, r0=0, r1=None):
    """rows [r0, r1) of the boolean product as (row_ptr int64, col_idx int32), slice-local: every row is np.unique of its
    concatenated B rows (one np.unique over (row, column) keys).  Independent of the C oracle."""
    a_rp = np.asarray(a_rp, np.int64)
    b_rp = np.asarray(b_rp, np.int64)
    r1 = a_rp.size - 1 if r1 is None else r1
    R = r1 - r0
    lo, hi = int(a_rp[r0]), int(a_rp[r1])
    aci = np.asarray(a_ci[lo:hi], np.int64)
    L = (b_rp[1:] - b_rp[:-1])[aci]
    arow = _seg_ids(np.diff(a_rp[r0:r1 + 1]))
    cs = np.cumsum(L)
    tot = int(cs[-1]) if cs.size else 0
    src = np.repeat(b_rp[:-1][aci] - (cs - L), L) + np.arange(tot)
    key = np.unique((np.repeat(arow, L) << 32) | np.asarray(b_ci, np.int64)[src].astype(np.uint32))
    rp = np.concatenate([[0], np.cumsum(np.bincount(key >> 32, minlength=R))]).astype(np.int64)
    return rp, (key & 0xFFFFFFFF).astype(np.int32)


def small_targets(reps, extra=(), seed=0):
    """`reps` ladders and `extra`, shuffled: lane-rows and wave-rows share the 64-row batches of k_small_rows"""
    t = np.array(list(SMALL_LADDER) * reps + list(extra), np.int64)
    return t[np.random.default_rng(seed).permutation(t.size)]


def _small_distinct(content, F):
    """distinct columns of a row of F products"""
    return {"same": 1, "pairs": max(1, F // 2), "to16": min(F, 16), "to17": min(F, 17)}.get(content, F)


def _small_columns(rng, content, n, F, cols, periodic):
    """n rows x F product columns in gather order; periodic: column k % u at place k (for the `repeat` split), otherwise
    scrambled -- but `distinct`, which is gathered in descending order"""
    u = _small_distinct(content, F)
    base = _strata(rng, n, u, 0, cols)
    if content == "edges":                              # column 0 and the last column (a one-product row: one of the two)
        base[:, 0] = 0
        base[:, u - 1] = cols - 1
        if u == 1:
            base[::2, 0] = 0
    if content == "distinct":
        return base[:, ::-1].copy()
    if periodic:
        return base[:, rng.permutation(u)][:, np.arange(F) % u]
    return _scramble(rng, base[:, np.arange(F) % u])


def _small_split(rng, split, F):
    """source lengths (0: an empty B row) of a row of F products"""
    if split == "one":
        return [F]
    if split == "ones":
        return [1] * F
    if split in ("s64", "s65"):                         # exactly 64 / 65 A-entries
        K = int(split[1:])
        if F >= K:
            return list(1 + rng.multinomial(F - K, np.full(K, 1.0 / K)))
        L = np.zeros(K, np.int64)
        L[rng.permutation(K)[:F]] = 1
        return list(L)
    assert split == "holes", split                      # A-entries on empty B rows before, between and behind the others
    L = [0]
    while sum(L) < F:
        L += [min(int(rng.integers(1, F // 3 + 2)), F - sum(L)), 0] + [0] * int(rng.integers(0, 2))
    return L


def small_rows_case(targets, content, split, cols, seed):
    """A (R x nB) and B (nB x cols) for the small path: row i of A has exactly targets[i] products (0: an empty row; -1: two
    A-entries on an empty B row, no product).  Shuffle the targets (small_targets) to mix lane-rows and wave-rows in the
    64-row batches.  Every A row has B rows of its own, numbered in shuffled order, so A, B and the gathered products are
    unsorted.
    content   distinct: all columns differ, gathered in descending order; same: one column repeated; pairs: every column
              twice (F odd: one of them three times); to16 / to17: exactly 16 / 17 distinct columns (F below that: F);
              edges: distinct, column 0 and column cols - 1 among them
    split     one: one A-entry on a B row of F entries; ones: F A-entries on one-entry B rows; s64 / s65: exactly 64 / 65
              A-entries (empty B rows among them when F is smaller); holes: A-entries on empty B rows interleaved;
              repeat: the same B row of the row's distinct columns referenced again and again (not for distinct / edges);
              mixed: the rows of one size take the splits in turn
    Returns a_rp, a_ci, b_rp, b_ci (int32)."""
    assert content in SMALL_CONTENTS and split in SMALL_SPLITS and not (split == "repeat" and content in ("distinct", "edges"))
    rng = np.random.default_rng(seed)
    targets = np.asarray(targets, np.int64)
    R = targets.size
    turn = [s for s in SMALL_SPLITS[:-1] if s != "repeat" or content not in ("distinct", "edges")] if split == "mixed" else [split]
    alen = np.zeros(R, np.int64)
    g_pos, g_acols, b_lens, b_cols = [], [], [], []
    nb = 1                                              # B row 0 stays empty: the rows of target -1 point at it
    dead = np.flatnonzero(targets == -1)
    alen[dead] = 2
    g_pos.append(dead)
    g_acols.append(np.zeros(2 * dead.size, np.int64))
    b_lens.append(np.zeros(1, np.int64))
    for F in np.unique(targets[targets > 0]):
        F = int(F)
        rows = np.flatnonzero(targets == F)
        for v, sp in enumerate(turn):
            pos = rows[v::len(turn)]
            n = pos.size
            if n == 0:
                continue
            c = _small_columns(rng, content, n, F, cols, sp == "repeat")
            if sp == "repeat":                          # B row 0 of the block: the distinct columns; B row 1: the first F % u
                u = _small_distinct(content, F)
                k, rem = F // u, F % u
                src = np.array([0] * (k // 2) + ([1] if rem else []) + [0] * (k - k // 2))
                blen = np.array([u] + ([rem] if rem else []))
                bidx = np.concatenate([np.arange(u), np.arange(rem)])
            else:                                       # source s of the row is B row perm[s] of the block
                L = np.asarray(_small_split(rng, sp, F), np.int64)
                src = rng.permutation(L.size)
                order = np.argsort(src)
                start = np.cumsum(L) - L
                blen = L[order]
                bidx = np.repeat(start[order] - (np.cumsum(blen) - blen), blen) + np.arange(F)
            alen[pos] = src.size
            g_pos.append(pos)
            g_acols.append((nb + blen.size * np.arange(n)[:, None] + src[None, :]).ravel())
            b_lens.append(np.tile(blen, n))
            b_cols.append(c[:, bidx].ravel())
            nb += n * blen.size
    a_rp = np.concatenate([[0], np.cumsum(alen)])
    a_ci = np.zeros(int(a_rp[-1]), np.int64)
    pos = np.concatenate(g_pos)
    a_ci[np.repeat(a_rp[pos] - (np.cumsum(alen[pos]) - alen[pos]), alen[pos]) + np.arange(a_ci.size)] = np.concatenate(g_acols)
    renum = np.concatenate([[0], 1 + rng.permutation(nb - 1)])            # B's rows in shuffled order
    lens = np.zeros(nb, np.int64)
    lens[renum] = np.concatenate(b_lens)
    b_rp = np.concatenate([[0], np.cumsum(lens)])
    old_cols = np.concatenate(b_cols) if b_cols else np.zeros(0, np.int64)
    old_lens = np.concatenate(b_lens)
    b_ci = np.zeros(int(b_rp[-1]), np.int64)
    b_ci[np.repeat(b_rp[renum] - (np.cumsum(old_lens) - old_lens), old_lens) + np.arange(b_ci.size)] = old_cols
    assert cols <= 0x7fffffff and (b_ci.size == 0 or int(b_ci.max()) < cols)
    return a_rp.astype(np.int32), renum[a_ci].astype(np.int32), b_rp.astype(np.int32), b_ci.astype(np.int32)


# ---- the products of tests/test_gpu_small_path.py, checked without a GPU by tests/test_small_path_shapes.py ------------------
def _small_case(targets, content, split, cols, seed, **kw):
    a_rp, a_ci, b_rp, b_ci = small_rows_case(targets, content, split, cols, seed)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=cols, content=content, split=split, **kw)


SMALL_LADDER_PLAN = (       # (content, split, columns, ladders): `ones` and same x repeat have one A-entry per product
    ("distinct", "one", 6000, 6), ("distinct", "s65", 6000, 6), ("distinct", "mixed", 6000, 6), ("same", "ones", 6000, 3),
    ("same", "repeat", 6000, 3), ("pairs", "s64", 6000, 6), ("pairs", "holes", 6000, 6), ("to16", "repeat", 6000, 6),
    ("to16", "one", 6000, 6), ("to17", "s65", 6000, 6), ("to17", "mixed", 6000, 6), ("edges", "holes", 6000, 6),
    ("edges", "ones", 6000, 3),
    ("distinct", "ones", 600_000_000, 3), ("same", "s64", 600_000_000, 6), ("pairs", "repeat", 600_000_000, 6),
    ("to16", "s65", 600_000_000, 6), ("to17", "holes", 600_000_000, 6), ("edges", "one", 600_000_000, 6),
    ("edges", "mixed", 2**31 - 1, 6),       # the largest column, 2^31 - 2, against the sort's sentinel: the small path only
)


def small_ladder_cases():
    """{name: builder} of the row-ladder products: every size of SMALL_LADDER `ladders` times and 1 .. 16 twice, shuffled"""
    out = {}
    for k, (content, split, cols, reps) in enumerate(SMALL_LADDER_PLAN):
        out["ladder_%s_%s_%d" % (content, split, cols)] = lambda k=k, a=(content, split, cols), reps=reps: _small_case(
            small_targets(reps, list(range(1, 17)) * 2, seed=2100 + k), *a, seed=2200 + k, reps=reps, small_only=a[2] > 600_000_000)
    return out


def _sprinkle(R, n, value, seed, forced=()):
    """targets of R rows: `value` at `n` rows (the `forced` ones first, the others random), 0 elsewhere"""
    rng = np.random.default_rng(seed)
    t = np.zeros(R, np.int64)
    forced = np.array(sorted(set(int(r) for r in forced if 0 <= r < R)), np.int64)
    free = np.setdiff1d(np.arange(R), forced)
    t[np.concatenate([forced, rng.permutation(free)[:max(0, n - forced.size)]])[:max(n, 0)]] = value
    return t


def _fit_total(total):
    """R = 2^17, 32768 one-entry rows on two-entry B rows, all distinct: 65536 products = nnz(C); the last non-empty row
    one product more or less for 65537 / 65535"""
    t = _sprinkle(SMALL_MAX_ROWS, 32768, 2, 2301, forced=(0, SMALL_MAX_ROWS - 1))
    t[np.flatnonzero(t)[-2]] += total - 65536
    return _small_case(t, "distinct", "one", 6000, 2302, total=total)


def _fit_row(big):
    """one row of `big` products among 300 rows of 1 .. 3, at row 8250: its 32-row tile is number 257, which k_small_plan's
    strided loop reaches on its second trip"""
    t = _sprinkle(8300, 300, 1, 2311, forced=(0, 8191, 8192, 8299))
    nz = np.flatnonzero(t)
    t[nz] = 1 + np.arange(nz.size) % 3
    t[8250] = big
    return _small_case(t, "pairs", "s65", 600_000_000, 2312, big_row=8250)


def _fit_nnz_a(nnz_a):
    """`nnz_a` one-entry rows on one-entry B rows among 2^17: the host's limit on A-nonzeros"""
    return _small_case(_sprinkle(SMALL_MAX_ROWS, nnz_a, 1, 2321), "distinct", "one", 6000, 2322)


def _fit_rows(R):
    return _small_case(_sprinkle(R, 500, 5, 2331, forced=(0, R - 1)), "pairs", "holes", 6000, 2332)


def _fit_auto(extra):
    """256 x 16 A-entries on rows 0 .. 62 of a 64 x 8 B: 4096 x 8.0 = 32768, the automatic choice's limit; `extra` more
    entries in B's unreferenced row 63 put the estimate above it (same product)"""
    rng = np.random.default_rng(2341)
    b_len = np.full(64, 8)
    b_len[63] += extra
    b_rp = np.concatenate([[0], np.cumsum(b_len)]).astype(np.int32)
    a_rp = (16 * np.arange(257)).astype(np.int32)
    a_ci = rng.integers(0, 63, size=4096).astype(np.int32)
    b_ci = rng.integers(0, 1000, size=int(b_rp[-1])).astype(np.int32)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=1000)


def small_fit_cases():
    return {"fit_total_65536": lambda: _fit_total(65536), "fit_total_65537": lambda: _fit_total(65537),
            "fit_total_65535": lambda: _fit_total(65535), "fit_row_2049": lambda: _fit_row(2049), "fit_row_2048": lambda: _fit_row(2048),
            "fit_nnz_a_32769": lambda: _fit_nnz_a(32769), "fit_rows_131073": lambda: _fit_rows(SMALL_MAX_ROWS + 1),
            "fit_auto_at_limit": lambda: _fit_auto(0), "fit_auto_above_limit": lambda: _fit_auto(1)}


SMALL_TILE_ROWS = (1, 31, 32, 33, 255, 256, 257, 8191, 8192, 8193, 65537)
SMALL_TILE_NONEMPTY = {255: 63, 256: 64, 257: 65}          # the list is 63, 64, 65 rows long: one batch of k_small_rows +- 1


def _tile_case(R):
    """R rows, the non-empty ones at the 32-, 256- and 8192-row tile edges and at random places: sizes 1 .. 40 (lane-rows and
    wave-rows), every seventh other row with A-entries on an empty B row only (no product: not listed)"""
    edge = [r for r in (0, 31, 32, 255, 256, 257, 8191, 8192, R - 1) if r < R]
    n = SMALL_TILE_NONEMPTY.get(R, min(R, max(len(edge), 1) + min(R // 3, 120)))
    t = _sprinkle(R, n, 1, 2400 + R, forced=edge)
    nz = np.flatnonzero(t)
    t[nz] = 1 + (7 * np.arange(nz.size) + R) % 40
    dead = np.flatnonzero(t == 0)[::7]
    t[dead] = -1
    return _small_case(t, "pairs", "mixed", 6000, 2500 + R, edge=edge, nonempty=n)


def small_tile_cases():
    return {"tile_rows_%d" % R: (lambda R=R: _tile_case(R)) for R in SMALL_TILE_ROWS}


SMALL_RANGES = ((5, 6), (37, 70), (101, 358))              # r0 % 32 != 0, r1 - r0 = 1, 33, 257


def small_range_case():
    """700 rows of 0 .. 40 products, some without a product, rows 5 and 300 of 600: the operand of the row-range products"""
    rng = np.random.default_rng(2601)
    t = rng.integers(-1, 41, size=700)
    t[5], t[300], t[37], t[69], t[101], t[357] = 600, 600, 17, 16, 2, 33
    t[[40, 110]], t[[41, 111]] = 0, -1
    return _small_case(t, "pairs", "mixed", 6000, 2602, ranges=SMALL_RANGES)


# ---- masks with columns at or above B.cols: tests/test_gpu_masked.py, checked without a GPU by tests/test_masked_shapes.py ----
INT_MAX = 2**31 - 1
MASK_CAPS = (64, 128, 256, 512, 768, 1024, 2048)    # mask-row capacities of k_wave_masked (wave_masked.hip launch_mask_levels)
# the three depths of k_wave_masked and both sides of each depth boundary
MASK_ONE_WAVE_COLS = (1000, 8192, 8193, 100_000, 1 << 18, (1 << 18) + 1, 5_000_000, 1 << 23)
MASK_WINDOW_COLS = (300_001, 700_001, (1 << 23) + 1)  # one window, two windows, every row on the window kernel (17 windows)
MASK_KEEP_WINDOW = 1 << 19                          # columns per window of the Keep window kernel: two bitmaps share 128 KiB
MASK_KINDS = ("mixed", "beyond only", "one in range")


def mask_levels(cols):
    """LEVELS of k_wave_masked for `cols` columns (kernels.hpp levels_for_cols); 0: above 2^23, the window kernel only"""
    return next((lv for lv in (1, 2, 3) if cols <= 256 << (5 * lv)), 0)


def mask_cap_of_len(m):
    """the capacity of the k_wave_masked instance that takes a mask row of m entries (1 .. 2048)"""
    return MASK_CAPS[int(np.searchsorted(np.array(MASK_CAPS), m, side="left"))]


def mask_window(cols):
    """columns per window of the Keep window kernel (dense_rows.hip launch_dense_impl)"""
    return min(-(-cols // 64) * 64, MASK_KEEP_WINDOW)


def mask_alias_spans(cols):
    """the distances at which a mask column at or above B.cols would land on a product column in a kernel that truncated
    or wrapped its index: the reach of the top bitmap, 256 * 32^LEVELS (k_wave_masked), and the window (k_dense_rows)"""
    L = mask_levels(cols)
    return ([256 << (5 * L)] if L else []) + [mask_window(cols)]


def masked_reference(want, f_rp, f_ci, r0=0, r1=None):
    """rows [r0, r1) of `want` (the product, (row_ptr, col_idx) with sorted duplicate-free rows) restricted to F's entries,
    F indexed by absolute row: (row_ptr int64 slice-local, col_idx int32).  F's columns are compared as they are stored, so
    F may hold any column, repeats and unsorted rows."""
    rp, ci = np.asarray(want[0], np.int64), np.asarray(want[1])
    r1 = rp.size - 1 if r1 is None else r1
    f_rp = np.asarray(f_rp, np.int64)
    rows = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(rp[r0:r1 + 1]))
    kc = (rows << 32) | ci[rp[r0]:rp[r1]].astype(np.int64)
    frow = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(f_rp[r0:r1 + 1]))
    kf = (frow << 32) | np.asarray(f_ci[f_rp[r0]:f_rp[r1]], np.int64)
    keep = np.isin(kc, kf)
    counts = np.bincount((kc[keep] >> 32) - r0, minlength=r1 - r0)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), ci[rp[r0]:rp[r1]][keep].astype(np.int32)


def _beyond_columns(rng, cols, absent, top):
    """mask columns at or above `cols` (and at most `top`) that must change nothing, the telling ones first: B.cols itself;
    for every alias span S: S itself, a column of [B.cols, S) and p + k * S (k = 1, 2, 3) for product columns p of the row
    that are NOT in the mask; the next window edge and a column below it; p + 2^30; `top`"""
    spans = mask_alias_spans(cols)
    W = mask_window(cols)
    edge = -(-cols // W) * W
    out = [cols]
    ps = [int(p) for p in absent[:2]]
    for S in spans:
        out.append(S)
        if S > cols:
            out.append(int(rng.integers(cols, S)))
        out += [p + k * S for p in ps[:1] for k in (1, 2, 3)]
    out.append(edge)
    if edge > cols:
        out.append(int(rng.integers(cols, edge)))
    out += [p + k * S for S in spans for p in ps[1:] for k in (1, 2, 3)]
    out += [p + (1 << 30) for p in ps]
    out.append(top)
    return np.array([c for c in out if cols <= c <= top], np.int64)


def _mask_row(rng, prod, n_in, noise, length, cols, top):
    """one mask row: n_in of the row's product columns `prod`, `noise` random columns of [0, cols), the columns of
    _beyond_columns, some entries twice, and random columns at or above `cols` up to exactly `length` entries (None: no
    filling); shuffled.  The product columns go first when `length` is short."""
    pick = rng.permutation(prod)[:n_in]
    inr = np.concatenate([pick, rng.integers(0, cols, size=noise)]) if noise else pick
    bey = _beyond_columns(rng, cols, np.setdiff1d(prod, inr), top)
    if length is None:
        row = np.concatenate([inr, bey])
        row = np.concatenate([row, row[rng.integers(0, row.size, size=min(5, row.size))]])
        return rng.permutation(row)
    inr = inr[:length]
    bey = bey[:length - inr.size]
    row = np.concatenate([inr, bey])
    nrep = min(length - row.size, 5, length // 8)
    fill = length - row.size - nrep
    S = mask_alias_spans(cols)[0]
    near = fill // 2 if S > cols else 0                  # half of the filling within the top bitmap / the last window
    parts = [row, row[rng.integers(0, row.size, size=nrep)] if nrep else row[:0],
             rng.integers(cols, max(S, cols + 1), size=near), rng.integers(cols, top, size=fill - near)]
    return rng.permutation(np.concatenate(parts))


def _case(a_rp, a_ci, b_rp, b_ci, cols, rows, kinds, top):
    f_rp = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    f_ci = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    assert f_ci.min() >= 0 and f_ci.max() <= top <= INT_MAX
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    return dict(a_rp=i32(a_rp), a_ci=i32(a_ci), b_rp=i32(b_rp), b_ci=i32(b_ci), ncols=cols, f_rp=i32(f_rp), f_ci=i32(f_ci),
                kinds=np.array(kinds), top=top, products=row_products(a_rp, a_ci, b_rp, 0, len(rows)))


def masked_one_wave_case(cols, top=INT_MAX, nrows=2000):
    """A (nrows x 500, 6 entries per row, every 97th row empty), B (500 x cols, 1 to 39 entries per row: no row has more
    than 8192 products) and a mask F whose rows hold columns at and far above B.cols (_beyond_columns) up to `top`.
    Row i is of capacity MASK_CAPS[i % 7]; within a capacity the rows take the lengths (bottom, top, between) and the
    kinds MASK_KINDS in turn: mixed = a random half of the row's product columns, three columns of [0, cols) and the columns
    beyond; beyond only = no column below B.cols (an empty output row); one in range = one product column and else
    columns beyond.  Returns the operands, f_rp / f_ci, kinds (per row), products (per row), top."""
    rng = np.random.default_rng(7100 + cols % 9973)
    a_rp, a_ci = uniform_rect(nrows, 500, 6, seed=1901)
    ar = np.repeat(np.arange(nrows), np.diff(a_rp))
    a_rp, a_ci = _csr_from_pairs(ar[ar % 97 != 5], a_ci[ar % 97 != 5], nrows)
    lens = rng.integers(1, 40, size=500)
    b_cols = rng.integers(0, cols, size=int(lens.sum()))
    b_cols[::53], b_cols[7::53] = cols - 1, 0              # the last column and column 0 among the products
    b_rp, b_ci = _csr_from_pairs(np.repeat(np.arange(500), lens), b_cols, 500)
    p_rp, p_ci = small_reference(a_rp, a_ci, b_rp, b_ci)
    rows, kinds = [], []
    for i in range(nrows):
        g, j = i % 7, i // 7
        lo, hi = (MASK_CAPS[g - 1] + 1 if g else 1), MASK_CAPS[g]
        length = (lo, hi, int(rng.integers(lo, hi + 1)))[j % 3]
        kind = MASK_KINDS[(j // 3) % 3]
        prod = p_ci[p_rp[i]:p_rp[i + 1]].astype(np.int64)
        n_in, noise = {"mixed": ((prod.size + 1) // 2, 3), "beyond only": (0, 0), "one in range": (1, 0)}[kind]
        rows.append(_mask_row(rng, prod, n_in, noise, length, cols, top))
        kinds.append(kind)
    return _case(a_rp, a_ci, b_rp, b_ci, cols, rows, kinds, top)


MASK_WINDOW_KINDS = ("half", "short", "beyond only, long", "half, filled long")


def masked_window_case(cols, top=INT_MAX, nrows=402):
    """A (nrows x 300) and B (300 x cols, 100 to 299 entries per row, unsorted with repeats, a fifth of them in the last
    3000 columns) for the Keep window kernel.  Rows 0 and 1 of A draw every B row (about 60 000 products), the others 1 to
    60 of them (up to 12 000 products).  Masks, MASK_WINDOW_KINDS in turn from row 2 on: half = a random half of the row's
    product columns (row 0 too: far more than 2048); short = at most 100 of them (row 1 too: a short mask on a row of more
    than 8192 products); beyond only, long = 2100 columns at or above B.cols; half, filled long = half of the product
    columns and columns beyond up to 2049 entries or more.  Every row also holds _beyond_columns, up to `top`."""
    rng = np.random.default_rng(7300 + cols % 9973)
    nb = 300
    lens = rng.integers(100, 300, size=nb)
    b_rows = np.repeat(np.arange(nb), lens)
    b_cols = np.where(rng.random(b_rows.size) < 0.2, rng.integers(max(0, cols - 3000), cols, size=b_rows.size),
                      rng.integers(0, cols, size=b_rows.size))
    b_cols[::97], b_cols[7::97] = cols - 1, 0              # the last column and column 0 among the products
    b_rp, b_ci = _csr_from_pairs(b_rows, b_cols, nb, dedup=False, sort=False)
    a_rows = [np.concatenate([np.arange(nb), rng.integers(0, nb, size=50)]) for _ in range(2)]
    a_rows += [rng.integers(0, nb, size=int(rng.integers(1, 61))) for _ in range(nrows - 2)]
    a_rp = np.concatenate([[0], np.cumsum([r.size for r in a_rows])])
    a_ci = np.concatenate(a_rows)
    p_rp, p_ci = small_reference(a_rp, a_ci, b_rp, b_ci)
    rows, kinds = [], []
    for i in range(nrows):
        kind = MASK_WINDOW_KINDS[(0, 1)[i] if i < 2 else i % 4]
        prod = p_ci[p_rp[i]:p_rp[i + 1]].astype(np.int64)
        half = (prod.size + 1) // 2
        n_in, noise, length = {"half": (half, 3, None), "short": (min(half, 100), 3, None), "beyond only, long": (0, 0, 2100),
                               "half, filled long": (half, 3, max(2049, half + 40))}[kind]
        rows.append(_mask_row(rng, prod, n_in, noise, length, cols, top))
        kinds.append(kind)
    return _case(a_rp, a_ci, b_rp, b_ci, cols, rows, kinds, top)


# ---- the heavy rows (csrc/dense_rows.hip over csrc/heavy_gather.hpp): constants, host model, shapes -------------------------
# tests/test_gpu_heavy_rows.py; every constant mirrors the kernels' by name
HEAVY_SHAPES = {512: (512, 8, 4),       # dense_rows.hip kDenseThreadsMid, kDenseQuadsPerThreadMid, kDenseInFlightMid (= kRankThreads, kRankQPT, kRankInFlight)
                1024: (1024, 16, 8)}    # dense_rows.hip kDenseThreadsBig, kDenseQuadsPerThreadBig, kDenseInFlightBig (Keep, Count too)
HEAVY_WINDOW_WORDS = {512: 4096, 1024: 16384, "keep": 8192}    # dense_rows.hip kMidMaxWords, kDenseMaxWords, launch_dense_impl max_words (two bitmaps)
RANK_SPAN = 1 << 20                     # dense_rows.hip kRankSpan
RANK_CAP = 6144                         # kernels.hpp kRankCap
RANK_THREADS = 512                      # dense_rows.hip kRankThreads
READOUT_STEP_WORDS, READOUT_WPL = 256, 4    # dense_rows.hip k_dense_rows kStepWords, kWpl
DENSE_WORD_BITS = 12                    # dense_rows.hip kDenseWordBits
COUNT_MAX_COLS, COUNT_SLOTS = 1 << 18, 20480    # dense_rows.hip kCountMaxCols, kCountSlots
HEAVY_MIN = 2048                        # kernels.hpp kMaxWaveCap: rows with more products are heavy
HEAVY_POPS = (1, 2, 3, 11, 12, 13, 63, 64)      # word popcounts around the pair store's tail and kDenseWordBits
HEAVY_MODES = ("none", "keep", "drop", "insert", "count")
HEAVY_LEFTS = ("1", "q", "q+1", "2q", "2q+1", "3q", "3q+1", "step")


def heavy_tile(shape):
    """(tile, step, quarter step) in quads of a thread shape (heavy_gather.hpp kTileQ, kInFlight * kThreads, the thresholds)"""
    T, qpt, fl = shape
    return T * qpt, T * fl, T * fl // 4


def heavy_window_geometry(cols, threads, keep=False):
    """(wwords, nwin, wpw) of k_dense_rows: launch_dense_impl's words per window, the windows, the words per wave"""
    cap = HEAVY_WINDOW_WORDS["keep" if keep else threads]
    wwords = max(1, min(-(-cols // 64), cap))
    nwin = -(-cols // (64 * wwords))
    wpw = -(-(-(-wwords // (threads // 64))) // READOUT_STEP_WORDS) * READOUT_STEP_WORDS
    return wwords, nwin, wpw


def _row_entries(b_rp, b_ci, src):
    """the products of one A row in gather order: (columns, source index, B position) per entry"""
    s, L = b_rp[src], b_rp[src + 1] - b_rp[src]
    tot = int(L.sum())
    sid = np.repeat(np.arange(src.size), L)
    pos = np.repeat(s - (np.cumsum(L) - L), L) + np.arange(tot)
    return np.asarray(b_ci, np.int64)[pos], sid, pos


def heavy_gather_plan(L, shape):
    """gather_sweep's decisions for a row whose sources have the lengths L: batches (sources, nonempty, QB, tiles of
    (nqt, left, nu, starts)), kept, and the cells the plan reaches as strings"""
    T, qpt, fl = shape
    tile, step, q = heavy_tile(shape)
    L = np.asarray(L, np.int64)
    nq_all = -(-L // 4)
    names = {1: "1", q: "q", q + 1: "q+1", 2 * q: "2q", 2 * q + 1: "2q+1", 3 * q: "3q", 3 * q + 1: "3q+1", step: "step"}
    batches, cells = [], set()
    nb = -(-L.size // T)
    for j in range(nb):
        n = nq_all[j * T:(j + 1) * T]
        QB = int(n.sum())
        ex = np.cumsum(n) - n
        st, ln = ex[n > 0], n[n > 0]
        tiles = []
        for T0 in range(0, QB, tile):
            nqt = min(QB - T0, tile)
            left = nqt - (nqt - 1) // step * step
            nu = fl if left > 3 * q else 3 * fl // 4 if left > 2 * q else fl // 2 if left > q else fl // 4
            starts = int(((st >= T0) & (st < T0 + tile)).sum())
            tiles.append(dict(nqt=nqt, left=left, nu=nu, starts=starts))
            cells.add("g:nu=%d/4" % (4 * nu // fl))
            if left in names:
                cells.add("g:left=" + names[left])
            if starts == 0:
                cells.add("g:tile without a start")
        batches.append(dict(sources=int(n.size), nonempty=int((n > 0).sum()), QB=QB, tiles=tiles))
        if QB == 0 and nb > 1:
            cells.add("g:empty batch " + ("first" if j == 0 else "last" if j == nb - 1 else "middle"))
        if ((st % tile == 0) & (st > 0)).any():
            cells.add("g:start on quad 0 of a later tile")
        if (st % tile == tile - 1).any():
            cells.add("g:start on the last quad of a tile")
        if (st // tile != (st + ln - 1) // tile).any():
            cells.add("g:source crosses a tile boundary")
        if len(tiles) > 1:
            cells.add("g:several tiles")
    if nb > 1:
        cells.add("g:several batches")
    QBl = batches[-1]["QB"] if batches else 0
    kept = L.size <= T and 0 < QBl <= tile
    for k in range(1, 9):
        if (L == k).any():
            cells.add("g:len%d" % k)
    if L.size == T and QBl == tile:
        cells.add("g:T sources, QB == tile")
    if L.size == T + 1:
        cells.add("g:T+1 sources")
    if nb == 1 and QBl == tile + 1:
        cells.add("g:QB == tile+1")
    return dict(batches=batches, kept=bool(kept), QB=QBl, cells=cells)


def _quad_cells(c, sid, pos, b_rp, src, nnz_b):
    """cells of the quads' content: lanes as the kernel lays them (the last quad of a source ends at the source's end, a quad
    never starts before B.col_idx), word order inside a quad; returns (cells, lane of every entry)"""
    cells = set()
    s = b_rp[src][sid]
    e = b_rp[src + 1][sid]
    p = pos - s
    qs = s + 4 * (p // 4)
    b = np.maximum(np.minimum(qs, e - 4), 0)
    lane = pos - b
    nqs = -(-(b_rp[src + 1] - b_rp[src]) // 4)
    quad = np.repeat(np.cumsum(nqs) - nqs, b_rp[src + 1] - b_rp[src]) + p // 4
    nquads = int(nqs.sum())
    w = np.full((nquads, 4), -1, np.int64)
    w[quad, lane] = c >> 5
    v = w >= 0
    for k in range(3):
        if (v[:, k] & v[:, k + 1] & (w[:, k + 1] < w[:, k])).any():
            cells.add("g:words not ascending")
    for i, j in ((0, 2), (1, 3), (0, 3)):
        if (v[:, i] & v[:, j] & (w[:, i] == w[:, j]) & (w[:, i + 1] != w[:, i])).any():
            cells.add("g:equal words apart")
    if (e[pos == e - 1] == nnz_b).any():
        cells.add("g:quad ends at nnzB")
    if (np.minimum(qs, e - 4) < 0).any():
        cells.add("g:quad clamped to 0")
    return cells, lane


def heavy_readout(out, cols, threads, keep=False):
    """the window read-out of k_dense_rows for the output row `out` (sorted distinct columns): windows and the empty ones,
    wave_words (every wave's word range [wbeg, wend), empty for the waves of `idle`), per step the outputs and stage_cap, cells"""
    wwords, nwin, wpw = heavy_window_geometry(cols, threads, keep)
    waves = threads // 64
    W = 64 * wwords
    cells = set()
    pc = np.bincount(out >> 6, minlength=nwin * wwords).reshape(nwin, wwords)
    idle = [k for k in range(waves) if k * wpw >= wwords]
    if idle:
        cells.add("r:idle waves")
    w0 = np.arange(0, wwords, READOUT_STEP_WORDS)
    width = np.minimum(READOUT_STEP_WORDS, wwords - w0)          # (waves start on multiples of the step)
    cap = 2 * width
    tot = np.add.reduceat(pc, w0, axis=1)
    empty_win = tot.sum(axis=1) == 0
    if empty_win.any():
        cells.add("r:empty window")
    if (~empty_win).sum() > 1:
        cells.add("r:several windows with outputs")
    staged = (tot > 0) & (tot <= cap)
    direct = tot > cap
    tail = np.broadcast_to(width < READOUT_STEP_WORDS, tot.shape)
    for name, f in (("r:step skipped", (tot == 0) & ~empty_win[:, None]), ("r:step staged", staged & ~tail), ("r:step direct", direct & ~tail),
                    ("r:outputs == 1", tot == 1), ("r:outputs == stage_cap", (tot == cap) & ~tail), ("r:outputs == stage_cap+1", (tot == cap + 1) & ~tail),
                    ("r:full step", tot == 64 * width), ("r:tail staged", staged & tail), ("r:tail direct", direct & tail),
                    ("r:tail outputs == stage_cap", (tot == cap) & tail), ("r:tail outputs == stage_cap+1", (tot == cap + 1) & tail),
                    ("r:tail skipped", (tot == 0) & tail & ~empty_win[:, None])):
        if f.any():
            cells.add(name)
    dmask = np.repeat(direct, width, axis=1)
    dp = pc[dmask]
    for k in HEAVY_POPS:
        if (dp == k).any():
            cells.add("r:direct pop %d" % k)
    have = set(out[np.isin(out, np.concatenate([np.arange(1, nwin) * W + d for d in (-1, 0, 1)] + [[cols - 1]]))].tolist()) if out.size else set()
    for k in range(1, nwin):
        for d, name in ((-1, "below"), (0, "at"), (1, "above")):
            if k * W + d < cols:
                cells.add("r:column %s a boundary %s" % (name, "set" if k * W + d in have else "clear"))
    if cols - 1 in have:
        cells.add("r:last column")
        if cols % W == 1 and nwin > 1:
            cells.add("r:last window of one column")
    return dict(wwords=wwords, nwin=nwin, wpw=wpw, idle=idle, wave_words=[(min(k * wpw, wwords), min((k + 1) * wpw, wwords)) for k in range(waves)],
                tail=int(width[-1]) if width[-1] < READOUT_STEP_WORDS else 0,
                empty_windows=np.flatnonzero(empty_win).tolist(), step_total=tot, stage_cap=cap, cells=cells)


def heavy_count_windows(fcols, prod, cols):
    """the windows of k_dense_rows_count for a row with the distinct in-range mask columns `fcols` (sorted): a list of
    (lo, W, what) with what in skipped / narrowed / swept, and the cells"""
    out, cells = [], set()
    lo, W = 0, COUNT_MAX_COLS
    swept = 0
    while lo < cols:
        W = min(W, cols - lo)
        nd = int(np.searchsorted(fcols, lo + W) - np.searchsorted(fcols, lo))
        if nd == 0:
            out.append((lo, W, "skipped"))
            cells.add("c:window skipped")
            lo += W
            W = min(2 * W, COUNT_MAX_COLS)
            continue
        if nd > COUNT_SLOTS:
            out.append((lo, W, "narrowed"))
            cells.add("c:window narrowed")
            Wn = W >> 1
            while Wn > COUNT_SLOTS and Wn * nd > COUNT_SLOTS * W:
                Wn >>= 1
            W = Wn & ~31
            continue
        out.append((lo, W, "swept"))
        if swept == 0 and lo > 0:
            cells.add("c:first sweep in a later window")
        swept += 1
        np_ = int(np.searchsorted(prod, lo + W) - np.searchsorted(prod, lo))
        cells.add("c:swept window " + ("with products" if np_ else "without a product"))
        lo += W
        if nd <= COUNT_SLOTS // 2:
            W = min(2 * W, COUNT_MAX_COLS)
    return out, swept, cells


def heavy_rank(prod, dcols, cols, mode):
    """k_rank_rows for a row with the distinct product columns `prod` and D's distinct in-range columns `dcols` (Insert)"""
    cells = set()
    span = min(cols, RANK_SPAN)
    topw = -(-(-(-span // 1024)) // RANK_THREADS) * RANK_THREADS
    nspans = -(-cols // RANK_SPAN)
    cells.add("k:topw %d" % topw)
    spans = []
    for sp in range(nspans):
        lo = sp * RANK_SPAN
        p = prod[(prod >= lo) & (prod < lo + RANK_SPAN)] - lo
        d = dcols[(dcols >= lo) & (dcols < lo + RANK_SPAN)] - lo if mode == "insert" else prod[:0]
        allc = np.union1d(p, d)
        slots = np.unique(allc >> 5)
        nslots = int(slots.size)
        spt = min(max(-(-nslots // RANK_THREADS), 1), RANK_CAP // RANK_THREADS)
        spans.append(dict(nslots=nslots, spt=spt, products=int(p.size)))
        if nslots:
            cells.add("k:spt %d" % spt)
            first = np.arange(0, nslots, spt)[:RANK_THREADS]        # the first slot of every thread that owns one
            tw = slots >> 5
            firsts = np.flatnonzero(np.concatenate([[True], tw[1:] != tw[:-1]]))
            if not np.isin(first, firsts).all():
                cells.add("k:skip > 0")
            if (np.diff(np.append(firsts, nslots)) == 32).any():
                cells.add("k:full top word")
            if (np.bincount(np.searchsorted(slots, allc >> 5)) == 32).any():
                cells.add("k:full slot")
        if p.size == 0:
            cells.add("k:span without a product" + (", D reaches it" if d.size else ""))
    if nspans > 1 and cols % RANK_SPAN == 1 and cols - 1 in set(prod[-1:].tolist()):
        cells.add("k:last span of one column")
    return dict(topw=topw, spans=spans, cells=cells)


def heavy_model(a_rp, a_ci, b_rp, b_ci, cols, mode, r0, r1, f=None):
    """What the heavy-row kernels decide for the product over rows [r0, r1), from the operands alone (numpy, no GPU).
    mode: none | keep | drop | insert | count; f = (f_rp, f_ci): the mask, or D.  Returns dict(F, bins, rows): rows maps every
    heavy row to dict(kernel, shape, plan, out, cells) -- kernel one of rank / rank spans / win512 / win1024 / keep / count,
    plan from heavy_gather_plan, cells the set of every cell of the issue's lists that the row reaches (strings)."""
    assert mode in HEAVY_MODES and (f is not None or mode == "none")
    a_rp, b_rp = np.asarray(a_rp, np.int64), np.asarray(b_rp, np.int64)
    a_ci = np.asarray(a_ci, np.int64)
    F = row_products(a_rp, a_ci, b_rp, r0, r1)
    flen = np.diff(np.asarray(f[0], np.int64))[r0:r1] if f is not None else np.zeros(r1 - r0, np.int64)
    if mode in ("keep", "count"):
        bins = masked_row_bins(F, flen, cols)
    else:
        bins = row_bins(F + flen if mode == "insert" else F, cols)
    nnz_b = int(b_rp[-1])
    rows = {}
    for i in np.flatnonzero(bins > 16) + r0:
        b = int(bins[i - r0])
        if mode in ("keep", "count"):
            kernel, threads = mode, 1024
        elif b == RANK_BIN:
            kernel, threads = ("rank spans" if cols > RANK_SPAN else "rank"), 512
        else:
            kernel, threads = ("win512", 512) if b == MID_BIN else ("win1024", 1024)
        shape = HEAVY_SHAPES[threads]
        src = a_ci[a_rp[i]:a_rp[i + 1]]
        L = b_rp[src + 1] - b_rp[src]
        plan = heavy_gather_plan(L, shape)
        cells = set(plan["cells"])
        c, sid, pos = _row_entries(b_rp, b_ci, src)
        qc, lane = _quad_cells(c, sid, pos, b_rp, src, nnz_b)
        cells |= qc
        if (src == 0).any() and 1 <= b_rp[1] - b_rp[0] <= 3:
            cells.add("g:B row 0 of 1-3 entries")
        if ((src == b_rp.size - 2) & (L > 0)).any():
            cells.add("g:B's last row")
        prod = np.unique(c)
        fc = np.asarray(f[1][f[0][i]:f[0][i + 1]], np.int64) if f is not None else prod[:0]
        fin = np.unique(fc[(fc >= 0) & (fc < cols)])
        out = {"none": prod, "drop": np.setdiff1d(prod, fin), "insert": np.union1d(prod, fin)}.get(mode, np.intersect1d(prod, fin))
        r = dict(row=int(i), F=int(F[i - r0]), bin=b, kernel=kernel, shape=shape, plan=plan, out=out)
        later = False
        if kernel.startswith("rank"):
            r["rank"] = heavy_rank(prod, fin, cols, mode)
            cells |= r["rank"]["cells"]
            r["held"] = kernel == "rank" and plan["kept"] and plan["QB"] <= shape[0] * shape[2]
            later = not r["held"]
            cells.add("g:held" if r["held"] else "g:not held")
            W = RANK_SPAN
        elif kernel == "count":
            r["windows"], swept, cc = heavy_count_windows(fin, prod, cols)
            cells |= cc
            later = swept > 1
            W = COUNT_MAX_COLS
        else:
            r["readout"] = heavy_readout(out, cols, threads, kernel == "keep")
            cells |= r["readout"]["cells"]
            later = r["readout"]["nwin"] > 1
            W = 64 * r["readout"]["wwords"]
        cells.add("g:plan kept" if plan["kept"] else "g:plan not kept")
        if plan["kept"] and later:
            cells.add("g:plan kept and used")
        if mode != "none" and kernel != "count":
            nw = -(-cols // W)
            pw = np.bincount(prod // W, minlength=nw) > 0
            if (fc >= cols).any():
                cells.add("f:column at or beyond cols")
            if fin.size and (~pw[fin // W]).any():
                cells.add("f:column in a window without a product")
            if fin.size and pw[fin // W].any():
                cells.add("f:column in a window with products")
            if np.intersect1d(prod, fin).size:
                cells.add("f:column that is a product")
            if mode == "drop" and not kernel.startswith("rank"):
                l0 = np.bincount(c[lane == 0] // W, minlength=nw) > 0
                hit = np.bincount(np.intersect1d(prod, fin) // W, minlength=nw) > 0
                if (pw & ~l0 & hit).any():
                    cells.add("f:dropped product in a window fed by lanes 1-3 only")
        if mode == "count" and (fc >= cols).any():
            cells.add("f:column at or beyond cols")
        r["later_sweep"] = bool(later)
        r["cells"] = cells
        rows[int(i)] = r
    return dict(F=F, bins=bins, rows=rows, flen=flen)


# ---- shapes that drive the heavy-row kernels into their edges: heavy_gather_case, heavy_readout_case, heavy_masks ------------
ROW0, EMPTY, LAST = -1, -2, -3          # the shared B rows in a row's source list (_heavy_assemble)
HEAVY_COLS = (6000, (1 << 18) + 1, (1 << 20) + 1, 3 * (1 << 20) + 777)
_READOUT_CYCLE = ("one", "cap", "zero", "cap+1", "pops", "noise", "zero", "full", "one", "zero")
READOUT_VARIANTS = len(_READOUT_CYCLE)


def _heavy_columns(rng, cols, n, lo=0, hi=None):
    """n product columns of [lo, hi) in gather order: distinct while they fit, then one in fifty overwritten by another; unsorted"""
    hi = cols if hi is None else hi
    c = _strata(rng, 1, n, lo, hi)[0] if n <= hi - lo else lo + np.arange(n, dtype=np.int64) % (hi - lo)
    c = rng.permutation(c)
    if n >= 50:
        c[rng.integers(0, n, size=n // 50)] = c[rng.integers(0, n, size=n // 50)]
    return c


def _gather_sources(rng, cols, nsrc, QB, fmin=0, fmax=None, shared=True):
    """the sources of one A row as _heavy_assemble takes them: `nsrc` sources of exactly `QB` quads in all (a quad: four
    entries of one B row or its remainder), fmin <= products <= fmax.  With `shared` (and room): B row 0 first (two
    entries, one quad), the shared empty B row in the middle and B's last row (five entries, two quads) last.  Lengths
    1 .. 8 are present where the row has sources of one and two quads; sources beyond the quads are empty B rows."""
    fixed = shared and nsrc >= 8 and QB >= 8
    m, Q, Ff = (nsrc - 3, QB - 3, 7) if fixed else (nsrc, QB, 0)
    nq = np.zeros(m, np.int64)
    ne = min(m, Q)
    nq[:ne] = 1
    if Q > ne:
        nq[:ne] += rng.multinomial(Q - ne, np.full(ne, 1.0 / ne))
    r = rng.integers(0, 4, size=m)                          # entries the last quad of the source lacks
    r[nq == 0] = 0
    for k in (1, 2):
        idx = np.flatnonzero(nq == k)[:4]
        r[idx] = np.array([3, 2, 1, 0])[:idx.size]
    F = Ff + 4 * int(nq.sum()) - int(r.sum())
    fmax = max(F, fmin) if fmax is None else fmax
    if not fmin <= F <= fmax:
        up = F > fmax                                       # more entries lacking, or fewer
        need = F - fmax if up else fmin - F
        order = rng.permutation(np.flatnonzero(nq > 0))
        room = 3 - r[order] if up else r[order]
        cum = np.cumsum(room)
        k = int(np.searchsorted(cum, need))
        assert k < order.size, "no row of %d sources and %d quads has %d .. %d products" % (nsrc, QB, fmin, fmax)
        r[order[:k + 1]] = 3 if up else 0
        r[order[k]] += -(int(cum[k]) - need) if up else int(cum[k]) - need
    L = (4 * nq - r)[rng.permutation(m)]
    assert fmin <= Ff + int(L.sum()) <= fmax and int((-(-L // 4)).sum()) == Q
    src = np.split(_heavy_columns(rng, cols, int(L.sum())), np.cumsum(L)[:-1])
    return [ROW0] + src[:m // 2] + [EMPTY] + src[m // 2:] + [LAST] if fixed else src


def _quad_sources(rng, cols, quads):
    """sources of exactly the given quad counts (full quads), in this order"""
    L = 4 * np.asarray(quads, np.int64)
    return np.split(_heavy_columns(rng, cols, int(L.sum())), np.cumsum(L)[:-1])


def _heavy_assemble(cols, rows, names, **kw):
    """A and B from per-row source lists.  A source is an int array (a B row of its own: any order, repeats, empty), ROW0 /
    EMPTY / LAST (the shared B rows: row 0 = {cols - 1, 0}, row 1 empty, B's last row of five entries around the last
    column) or ("again", k): source k of the same row once more (a repeated column of A)."""
    b_lens, b_cols = [2, 0], [np.array([cols - 1, 0], np.int64)]
    lists = []
    for srcs in rows:
        ids = []
        for s in srcs:
            if isinstance(s, tuple):
                ids.append(ids[s[1]])
            elif isinstance(s, (int, np.integer)):
                ids.append({ROW0: 0, EMPTY: 1, LAST: -1}[int(s)])
            else:
                ids.append(len(b_lens))
                b_lens.append(s.size)
                b_cols.append(np.asarray(s, np.int64))
        lists.append(np.array(ids, np.int64))
    last = len(b_lens)
    b_lens.append(5)
    b_cols.append(np.array([cols - 1, min(1, cols - 1), cols - 1, min(64, cols - 1), cols // 2], np.int64))
    a_ci = np.concatenate(lists)
    a_ci[a_ci == -1] = last
    a_rp = np.concatenate([[0], np.cumsum([x.size for x in lists])])
    b_rp = np.concatenate([[0], np.cumsum(b_lens)])
    b_ci = np.concatenate(b_cols)
    assert b_ci.min() >= 0 and b_ci.max() < cols and b_rp[-1] < 2**31
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    return dict(a_rp=i32(a_rp), a_ci=i32(a_ci), b_rp=i32(b_rp), b_ci=i32(b_ci), ncols=cols, names=list(names), **kw)


def _light_rows(rng, cols):
    return [[_heavy_columns(rng, cols, 10)], [EMPTY, EMPTY], [], [ROW0, _heavy_columns(rng, cols, 100)]]


def heavy_gather_case(cols, seed):
    """A and B for the gather of the heavy rows (heavy_gather.hpp gather_sweep): per thread shape rows of exact (sources, QB):
    QB mod step in {1, q, q+1, 2q, 2q+1, 3q, 3q+1, 0}; exactly `threads` sources with QB == tile, threads + 1 sources,
    QB == tile + 1; batches without a non-empty source first, in the middle and last; sources that start on the last quad
    of a tile, on quad 0 of the next, that cross a tile boundary; one B row of 2 * tile quads behind a one-quad source, so that
    a whole tile has no start.  Every row's sources are B rows of its own, unsorted with repeats, among them B row 0 (two
    entries), empty B rows and B's last row.  The products of every row fit the class the row is meant for at this column
    count (gen.heavy_model is the authority on where it lands); two more rows lie in the last class."""
    rng = np.random.default_rng(seed)
    mid_cap, rank_cap = _mid_rank_caps(cols)
    rows, names = [], []

    def add(name, srcs):
        rows.append(srcs)
        names.append(name)

    G = lambda *a, **k: _gather_sources(rng, cols, *a, **k)
    empty_batch = lambda T: [EMPTY] * T
    # ---- the rank class (512, 8, 4): at most 6144 products; D of heavy_masks adds up to 16 (Insert bins by F_i + |D_i|)
    if rank_cap:
        lo, hi = HEAVY_MIN + 1, rank_cap - 16
        for QB, nsrc in ((513, 20), (1024, 200), (1025, 300), (1536, 400), (1537, 512), (800, 513), (1900, 512)):
            add("rank QB %d, %d sources" % (QB, nsrc), G(nsrc, QB, lo, hi, shared=QB > 513))   # (513 quads with B row 0: 2047 products)
        add("rank, batches of 512, 1, 0, 700 quads", G(512, 512, shared=False) + G(512, 1, shared=False) + empty_batch(512) + G(300, 700, 700, 2800))
        add("rank, empty batch first", empty_batch(512) + G(300, 900, lo, hi))
        add("rank, empty batch last", G(512, 1000, lo, hi) + empty_batch(512))
        add("rank, 6000 one-entry sources", [c for c in _heavy_columns(rng, cols, 6000).reshape(-1, 1)])
    # ---- the 512-thread window shape: above the rank class, at most mid_cap products
    T, (tile, step, q) = 512, heavy_tile(HEAVY_SHAPES[512])
    lo, hi = max(rank_cap, HEAVY_MIN) + 1, mid_cap
    for r in (1, q, q + 1, 2 * q, 2 * q + 1, 3 * q, 3 * q + 1, step):
        add("win512 QB step + %d" % r, G(300, step + r, lo, hi))
    add("win512 %d sources, QB == tile" % T, G(T, tile, lo, hi))
    add("win512 %d sources" % (T + 1), G(T + 1, tile, lo, hi))
    add("win512 QB == tile + 1", G(400, tile + 1, lo, hi))
    add("win512, empty batch first", empty_batch(T) + G(300, 2500, lo, hi))
    add("win512, empty batch in the middle", G(T, 1200, shared=False) + empty_batch(T) + G(300, 1300, lo - 4800, hi - 4800))
    add("win512, empty batch last", G(T, 2400, lo, hi) + empty_batch(T))
    add("win512, tile-boundary sources", _quad_sources(rng, cols, [tile - 1, 1, 2, 3, tile + 90, 7]))
    add("win512, a tile without a start", [ROW0] + _quad_sources(rng, cols, [2 * tile, 5]) + [LAST])
    # ---- the 1024-thread shape: Keep and Count at any size, None / Drop / Insert above mid_cap
    T, (tile, step, q) = 1024, heavy_tile(HEAVY_SHAPES[1024])
    k = mid_cap // (4 * step) + 1
    k = k if k <= 4 else 2                                  # (above that the rows would cost millions of products: Keep and Count only)
    lo = mid_cap + 1 if 4 * step * k > mid_cap else HEAVY_MIN + 1
    for r in (1, q, q + 1, 2 * q, 2 * q + 1, 3 * q, 3 * q + 1, step):
        add("win1024 QB %d steps + %d" % (k, r), G(700, k * step + r, min(lo, 4 * (k * step + r) - 2200)))
    add("win1024 %d sources, QB == tile" % T, G(T, tile, 4 * tile, shared=False))
    add("win1024 %d sources" % (T + 1), G(T + 1, tile, 4 * tile - 3000))
    add("win1024 QB == tile + 1", G(600, tile + 1, 4 * tile - 1000))
    add("win1024, empty batches first, in the middle and last",
        empty_batch(T) + G(T, 9000, shared=False) + empty_batch(T) + G(500, 8000) + empty_batch(T))
    add("win1024, tile-boundary sources", _quad_sources(rng, cols, [tile - 1, 1, 2, 3, tile + 90, 7]))
    add("win1024, a tile without a start", [ROW0] + _quad_sources(rng, cols, [2 * tile, 5]) + [LAST])
    for j in range(2):                                      # the last class holds at least two rows: the hub-row ordering runs
        s = G(1500, mid_cap // 4 + 900, mid_cap + 1)
        add("hub row %d" % j, s + [("again", 3), ("again", 4)])
    for srcs in _lane_rows(rng, cols):
        add("lane row", srcs)
    mid = len(rows) // 2
    light = _light_rows(rng, cols)
    rows[mid:mid] = light
    names[mid:mid] = ["light"] * len(light)
    # `late` rows (heavy_masks): the rows that keep their plan get a mask without a column below 2^18 -- Count's first product
    # sweep, which builds the plan, then happens in a later window
    return _heavy_assemble(cols, rows, names, lane_rows=[i for i, n in enumerate(names) if n == "lane row"],
                           late_rows=[i for i, n in enumerate(names) if "QB == tile" in n] if cols > COUNT_MAX_COLS else [])


def _pick(rng, lo, hi, n, have):
    """n distinct columns of [lo, hi), those of `have` among them"""
    pool = np.setdiff1d(np.arange(lo, hi, dtype=np.int64), have)
    return np.concatenate([have, rng.permutation(pool)[:n - have.size]])


def _pops_step(rng, lo, nfull, width):
    """the columns of a direct step: one word of each popcount of HEAVY_POPS (as many as the step has whole words, the
    fullest first), two columns in every other whole word: more than stage_cap = 2 * width outputs"""
    if nfull == 0:
        return np.zeros(0, np.int64)
    words = rng.permutation(nfull)
    pops = sorted(HEAVY_POPS, reverse=True)[:nfull]
    out = [lo + 64 * int(w) + rng.permutation(64)[:p] for w, p in zip(words, pops)]
    out += [lo + 64 * int(w) + rng.permutation(64)[:2] for w in words[len(pops):]]
    c = np.concatenate(out)
    return c if c.size > 2 * width else c[:0]


def _readout_output(rng, cols, threads, keep, variant, budget):
    """(S, X): the output row S prescribed per read-out step of the window shape (`threads`, keep) at `cols` columns, and noise
    columns X in steps of their own.  Step t takes the kind _READOUT_CYCLE[(t + variant) % 10]: no output, one, exactly
    stage_cap, stage_cap + 1, a full step, a direct step with words of every popcount of HEAVY_POPS, noise; in random
    order while the budget of distinct columns lasts.  Even variants set the three columns around every window boundary and
    the last column; odd variants set none of them and leave every fourth window empty."""
    wwords, nwin, _ = heavy_window_geometry(cols, threads, keep)
    W = 64 * wwords
    nsteps = -(-wwords // READOUT_STEP_WORDS)
    pre = np.zeros(0, np.int64)
    if variant % 2 == 0:
        pre = np.concatenate([np.arange(1, nwin) * W + d for d in (-1, 0, 1)] + [[cols - 1]]).astype(np.int64)
        pre = np.unique(pre[(pre >= 0) & (pre < cols)])
    S, X, spent, placed = [pre], [], pre.size, np.zeros(pre.size, bool)
    for t in rng.permutation(nwin * nsteps):
        win, st = divmod(int(t), nsteps)
        w0 = st * READOUT_STEP_WORDS
        width = min(READOUT_STEP_WORDS, wwords - w0)
        lo = win * W + 64 * w0
        hi = min(lo + 64 * width, cols)
        if hi <= lo or (nwin > 1 and variant % 2 == 1 and (win + variant // 2) % 4 == 3):
            continue
        have = pre[(pre >= lo) & (pre < hi)]
        kind = _READOUT_CYCLE[(int(t) + variant) % READOUT_VARIANTS]
        if kind == "pops":
            c = _pops_step(rng, lo, (hi - lo) // 64, width)
        else:
            n = {"zero": 0, "one": 1, "cap": 2 * width, "cap+1": 2 * width + 1, "full": 64 * width, "noise": min(40, hi - lo)}[kind]
            if n > hi - lo or n < have.size:
                continue
            c = _pick(rng, lo, hi, n, have)
        if spent + c.size > budget:
            continue
        spent += c.size
        (X if kind == "noise" else S).append(c)
    return np.unique(np.concatenate(S)), np.unique(np.concatenate(X)) if X else pre[:0]


def _sources_from_output(rng, cols_out, F):
    """sources whose products are exactly the columns `cols_out`, F of them (repeats fill up), unsorted, in B rows of mixed lengths"""
    c = rng.permutation(cols_out[np.arange(F) % cols_out.size])
    nsrc = max(2, min(200, F // 40))
    L = rng.multinomial(F - nsrc, np.full(nsrc, 1.0 / nsrc)) + 1
    L[0] += L[1] - 1                                        # one long source, one of one entry
    L[1] = 1
    src = np.split(c, np.cumsum(L)[:-1])
    return src[:nsrc // 2] + [EMPTY] + src[nsrc // 2:] + [("again", 2)]


def _rank_output(rng, cols, nslots, variant):
    """the product columns of a rank row: `nslots` 32-column words in span `variant % spans` (a whole 1024-column top word
    among them, whole 32-column slots, 2100 products or nslots + 50), and in the other spans five columns each or none"""
    nspans = -(-cols // RANK_SPAN)
    sp = variant % nspans
    lo = sp * RANK_SPAN
    hi = min(lo + RANK_SPAN, cols)
    if hi - lo < 32 * nslots + 2048:                        # (a last span of a few columns: take the first)
        sp, lo, hi = 0, 0, min(RANK_SPAN, cols)
    nw = (hi - lo) // 32
    g = int(rng.integers(0, nw // 32)) * 32
    words = np.concatenate([np.arange(g, g + 32), rng.permutation(np.setdiff1d(np.arange(nw), np.arange(g, g + 32)))[:nslots - 32]])
    bits = np.ones(nslots, np.int64)
    extra = max(2100, nslots + 50) - nslots
    nfull = min(extra // 31, nslots - 1)
    bits[:nfull] = 32
    bits[nfull] += min(extra - 31 * nfull, 30)
    bits = rng.permutation(bits)
    out = [lo + 32 * int(w) + rng.permutation(32)[:b] for w, b in zip(words, bits)]
    if (variant // nspans) % 2 == 0:
        for s in range(nspans):
            if s != sp:
                s_lo, s_hi = s * RANK_SPAN, min((s + 1) * RANK_SPAN, cols)
                out.append(np.unique(np.concatenate([rng.integers(s_lo, s_hi, size=5), [s_hi - 1, s_lo]])))
    return np.unique(np.concatenate(out))


RANK_SLOT_TARGETS = (70, 400, 900, 1300, 2000, 2500, 3000, 3500, 4000, 4500, 5000, 5500, 6000)   # spt 1, 1, 2 .. 12


def heavy_readout_case(cols, seed):
    """A and B whose heavy rows have their OUTPUT prescribed: per window shape (512 threads, 1024 threads, Keep's windows)
    READOUT_VARIANTS rows from _readout_output, sized into the class that takes the shape at this column count (repeats fill
    the products up); and rank rows of RANK_SLOT_TARGETS slots (_rank_output) where the class exists.  `sx` maps a row to
    its (S, X), `made_for` to the shape it was built for: heavy_masks gives Keep's rows the mask S, the others X."""
    rng = np.random.default_rng(seed)
    mid_cap, rank_cap = _mid_rank_caps(cols)
    rows, names, sx, made_for, variant = [], [], {}, {}, {}
    lo512 = max(rank_cap, HEAVY_MIN) + 1
    plans = [("win512", 512, False, READOUT_VARIANTS, lo512 + 40, mid_cap - 1000),
             ("win1024", 1024, False, READOUT_VARIANTS if mid_cap < 200000 else 4, mid_cap + 1, mid_cap + 30000),
             ("keep", 1024, True, READOUT_VARIANTS, HEAVY_MIN + 40, 60000)]
    for name, threads, keep, nvar, fmin, fmax in plans:
        for v in range(nvar):
            S, X = _readout_output(rng, cols, threads, keep, v, fmax - 100)
            if S.size + X.size == 0:                        # (one step in all, and its turn is "no output": a heavy row has one)
                S = np.array([cols // 3], np.int64)
            out = np.union1d(S, X)
            sx[len(rows)], made_for[len(rows)], variant[len(rows)] = (S, X), name, v
            rows.append(_sources_from_output(rng, out, max(fmin, out.size + 30)))
            names.append("%s variant %d" % (name, v))
    if rank_cap:
        for v, ns in enumerate(RANK_SLOT_TARGETS):
            rows.append(_sources_from_output(rng, _rank_output(rng, cols, ns, v), max(2100, ns + 50) + 20))
            names.append("rank %d slots" % ns)
    mid = len(rows) // 2
    light = _light_rows(rng, cols)
    rows[mid:mid] = light
    names[mid:mid] = ["light"] * len(light)
    shift = lambda d: {(i if i < mid else i + len(light)): x for i, x in d.items()}
    return _heavy_assemble(cols, rows, names, sx=shift(sx), made_for=shift(made_for), variant=shift(variant))


def _lane_rows(rng, cols):
    """two rows for Drop whose windows above the first receive products in lanes 1 to 3 of their quads only: every B row is
    whole quads whose first entry lies below 2^18 (2^20 for the row of the 1024-thread shape) and whose others lie above"""
    mid_cap, rank_cap = _mid_rank_caps(cols)
    out = []
    for W, F in ((1 << 18, max(rank_cap, HEAVY_MIN) + 2000), (1 << 20, mid_cap + 2000)):
        if cols <= W + 64 or (W == 1 << 18 and F > mid_cap):
            continue
        n = -(-F // 4)
        quad = np.stack([_heavy_columns(rng, cols, n, 0, W)] + [_heavy_columns(rng, cols, n, W, cols) for _ in range(3)], axis=1)
        out.append(np.split(quad.ravel(), [4 * (n // 3), 4 * (n // 2)]))
    return out


def heavy_masks(s, seed):
    """The mask F (f_rp, f_ci: Keep, Drop, Count) and D (d_rp, d_ci: Insert) of a heavy case, from its product pattern.
    F's row: the row's product columns X (rows with `sx` made for Keep: S; the others half of the products; lane rows: the
    products from 2^18 on; `late` rows, for Count: none below 2^18), one column in a window without a product per window
    width (2^18, 2^19, 2^20), columns at and beyond B.cols, some entries twice, and -- rows of at most 8192 products and
    every other row -- columns at or beyond B.cols up to 2100 stored entries, so that Keep and Count send the row to the window kernels.
    D's row: at most 16 entries: three products, a column per empty window, the last column, columns beyond, one twice."""
    rng = np.random.default_rng(seed)
    cols = s["ncols"]
    a_rp, b_rp = s["a_rp"].astype(np.int64), s["b_rp"].astype(np.int64)
    R = a_rp.size - 1
    F = row_products(a_rp, s["a_ci"], b_rp, 0, R)
    frows, drows = [], []
    for i in range(R):
        prod = np.unique(_row_entries(b_rp, s["b_ci"], s["a_ci"][a_rp[i]:a_rp[i + 1]].astype(np.int64))[0])
        if F[i] <= HEAVY_MIN:
            frows.append(prod[:3])
            drows.append(np.array([cols - 1, cols], np.int64))
            continue
        if i in s.get("sx", {}):
            inr = s["sx"][i][0] if s["made_for"][i] == "keep" else s["sx"][i][1]
        elif i in s.get("lane_rows", ()):
            inr = prod[prod >= (1 << 18)]
        else:
            inr = rng.permutation(prod)[:(prod.size + 1) // 2]
        if i in s.get("late_rows", ()):
            inr = inr[inr >= COUNT_MAX_COLS]
        empties = []
        for W in (1 << 18, 1 << 19, 1 << 20):
            nw = -(-cols // W)
            free = np.flatnonzero(np.bincount(prod // W, minlength=nw) == 0)
            if free.size:
                w = int(free[rng.integers(0, free.size)])
                empties.append(int(rng.integers(w * W, min((w + 1) * W, cols))))
        beyond = np.array([cols, cols + 1, cols + (1 << 18), INT_MAX - 1], np.int64)
        row = np.concatenate([inr, np.array(empties, np.int64), beyond])
        row = np.concatenate([row, row[rng.integers(0, row.size, size=5)]])
        if (F[i] <= MASK_WAVE_MAX_PRODUCTS or i % 2 == 0) and row.size < 2100:
            row = np.concatenate([row, rng.integers(cols, INT_MAX, size=2100 - row.size)])
        frows.append(rng.permutation(row))
        d = np.concatenate([rng.permutation(prod)[:3], np.array(empties, np.int64), [cols - 1, cols, cols + 7, INT_MAX - 1]])
        if s.get("variant", {}).get(i, 0) % 2 == 1:         # (the odd variants keep their prescribed output under Insert)
            d = np.concatenate([rng.permutation(prod)[:3], [cols, cols + 7, INT_MAX - 1]])
        drows.append(rng.permutation(np.concatenate([d, d[:1]])))
    out = dict(s)
    for key, rws in (("f", frows), ("d", drows)):
        out[key + "_rp"] = np.concatenate([[0], np.cumsum([r.size for r in rws])]).astype(np.int32)
        out[key + "_ci"] = np.concatenate(rws).astype(np.int32)
    return out
