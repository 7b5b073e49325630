"""bspgemm_multiply_masked_dot on the GPU against the scipy model (tests/dot_ref.py): row_ptr, col_idx and values compared
completely, every shape under dot_light = 0 (every entry with two non-empty rows goes to the one-wave-per-entry kernel),
the default and 2^30 (none does), with info.heavy_entries asserted accordingly.  The shapes are the smallest at which
each piece can go wrong: every shorter-row length 0 .. 130 with each kind of intersection, shorter rows at the edges of
one and two trips of the one-wave kernel, deep heavy entries, the tile
edges of the entry walk (kSelTile = 4096), rectangular operands, non-canonical input, wrapped arrays off 16-byte
alignment, empty operands, one handle in all three roles, equivalence with the counting product, determinism, errors and
the result object."""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import dot_ref
import gen
import ktruss_ref
import lcc_ref
from dot_ref import csr

pytestmark = pytest.mark.gpu

SKEW = (0.57, 0.19, 0.19, 0.05)
NEVER = 1 << 30
VP = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _diff(got, exp, what):
    for name, g, e in zip(("row_ptr", "col_idx", "values"), got, exp):
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape:
            return "%s: %s has %d entries, expected %d" % (what, name, g.size, e.size)
        if not np.array_equal(g, e):
            k = int(np.flatnonzero(g != e)[0])
            return "%s: %s differs first at %d: got %d, expected %d (%d differ)" % (what, name, k, g[k], e[k],
                                                                                   int((g != e).sum()))
    return None


def _download(Cr):
    rp, ci = Cr.download()
    v = Cr.download_values()
    Cr.free()
    return rp, ci, v


def _sweep(ctx, A, B, Fm, exp, heavy0, entries, what, canon=0):
    """the call under the three settings of the knob; returns the failures"""
    bad = []
    default = ctx.get_option("dot_light")
    try:
        for T in (0, default, NEVER):
            ctx.set_option("dot_light", T)
            assert ctx.get_option("dot_light") == T
            Cr, info = ctx.multiply_masked_dot(A, B, Fm)
            assert Cr.rows == A.rows
            got = _download(Cr)
            tag = "%s, dot_light %d" % (what, T)
            d = _diff(got, exp, tag)
            if d:
                bad.append(d)
            if info["entries"] != entries or info["kept"] != exp[1].size or info["canonicalised"] != canon:
                bad.append("%s: info %r, expected entries %d kept %d canonicalised %d" % (tag, info, entries, exp[1].size, canon))
            if T == 0 and info["heavy_entries"] != heavy0:
                bad.append("%s: %d heavy entries, expected %d" % (tag, info["heavy_entries"], heavy0))
            if T == NEVER and info["heavy_entries"] != 0:
                bad.append("%s: %d heavy entries, expected none" % (tag, info["heavy_entries"]))
            if not 0 <= info["heavy_entries"] <= heavy0:
                bad.append("%s: %d heavy entries outside [0, %d]" % (tag, info["heavy_entries"], heavy0))
    finally:
        ctx.set_option("dot_light", default)
    return bad


def _check(ctx, a, b, f, a_rows, b_rows, cols, f_cols, what, canon=0):
    exp = dot_ref.dot_ref(a, b, f, a_rows, b_rows, cols, f_cols)
    heavy0, entries = dot_ref.heavy_at_zero(a, b, f, a_rows, b_rows, cols, f_cols)
    A, B, Fm = ctx.upload(a[0], a[1], cols), ctx.upload(b[0], b[1], cols), ctx.upload(f[0], f[1], f_cols)
    assert (A.rows, B.rows, Fm.rows) == (a_rows, b_rows, a_rows)
    try:
        return _sweep(ctx, A, B, Fm, exp, heavy0, entries, what, canon)
    finally:
        for h in (A, B, Fm):
            h.free()


def _rand_rows(rng, lens, ncols):
    return [np.sort(rng.choice(ncols, size=int(k), replace=False)).tolist() for k in lens]


def _at(exp, i, j):
    """the value of entry (i, j) of a (row_ptr, col_idx, values) result, 0 when it is not stored"""
    lo, hi = int(exp[0][i]), int(exp[0][i + 1])
    hit = np.flatnonzero(exp[1][lo:hi] == j)
    return int(exp[2][lo + hit[0]]) if hit.size else 0


# ---------------------------------------------------------------- 1. length sweep ------------------------------------
def _row_pair(kind, m, top, rng):
    """a shorter row of m entries and a longer one of m + 3 with the given kind of intersection; every column below top"""
    evens, odds = list(range(2, 2 * m + 2, 2)), list(range(3, 2 * (m + 3) + 3, 2))
    if kind == "empty":
        return evens, odds
    if kind == "first":                                 # only the first element of both rows
        return ([0] + evens[1:]) if m else [], [0] + odds[1:]
    if kind == "last":                                  # only the last element of both rows
        return (evens[:-1] + [top]) if m else [], odds[:-1] + [top]
    if kind == "all":                                   # every element of the shorter row
        return [odds[t] for t in np.sort(rng.choice(m + 3, size=m, replace=False))], odds
    return evens, evens                                 # "equal": the same row on both sides


def _length_sweep():
    """mask entries (r, r): the shorter row has m = 0 .. 130 entries, the longer one m + 3 (A the shorter for even m, B for
    odd m), five kinds of intersection each"""
    rng = np.random.default_rng(7101)
    top = 2 * 140 + 1
    a_rows, b_rows = [], []
    for kind in ("empty", "first", "last", "all", "equal"):
        for m in range(131):
            short, long_ = _row_pair(kind, m, top, rng)
            a_short = m % 2 == 0
            a_rows.append(short if a_short else long_)
            b_rows.append(long_ if a_short else short)
    n = len(a_rows)
    return csr(a_rows), csr(b_rows), csr([[r] for r in range(n)]), n, top + 1


def test_length_sweep(ctx):
    a, b, f, n, cols = _length_sweep()
    exp = dot_ref.dot_ref(a, b, f, n, n, cols, n)
    la, lb = np.diff(a[0]), np.diff(b[0])
    shorter = np.minimum(la, lb)
    assert set(shorter.tolist()) >= set(range(131))
    assert exp[2].max() == 130 and (exp[2] == 1).sum() >= 2 * 130     # every element / one element
    bad = _check(ctx, a, b, f, n, n, cols, n, "length sweep")
    assert not bad, bad


def test_deep_trip_edges(ctx):
    """the shorter row ends one element before, at and one element behind one and two trips of the one-wave kernel (64
    lanes times the 4 steps in flight, lcc_ref.K_DEEP): kinds "all" and "empty" of the length sweep, either operand the
    shorter"""
    rng = np.random.default_rng(7102)
    trip = 64 * lcc_ref.K_DEEP
    ms = [t * trip + d for t in (1, 2) for d in (-1, 0, 1)]
    assert ms == [255, 256, 257, 511, 512, 513]
    a_rows, b_rows, hits = [], [], []
    for kind in ("all", "empty"):
        for m in ms:
            for a_short in (True, False):
                short, long_ = _row_pair(kind, m, None, rng)
                a_rows.append(short if a_short else long_)
                b_rows.append(long_ if a_short else short)
                hits.append(m if kind == "all" else 0)
    n, cols = len(a_rows), 2 * (ms[-1] + 3) + 3
    assert n == 24 and cols < 1100
    a, b, f = csr(a_rows), csr(b_rows), csr([[r] for r in range(n)])
    exp = dot_ref.dot_ref(a, b, f, n, n, cols, n)
    assert [_at(exp, r, r) for r in range(n)] == hits
    assert dot_ref.heavy_at_zero(a, b, f, n, n, cols, n) == (n, n)     # every entry goes to the one-wave kernel at dot_light 0
    bad = _check(ctx, a, b, f, n, n, cols, n, "deep trip edges")
    assert not bad, bad


# ---------------------------------------------------------------- 2. deep heavy entries ------------------------------
def test_deep_heavy_entries(ctx):
    rng = np.random.default_rng(7201)
    cols = 20000
    long_ = np.sort(rng.choice(cols, 5000, replace=False))
    a_rows = []
    for k in (64, 65, 1000):                                          # half of each short row inside the long one
        inside = rng.choice(long_, k // 2, replace=False)
        outside = rng.choice(np.setdiff1d(np.arange(cols), long_), k - k // 2, replace=False)
        a_rows.append(np.sort(np.concatenate([inside, outside])).tolist())
    both = rng.choice(cols, 4500, replace=False)                      # two rows of 3000 that share 1500
    a_rows.append(np.sort(both[:3000]).tolist())
    b_rows = [long_.tolist(), np.sort(both[1500:]).tolist(), a_rows[2]]
    a, b = csr(a_rows), csr(b_rows)
    f = csr([[0, 1, 2]] * 4)
    exp = dot_ref.dot_ref(a, b, f, 4, 3, cols, 3)
    assert [_at(exp, i, 0) for i in range(3)] == [32, 32, 500] and _at(exp, 3, 1) == 1500 and _at(exp, 2, 2) == 1000
    bad = _check(ctx, a, b, f, 4, 3, cols, 3, "deep heavy entries")
    bad += _check(ctx, b, a, csr([[0, 1, 2, 3]] * 3), 3, 4, cols, 4, "deep heavy entries, swapped")   # the longer row is A's
    assert not bad, bad


# ---------------------------------------------------------------- 3. tile edges of the walk --------------------------
def _mask_of(rng, lens, b_rows):
    return csr(_rand_rows(rng, lens, b_rows))


@pytest.mark.parametrize("nnz_f", [4095, 4096, 4097, 8193])
def test_tile_edges_by_nnz(ctx, nnz_f):
    rng = np.random.default_rng(7300 + nnz_f)
    b_rows, cols, per = 60, 48, 7
    full, rest = divmod(nnz_f, per)
    lens = [per] * full + ([rest] if rest else [])
    n = len(lens)
    a = csr(_rand_rows(rng, rng.integers(0, 9, n), cols))
    b = csr(_rand_rows(rng, rng.integers(0, 20, b_rows), cols))
    f = _mask_of(rng, lens, b_rows)
    assert f[1].size == nnz_f
    bad = _check(ctx, a, b, f, n, b_rows, cols, b_rows, "nnz(F) = %d" % nnz_f)
    assert not bad, bad


def test_tile_edges_by_rows(ctx):
    """one mask row of 5000 entries spanning two tiles; more than 4096 empty mask rows inside one tile (its window of
    row_ptr is not staged); leading and trailing empty rows"""
    rng = np.random.default_rng(7350)
    b_rows, cols = 6000, 64
    lens = [0] * 5 + [3, 5000, 2] + [0] * 4200 + [9, 1, 0, 40] + [0] * 7
    n = len(lens)
    a_len = rng.integers(1, 12, n)
    a_len[6] = 30                                                     # the hub mask row: heavy under the default too
    a = csr(_rand_rows(rng, a_len, cols))
    b = csr(_rand_rows(rng, rng.integers(0, 40, b_rows), cols))
    f = _mask_of(rng, lens, b_rows)
    assert f[0][6] <= 4096 < f[0][7] and n - 6 > 4096                # the second tile begins in row 6 and spans the rest
    bad = _check(ctx, a, b, f, n, b_rows, cols, b_rows, "hub mask row and a run of empty rows")
    assert not bad, bad


# ---------------------------------------------------------------- 4. rectangular operands ----------------------------
def test_rectangular_operands(ctx):
    """A 37 x 50, B 23 x 50, F 37 x 29: the mask entries with j >= 23 are dropped; empty rows on either side"""
    rng = np.random.default_rng(7401)
    a_len, b_len = rng.integers(1, 30, 37), rng.integers(1, 30, 23)
    a_len[[0, 11, 36]] = 0
    b_len[[0, 7, 22]] = 0
    a, b = csr(_rand_rows(rng, a_len, 50)), csr(_rand_rows(rng, b_len, 50))
    f = csr(_rand_rows(rng, rng.integers(10, 29, 37), 29))
    assert (f[1] >= 23).sum() > 20
    exp = dot_ref.dot_ref(a, b, f, 37, 23, 50, 29)
    assert exp[1].max() < 23 and exp[1].size > 100
    bad = _check(ctx, a, b, f, 37, 23, 50, 29, "rectangular")
    # a mask whose every entry is at or above B.rows
    bad += _check(ctx, a, b, csr([[23, 28]] * 37), 37, 23, 50, 29, "mask beyond B.rows")
    assert not bad, bad


# ---------------------------------------------------------------- 5. non-canonical input -----------------------------
def _noisy(rng, rows, unsorted=True, repeats=True):
    out = []
    for r in rows:
        r = list(r)
        if repeats and r:
            r = r + [r[int(k)] for k in rng.integers(0, len(r), max(1, len(r) // 3))]
            r.sort()
        if unsorted:
            r = [r[int(k)] for k in rng.permutation(len(r))]
        out.append(r)
    return out


def test_non_canonical_input(ctx):
    rng = np.random.default_rng(7501)
    n, m, cols = 300, 200, 90
    ra = _rand_rows(rng, rng.integers(2, 40, n), cols)
    rb = _rand_rows(rng, rng.integers(2, 40, m), cols)
    rf = _rand_rows(rng, rng.integers(2, 25, n), m)
    a, b, f = csr(ra), csr(rb), csr(rf)
    na = csr(_noisy(rng, ra, unsorted=False))                         # A: sorted rows with repeats
    nb = csr(_noisy(rng, rb, repeats=False))                          # B: unsorted
    nf = csr(_noisy(rng, rf))                                         # F: unsorted with repeats
    assert na[1].size > a[1].size and nf[1].size > f[1].size and nb[1].size == b[1].size
    bad = _check(ctx, a, b, f, n, m, cols, m, "canonical", canon=0)
    bad += _check(ctx, na, b, f, n, m, cols, m, "A with repeats", canon=1)
    bad += _check(ctx, a, nb, f, n, m, cols, m, "B unsorted", canon=2)
    bad += _check(ctx, a, b, nf, n, m, cols, m, "F unsorted with repeats", canon=4)
    bad += _check(ctx, na, nb, nf, n, m, cols, m, "all three", canon=7)
    assert not bad, bad
    # one non-canonical handle in all three roles: every bit
    rs = _noisy(rng, _rand_rows(rng, rng.integers(1, 30, 120), 120))
    s = csr(rs)
    S = ctx.upload(s[0], s[1], 120)
    exp = dot_ref.dot_ref(s, s, s, 120, 120, 120, 120)
    heavy0, entries = dot_ref.heavy_at_zero(s, s, s, 120, 120, 120, 120)
    bad = _sweep(ctx, S, S, S, exp, heavy0, entries, "one noisy handle", canon=7)
    S.free()
    assert not bad, bad


# ---------------------------------------------------------------- 6. wrapped device arrays ---------------------------
def test_wrapped_arrays_off_alignment(ctx):
    """each of A, B and F in turn as wrapped device arrays whose col_idx is one int off 16-byte alignment"""
    import torch
    rng = np.random.default_rng(7601)
    n, m, cols = 700, 90, 80
    a = csr(_rand_rows(rng, rng.integers(0, 30, n), cols))
    b = csr(_rand_rows(rng, rng.integers(0, 30, m), cols))
    f = csr(_rand_rows(rng, rng.integers(5, 10, n), m))
    assert f[1].size > 4096
    exp = dot_ref.dot_ref(a, b, f, n, m, cols, m)
    heavy0, entries = dot_ref.heavy_at_zero(a, b, f, n, m, cols, m)

    def wrap(x, rows, ncols):
        trp = torch.from_numpy(x[0]).cuda()
        buf = torch.zeros(x[1].size + 4, dtype=torch.int32, device="cuda")
        buf[1:1 + x[1].size] = torch.from_numpy(x[1]).cuda()
        torch.cuda.synchronize()
        tci = buf[1:]
        assert tci.data_ptr() % 16 == 4
        return ctx.wrap_device(rows, ncols, x[1].size, trp.data_ptr(), tci.data_ptr(), keep=(trp, buf))

    bad = []
    for role in range(3):
        hs = [wrap(x, r, c) if k == role else ctx.upload(x[0], x[1], c)
              for k, (x, r, c) in enumerate(((a, n, cols), (b, m, cols), (f, n, m)))]
        bad += _sweep(ctx, hs[0], hs[1], hs[2], exp, heavy0, entries, "wrapped %s" % "ABF"[role])
        for h in hs:
            h.free()
    assert not bad, bad


# ---------------------------------------------------------------- 7. empty cases -------------------------------------
def test_empty_cases(ctx):
    rng = np.random.default_rng(7701)
    n, m, cols = 50, 40, 30
    a = csr(_rand_rows(rng, rng.integers(1, 10, n), cols))
    b = csr(_rand_rows(rng, rng.integers(1, 10, m), cols))
    f = csr(_rand_rows(rng, rng.integers(1, 10, n), m))
    none_n, none_m, none_0 = csr([[]] * n), csr([[]] * m), csr([])
    bad = _check(ctx, a, b, none_n, n, m, cols, m, "nnz(F) = 0")
    bad += _check(ctx, none_n, b, f, n, m, cols, m, "nnz(A) = 0")
    bad += _check(ctx, a, none_m, f, n, m, cols, m, "nnz(B) = 0")
    bad += _check(ctx, none_0, b, none_0, 0, m, cols, m, "A.rows = 0")
    bad += _check(ctx, a, none_0, f, n, 0, cols, m, "B.rows = 0")
    assert not bad, bad


# ---------------------------------------------------------------- 8. one handle, equivalence, determinism ------------
def test_one_handle_in_three_roles(ctx):
    rp, ci, n = gen.rmat(10, 8, SKEW, 7801)
    s = ktruss_ref.symmetrise(rp, ci, n)
    S = ctx.upload(s[0], s[1], n)
    exp = dot_ref.dot_ref(s, s, s, n, n, n, n)
    heavy0, entries = dot_ref.heavy_at_zero(s, s, s, n, n, n, n)
    assert entries == s[1].size and int(np.diff(s[0]).max()) > 64
    bad = _sweep(ctx, S, S, S, exp, heavy0, entries, "A = B = F, one handle")
    S.free()
    assert not bad, bad


def test_equals_the_counting_product_and_is_deterministic(ctx):
    """the skewed R-MAT scale 13 graph of test_gpu_masked_count.py, F = A: bit-equal to multiply_masked_count(A, B^T, F);
    two runs give equal results"""
    rp, ci, n = gen.rmat(13, 16, SKEW, 1601)
    A = ctx.upload(rp, ci, n)
    Bt = ctx.transpose(A)
    Cc = ctx.multiply_masked_count(A, Bt, A)
    exp = _download(Cc)
    runs = []
    for _ in range(2):
        Cr, info = ctx.multiply_masked_dot(A, A, A)
        runs.append((_download(Cr), info))
    assert exp[1].size > 10000 and runs[0][1]["heavy_entries"] > 0 and runs[0][1]["canonicalised"] == 0
    assert not _diff(runs[0][0], exp, "dot against the counting product")
    assert not _diff(runs[1][0], runs[0][0], "second run") and runs[1][1] == runs[0][1]
    for h in (Bt, A):
        h.free()


# ---------------------------------------------------------------- 9. errors ------------------------------------------
def test_errors_leave_nothing_and_the_context_usable(ctx):
    L = bspgemm.lib()
    rng = np.random.default_rng(7901)
    n, m, cols = 30, 20, 25
    a = csr(_rand_rows(rng, rng.integers(1, 10, n), cols))
    b = csr(_rand_rows(rng, rng.integers(1, 10, m), cols))
    f = csr(_rand_rows(rng, rng.integers(1, 10, n), m))
    exp = dot_ref.dot_ref(a, b, f, n, m, cols, m)
    A, B, Fm = ctx.upload(a[0], a[1], cols), ctx.upload(b[0], b[1], cols), ctx.upload(f[0], f[1], m)
    other = bspgemm.Context(0)
    foreign = other.upload(a[0], a[1], cols)
    wide = ctx.upload(b[0], b[1], cols + 1)                           # A.cols != B.cols
    short = ctx.upload(f[0][:n], f[1][:f[0][n - 1]], m)               # F.rows != A.rows
    f_bad = (f[0], f[1].copy())
    f_bad[1][3] = m                                                   # a column of F outside [0, F.cols)
    f_neg = (f[0], f[1].copy())
    f_neg[1][0] = -1
    a_bad = (a[0], a[1].copy())
    a_bad[1][-1] = cols                                               # a column of A outside [0, cols)
    Fbad, Fneg, Abad = ctx.upload(f_bad[0], f_bad[1], m), ctx.upload(f_neg[0], f_neg[1], m), ctx.upload(a_bad[0], a_bad[1], cols)

    def call(c, x, y, z, flags=0, out=True):
        r, info = VP(0x5A5A), bspgemm.DotInfo(1, 1, 1, 1)
        st = L.bspgemm_multiply_masked_dot(c, x, y, z, flags, C.byref(r) if out else None, C.byref(info))
        return st, r, L.bspgemm_last_error().decode(errors="replace")

    def good(what):
        Cr, info = ctx.multiply_masked_dot(A, B, Fm)
        d = _diff(_download(Cr), exp, what)
        assert not d, d

    cases = [("NULL ctx", (None, A._h, B._h, Fm._h), {}, "NULL"), ("NULL A", (ctx._h, None, B._h, Fm._h), {}, "NULL"),
             ("NULL B", (ctx._h, A._h, None, Fm._h), {}, "NULL"), ("NULL F", (ctx._h, A._h, B._h, None), {}, "NULL"),
             ("flags", (ctx._h, A._h, B._h, Fm._h), {"flags": 1}, "flags"),
             ("foreign A", (ctx._h, foreign._h, B._h, Fm._h), {}, "another context"),
             ("foreign B", (ctx._h, A._h, foreign._h, Fm._h), {}, "another context"),
             ("foreign F", (ctx._h, A._h, B._h, foreign._h), {}, "another context"),
             ("A.cols != B.cols", (ctx._h, A._h, wide._h, Fm._h), {}, "A.cols"),
             ("F.rows != A.rows", (ctx._h, A._h, B._h, short._h), {}, "F.rows"),
             ("F column = F.cols", (ctx._h, A._h, B._h, Fbad._h), {}, "operand F"),
             ("F column < 0", (ctx._h, A._h, B._h, Fneg._h), {}, "operand F"),
             ("A column = A.cols", (ctx._h, Abad._h, B._h, Fm._h), {}, "operand A")]
    for what, args, kw, word in cases:
        st, r, msg = call(*args, **kw)
        assert st == 1, "%s: status %d (%s)" % (what, st, msg)
        assert r.value is None, "%s: *C is %r, not NULL" % (what, r.value)
        assert "bspgemm_multiply_masked_dot" in msg and word in msg, (what, msg)
        good("after " + what)
    st, _, msg = call(ctx._h, A._h, B._h, Fm._h, out=False)
    assert st == 1 and "bspgemm_multiply_masked_dot" in msg and "NULL" in msg
    good("after NULL C")
    # the loops' own errors
    T = VP(1)
    assert L.bspgemm_ktruss_ex(ctx._h, A._h, 4, 0, 1, C.byref(T), None, None) == 1 and not T.value      # not square
    assert L.bspgemm_ktruss_ex(ctx._h, A._h, 4, 0, 7, C.byref(T), None, None) == 1 and not T.value      # unknown method
    tri = C.c_int64(-3)
    assert L.bspgemm_triangle_count_ex(ctx._h, A._h, 1, C.byref(tri)) == 1 and tri.value == -3
    assert L.bspgemm_triangle_count_ex(ctx._h, A._h, 5, C.byref(tri)) == 1 and tri.value == -3
    with pytest.raises(bspgemm.BspgemmError):
        ctx.set_option("dot_light", -1)
    good("after the loops' errors")
    for h in (A, B, Fm, wide, short, Fbad, Fneg, Abad, foreign):
        h.free()
    other.close()


# ---------------------------------------------------------------- 10. the result object ------------------------------
def test_result_object(ctx):
    rp, ci, n = gen.rmat(9, 8, SKEW, 8001)
    s = ktruss_ref.symmetrise(rp, ci, n)
    S = ctx.upload(s[0], s[1], n)
    exp = dot_ref.dot_ref(s, s, s, n, n, n, n)
    Cr, info = ctx.multiply_masked_dot(S, S, S)
    assert Cr.rows == n and Cr.nnz == exp[1].size == info["kept"] and Cr.values_device
    rp64, cols = Cr.download()
    vals = Cr.download_values()
    assert rp64.dtype == np.int64 and not _diff((rp64, cols, vals), exp, "result object")
    assert Cr.values_sum() == int(exp[2].sum())
    c = int(np.bincount(exp[2]).argmax())
    W = ctx.matrix_from_result_where(Cr, n, "==", c)
    assert not _diff(W.download(), ktruss_ref.where_ref(exp[0], exp[1], exp[2], "==", c), "from_result_where(EQ)")
    M = ctx.matrix_from_result(Cr, n)
    assert not _diff(M.download(), (exp[0].astype(np.int32), exp[1]), "matrix_from_result")
    for h in (W, M):
        h.free()
    Cr.free()
    Cr2, _ = ctx.multiply_masked_dot(S, S, S)                         # (the freed buffers come back from the cache)
    assert not _diff(_download(Cr2), exp, "after free")
    S.free()
