"""The masked product C = F .* (A*B) (bspgemm_multiply_masked, Context.multiply_masked, the drop-in SpGEMM_hip_masked) under
masks that hold columns at or above B.cols: include/bspgemm.h lets F have any number of columns and says that such entries
have no effect.  Every one-wave Keep instance (three depths x seven mask-row capacities) and the Keep window kernel get rows
whose masks hold B.cols itself, columns within and beyond the top bitmap / the last window, aliases p + k * span of product
columns p that are NOT in the mask (a kernel that truncated or wrapped the index would keep p), p + 2^30 and 2^31 - 1.

The reference is independent of the library and of the masked oracle (which indexes a flag array of B.cols entries with
the mask's columns): the rows of the oracle's plain product intersected with F's (row, column) keys.  The mask's part
within [0, B.cols) goes through the masked oracle too, which must agree.  tests/test_masked_shapes.py shows without a GPU
that the inputs (tests/gen.py masked_one_wave_case, masked_window_case) reach every kernel instance.
"""
import numpy as np
import pytest

import bspgemm
import gen
from oracle import oracle as O

pytestmark = pytest.mark.gpu
INT_MAX = gen.INT_MAX
CASES = [("wave", c) for c in gen.MASK_ONE_WAVE_COLS] + [("window", c) for c in gen.MASK_WINDOW_COLS]
_ids = ["%s_%d" % k for k in CASES]


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- inputs and reference, built once ----------------------
_cache = {}


def in_range_part(f_rp, f_ci, cols):
    """F without its entries at or above cols"""
    rows = np.repeat(np.arange(f_rp.size - 1, dtype=np.int64), np.diff(np.asarray(f_rp, np.int64)))
    ok = (f_ci >= 0) & (f_ci < cols)
    return gen._csr_from_pairs(rows[ok], f_ci[ok], f_rp.size - 1, dedup=False, sort=False)


def _finish(s):
    """the oracle's product, the reference under the mask, and the masked oracle's say on the mask's in-range part"""
    cols = s["ncols"]
    s["want"] = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
    s["ref"] = gen.masked_reference(s["want"], s["f_rp"], s["f_ci"])
    i_rp, i_ci = in_range_part(s["f_rp"], s["f_ci"], cols)
    orc = O.spgemm_masked(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols, i_rp, i_ci)
    assert _diff(orc, s["ref"]) is None, "the masked oracle disagrees with the reference: %s" % _diff(orc, s["ref"])
    assert _diff(gen.masked_reference(s["want"], i_rp, i_ci), s["ref"]) is None
    s["mask_len"] = np.diff(s["f_rp"]).astype(np.int64)
    s["bins"] = np.bincount(gen.masked_row_bins(s["products"], s["mask_len"], cols), minlength=gen.NUM_BINS).tolist()
    return s


def _case(key):
    if key not in _cache:
        kind, cols = key[:2]
        build = gen.masked_one_wave_case if kind == "wave" else gen.masked_window_case
        _cache[key] = _finish(build(cols, *key[2:]))
    return _cache[key]


def _diff(got, exp):
    for what, g, e in zip(("row_ptr", "col_idx"), got, exp):
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape:
            return "%s: %d entries, expected %d" % (what, g.size, e.size)
        if not np.array_equal(g, e):
            return "%s differs (first at %s)" % (what, np.flatnonzero(g != e)[:5])
    return None


def _keys(rp, ci):
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    return (rows << 32) | np.asarray(ci, np.int64)


def _defaults(ctx):
    ctx.set_flow("auto")
    for k, v in (("small_path", -1), ("padded_rows", -1), ("blocked_extents", -1), ("check", 0), ("class_streams", 2)):
        ctx.set_option(k, v)


def _upload(ctx, s):
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], s["ncols"])
    return A, B


def _run(ctx, A, B, Fm, r0=0, r1=None, how="masked"):
    if how == "count":
        Cr = ctx.multiply_masked_count(A, B, Fm, r0, r1)
    else:
        Cr = ctx.multiply_masked(A, B, Fm, r0, r1, complement=how == "complement")
    st = ctx.stats()
    got = Cr.download()
    Cr.free()
    return got, st


def _check_path(s, st, got, bins=None):
    """upper-bound flow, no small path, the host model's classes (gen.masked_row_bins) and the product count"""
    exp = dict(flow=1, small_path=0, rows_per_bin=s["bins"] if bins is None else bins,
               bin_cap=gen.expected_bin_caps(s["ncols"], rank_cap=0), products=int(s["products"].sum()), nnz_c=int(got[1].size))
    path = {k: st[k] for k in exp}
    assert path == exp, "path %s, expected %s" % (path, exp)


# ---------------------------------------------------------------- (a) every one-wave Keep instance -----------------------
@pytest.mark.parametrize("cols", gen.MASK_ONE_WAVE_COLS)
def test_one_wave_mask_columns_beyond_the_top_bitmap(ctx, cols):
    """one-wave rows at one, two and three bitmap levels (both sides of each boundary), mask rows at the bottom and the top
    of each of the seven capacities, the masks full of columns at and above B.cols (gen._beyond_columns), F.cols = 2^31 - 1"""
    s = _case(("wave", cols))
    _defaults(ctx)
    A, B = _upload(ctx, s)
    Fm = ctx.upload(s["f_rp"], s["f_ci"], INT_MAX)
    try:
        got, st = _run(ctx, A, B, Fm)
    finally:
        for h in (A, B, Fm):
            h.free()
    print("cols %d: nnz(C) %d of %d mask entries, rows_per_bin %s" % (cols, got[1].size, s["f_ci"].size, st["rows_per_bin"]))
    bad = _diff(got, s["ref"])
    assert bad is None, bad
    _check_path(s, st, got)
    assert all(st["rows_per_bin"][1:17]) and not any(st["rows_per_bin"][17:]), st["rows_per_bin"]


@pytest.mark.parametrize("cols", gen.MASK_ONE_WAVE_COLS)
def test_one_wave_row_ranges(ctx, cols):
    """the same on the whole of A, an interior range that starts off a multiple of 16 rows, and one row; F is indexed by
    absolute row"""
    s = _case(("wave", cols))
    R = s["a_rp"].size - 1
    one = int(np.flatnonzero((s["kinds"] == "mixed") & (np.diff(s["ref"][0]) > 0) & (s["mask_len"] > 64))[3])
    ranges = ((0, R), (R // 7 + 5, R - R // 5), (one, one + 1))
    assert ranges[1][0] % 16 != 0
    _defaults(ctx)
    A, B = _upload(ctx, s)
    Fm = ctx.upload(s["f_rp"], s["f_ci"], INT_MAX)
    failures = []
    try:
        for r0, r1 in ranges:
            got, st = _run(ctx, A, B, Fm, r0, r1)
            exp = gen.masked_reference(s["want"], s["f_rp"], s["f_ci"], r0, r1)
            bad = _diff(got, exp)
            if bad:
                failures.append("rows [%d, %d): %s" % (r0, r1, bad))
            bins = np.bincount(gen.masked_row_bins(s["products"][r0:r1], s["mask_len"][r0:r1], cols), minlength=gen.NUM_BINS)
            if st["rows_per_bin"] != bins.tolist() or st["flow"] != 1 or st["small_path"] != 0:
                failures.append("rows [%d, %d): classes %s, expected %s" % (r0, r1, st["rows_per_bin"], bins.tolist()))
        assert exp[1].size > 0                              # (the single row keeps something)
    finally:
        for h in (A, B, Fm):
            h.free()
    assert not failures, "\n  ".join(failures)


# ---------------------------------------------------------------- (c) the window kernel's Keep instance -------------------
@pytest.mark.parametrize("cols", gen.MASK_WINDOW_COLS)
def test_window_mask_columns_beyond_b_cols(ctx, cols):
    """mask rows longer than 2048, short masks on rows of more than 8192 products, and B.cols = 2^23 + 1 where every row
    takes the window kernel; B.cols is no multiple of the window, the masks hold columns of [B.cols, next window edge), the
    edge itself, aliases p + k * window and columns far beyond"""
    s = _case(("window", cols))
    assert cols % gen.mask_window(cols) != 0
    _defaults(ctx)
    A, B = _upload(ctx, s)
    Fm = ctx.upload(s["f_rp"], s["f_ci"], INT_MAX)
    try:
        got, st = _run(ctx, A, B, Fm)
    finally:
        for h in (A, B, Fm):
            h.free()
    print("cols %d: nnz(C) %d of %d mask entries, rows_per_bin %s" % (cols, got[1].size, s["f_ci"].size, st["rows_per_bin"]))
    bad = _diff(got, s["ref"])
    assert bad is None, bad
    _check_path(s, st, got)
    assert sum(st["rows_per_bin"][17:]) > 0, st["rows_per_bin"]


# ---------------------------------------------------------------- (d) identities on the same arguments --------------------
@pytest.mark.parametrize("key", CASES, ids=_ids)
def test_identities(ctx, key):
    """the counting product has the masked product's pattern and classes; the masked and the complemented product are
    disjoint and make up the oracle's product; the mask's part at or above B.cols alone gives an all-zero row_ptr"""
    s = _case(key)
    cols, R = s["ncols"], s["a_rp"].size - 1
    _defaults(ctx)
    A, B = _upload(ctx, s)
    Fm = ctx.upload(s["f_rp"], s["f_ci"], INT_MAX)
    rows = np.repeat(np.arange(R, dtype=np.int64), s["mask_len"])
    far = s["f_ci"] >= cols
    o_rp, o_ci = gen._csr_from_pairs(rows[far], s["f_ci"][far], R, dedup=False, sort=False)
    Fo = ctx.upload(o_rp, o_ci, INT_MAX)
    try:
        kept, st_m = _run(ctx, A, B, Fm)
        cnt, st_c = _run(ctx, A, B, Fm, how="count")
        comp, _ = _run(ctx, A, B, Fm, how="complement")
        none, st_o = _run(ctx, A, B, Fo)
    finally:
        for h in (A, B, Fm, Fo):
            h.free()
    assert _diff(kept, s["ref"]) is None, _diff(kept, s["ref"])
    assert _diff(cnt, kept) is None, "counting product's pattern: %s" % _diff(cnt, kept)
    assert st_c["rows_per_bin"] == st_m["rows_per_bin"] == s["bins"] and st_c["bin_cap"] == st_m["bin_cap"]
    kk, kc = _keys(*kept), _keys(*comp)
    assert np.intersect1d(kk, kc).size == 0, "masked and complemented product share entries"
    assert np.array_equal(np.union1d(kk, kc), _keys(*s["want"])), "masked and complemented product do not make up the product"
    assert o_ci.size > R and not none[0].any() and none[1].size == 0, "a mask of columns >= B.cols kept %d entries" % none[1].size
    obins = np.bincount(gen.masked_row_bins(s["products"], np.diff(o_rp), cols), minlength=gen.NUM_BINS).tolist()
    assert st_o["rows_per_bin"] == obins, (st_o["rows_per_bin"], obins)


# ---------------------------------------------------------------- (e) where the mask comes from ---------------------------
FW = 300_000                    # the derived masks' column count: above B.cols = 1000, past the top bitmap (8192) and its aliases
SOURCES = ("wrap_device", "matrix_from_result", "transpose", "select", "setop")


@pytest.mark.parametrize("source", SOURCES)
def test_mask_provenance(ctx, source):
    """a mask of F.cols = 300 000 > B.cols = 1000 that is wrapped (arrays offset by one int: not 16-byte aligned), made from
    a result, transposed, selected or combined on the device gives what the same mask gives uploaded"""
    import torch
    s = _case(("wave", 1000, FW - 1))
    cols, R = s["ncols"], s["a_rp"].size - 1
    f_rp, f_ci = s["f_rp"], s["f_ci"]
    rows = np.repeat(np.arange(R, dtype=np.int64), s["mask_len"])
    assert int(f_ci.max()) == FW - 1 and np.any(f_ci >= 8192) and np.any(f_ci == cols)
    _defaults(ctx)
    A, B = _upload(ctx, s)
    made = []
    try:
        if source == "select":                             # F with the diagonal (i, i) added to every row, taken off again
            d_rp, d_ci = gen._csr_from_pairs(np.concatenate([rows, np.arange(R)]), np.concatenate([f_ci, np.arange(R)]), R,
                                             dedup=False, sort=False)
            drows = np.repeat(np.arange(R, dtype=np.int64), np.diff(d_rp))
            f_rp, f_ci = gen._csr_from_pairs(drows[d_ci != drows], d_ci[d_ci != drows], R, dedup=False, sort=False)
            made.append(ctx.upload(d_rp, d_ci, FW))
            Fd = ctx.select(made[-1], "offdiag")
        elif source == "wrap_device":
            t_rp = torch.zeros(R + 2, dtype=torch.int32, device="cuda")
            t_ci = torch.zeros(f_ci.size + 1, dtype=torch.int32, device="cuda")
            t_rp[1:] = torch.from_numpy(f_rp)
            t_ci[1:] = torch.from_numpy(f_ci)
            torch.cuda.synchronize()
            assert t_rp[1:].data_ptr() % 16 == 4 and t_ci[1:].data_ptr() % 16 == 4
            Fd = ctx.wrap_device(R, FW, f_ci.size, t_rp[1:].data_ptr(), t_ci[1:].data_ptr(), keep=(t_rp, t_ci))
        elif source == "matrix_from_result":               # I * F: a result with F's pattern
            made.append(ctx.upload(np.arange(R + 1), np.arange(R), R))
            made.append(ctx.upload(f_rp, f_ci, FW))
            P = ctx.multiply(made[0], made[1])
            try:
                Fd = ctx.matrix_from_result(P, FW)
            finally:
                P.free()
        elif source == "transpose":                        # F^T, FW x R, flipped back on the device
            t_rp, t_ci = gen._csr_from_pairs(f_ci, rows, FW)
            made.append(ctx.upload(t_rp, t_ci, R))
            Fd = ctx.transpose(made[-1])
        else:                                              # F's entries dealt out to two operands, joined again
            parts = [gen._csr_from_pairs(rows[k::2], f_ci[k::2], R, dedup=False, sort=False) for k in (0, 1)]
            made += [ctx.upload(rp, ci, FW) for rp, ci in parts]
            Fd = ctx.setop(made[0], made[1], "or")
        made.append(Fd)
        assert Fd.cols == FW > cols and Fd.rows == R
        Fu = ctx.upload(f_rp, f_ci, FW)
        made.append(Fu)
        base, st = _run(ctx, A, B, Fu)
        got, _ = _run(ctx, A, B, Fd)
    finally:
        for h in [A, B] + made:
            h.free()
    exp = gen.masked_reference(s["want"], f_rp, f_ci)
    assert exp[1].size > 0 and _diff(base, exp) is None, _diff(base, exp)
    assert _diff(got, base) is None, "%s: %s" % (source, _diff(got, base))
    assert st["flow"] == 1 and st["small_path"] == 0 and not any(st["rows_per_bin"][17:])


# ---------------------------------------------------------------- (f) the drop-in ------------------------------------------
@pytest.mark.parametrize("key", [("wave", 1000), ("window", 300_001)], ids=["one_wave", "window"])
def test_dropin_mask_columns_at_and_above_bm(key):
    """SpGEMM_hip_masked with an Fcol that holds Bm itself and columns far above it (past the top bitmap, up to 2^31 - 1),
    then a valid call within Bm"""
    s = _case(key)
    cols, R = s["ncols"], s["a_rp"].size - 1
    crow, ccol = bspgemm.SpGEMM_hip_masked(s["a_ci"], s["a_rp"], R, s["b_ci"], s["b_rp"], cols, s["f_ci"], s["f_rp"])
    assert int(s["f_ci"].max()) == INT_MAX and np.any(s["f_ci"] == cols)
    assert _diff((crow, ccol), s["ref"]) is None, _diff((crow, ccol), s["ref"])
    i_rp, i_ci = in_range_part(s["f_rp"], s["f_ci"], cols)
    crow, ccol = bspgemm.SpGEMM_hip_masked(s["a_ci"], s["a_rp"], R, s["b_ci"], s["b_rp"], cols, i_ci, i_rp)
    orc = O.spgemm_masked(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols, i_rp, i_ci)
    assert orc[1].size > 0 and _diff((crow, ccol), orc) is None, _diff((crow, ccol), orc)
