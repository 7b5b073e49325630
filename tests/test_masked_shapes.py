"""The inputs of tests/test_gpu_masked.py, checked without a GPU: the host model of the masked product's classes
(gen.masked_row_bins) shows that they reach every Keep instance of the one-wave kernel (three depths x seven mask-row
capacities, each at its shortest and its longest mask row) and the three kinds of rows of the Keep window kernel, that the
masks hold the columns at and above B.cols they are meant to hold, and that a kernel which wrapped such a column into the
top bitmap or the window would give another result than the reference -- so the GPU test can fail.
"""
import numpy as np

import gen
from oracle import oracle as O

INT_MAX = gen.INT_MAX


def _rows(s):
    return np.repeat(np.arange(s["f_rp"].size - 1, dtype=np.int64), np.diff(s["f_rp"]))


def _in_range_per_row(s):
    return np.bincount(_rows(s)[s["f_ci"] < s["ncols"]], minlength=s["f_rp"].size - 1)


def _wrapped(s, span):
    """the mask as a kernel would see it that wrapped every column at or above B.cols by `span`"""
    f = s["f_ci"].astype(np.int64)
    return s["f_rp"], np.where(f >= s["ncols"], f % span, f)


def _common(s):
    """what every input has: unsorted rows with repeats, and the columns at and above B.cols"""
    cols, f = s["ncols"], s["f_ci"].astype(np.int64)
    m = np.diff(s["f_rp"])
    keys = (_rows(s) << 32) | f
    assert np.unique(keys).size < keys.size, "no repeats"
    inner = np.ones(f.size, bool)
    inner[s["f_rp"][:-1][m > 0]] = False
    assert np.any(np.diff(f)[inner[1:]] < 0), "sorted rows"
    W = gen.mask_window(cols)
    edge = -(-cols // W) * W
    for what, ok in (("B.cols", f == cols), ("2^31 - 1", f == INT_MAX), ("p + 2^30", (f >= 1 << 30) & (f < (1 << 30) + cols)),
                     ("the window edge", f == edge), ("[B.cols, edge)", (f >= cols) & (f < edge) if edge > cols else None)):
        assert ok is None or ok.any(), "%d columns: no mask column %s" % (cols, what)
    for S in gen.mask_alias_spans(cols):
        assert S < cols or (np.any(f == S) and (S == cols or np.any((f > cols) & (f < S)))), (cols, S)
    return m


def test_shapes_cover_every_keep_kernel():
    populated = set()
    for cols in gen.MASK_ONE_WAVE_COLS:
        s = gen.masked_one_wave_case(cols)
        m = _common(s)
        L = gen.mask_levels(cols)
        span = 256 << (5 * L)
        assert L and (cols <= span) and gen.mask_alias_spans(cols)[0] == span
        F = s["products"]
        assert F.max() <= gen.MASK_WAVE_MAX_PRODUCTS and m.max() <= 2048
        bins = gen.masked_row_bins(F, m, cols)
        assert bins.max() <= 16 and np.any((bins == 0) & (m > 0)), "a row above the one-wave classes / none without products"
        assert np.array_equal(bins > 0, F > 0)
        nin = _in_range_per_row(s)
        want = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
        ref = gen.masked_reference(want, s["f_rp"], s["f_ci"])
        nout = np.diff(ref[0])
        for k, cap in enumerate(gen.MASK_CAPS):
            lo = gen.MASK_CAPS[k - 1] + 1 if k else 1
            sel = (bins > 0) & (m >= lo) & (m <= cap)
            assert sel.sum() >= 16 * 4 + 1, (cols, cap, int(sel.sum()))     # a full workgroup of 4 waves x 16 rows and a tail
            assert np.all(np.array(gen.WAVE_CAPS)[bins[sel] - 1] <= cap) and gen.mask_cap_of_len(lo) == cap
            for length in (lo, cap):
                at = sel & (m == length)
                assert np.any(at & (nin == 0)), "%d columns, mask rows of %d: none of columns >= B.cols only" % (cols, length)
                assert np.any(at & (nout > 0)), (cols, length)
            assert np.any(sel & (m == cap) & (nin == 1) & (nout == 1)), "%d columns: no full row of %d with one entry in range" % (cols, cap)
            populated.add((L, cap))
        assert np.all(nout[nin == 0] == 0) and np.any(nout > 10)
        # the aliases: a kernel that wrapped the top index would keep product columns that the mask does not hold
        alias = gen.masked_reference(want, *_wrapped(s, span))
        assert alias[1].size > ref[1].size + 100, (cols, alias[1].size, ref[1].size)
    assert populated == {(L, cap) for L in (1, 2, 3) for cap in gen.MASK_CAPS}, sorted(populated)

    kinds = set()
    for cols in gen.MASK_WINDOW_COLS:
        s = gen.masked_window_case(cols)
        m = _common(s)
        F = s["products"]
        W = gen.mask_window(cols)
        assert cols % W != 0 and cols % 64 != 0
        bins = gen.masked_row_bins(F, m, cols)
        here = set()
        if np.any((F > 0) & (m > 2048) & (bins > 16)):
            here.add("long mask")
        if np.any((m > 0) & (m <= 2048) & (F > gen.MASK_WAVE_MAX_PRODUCTS) & (bins > 16)):
            here.add("many products")
        if gen.mask_levels(cols) == 0:
            assert cols == (1 << 23) + 1 and np.any((bins >= 1) & (bins <= 16))
            here.add("wide")
        assert {"long mask", "many products"} <= here, (cols, here)
        kinds |= here
        nin = _in_range_per_row(s)
        assert np.any((nin == 0) & (m > 2048) & (F > 0)), "no long mask row of columns >= B.cols only"
        want = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
        ref = gen.masked_reference(want, s["f_rp"], s["f_ci"])
        assert np.any(want[1] == cols - 1) and np.diff(ref[0]).max() > 2048
        heavy = bins > 16 if gen.mask_levels(cols) else bins > 0
        alias = gen.masked_reference(want, *_wrapped(s, W))
        extra = np.diff(alias[0]) - np.diff(ref[0])
        assert np.all(extra >= 0) and np.count_nonzero(extra[heavy]) > 50, (cols, np.count_nonzero(extra[heavy]))
    assert kinds == {"long mask", "many products", "wide"}, kinds


def test_masked_row_bins_model():
    """gen.masked_row_bins: by the stored mask length, 0 without products, a heavy class above 8192 products"""
    F = np.array([0, 5, 5, 5, 5, 8192, 8193, 8193, 9000, 0])
    m = np.array([7, 0, 1, 64, 65, 2048, 1, 2048, 2049, 0])
    assert gen.masked_row_bins(F, m, 6000).tolist() == [0, 0, 1, 1, 2, 16, gen.MID_BIN, gen.MID_BIN, gen.MID_BIN, 0]
    # (the masked products have no rank class: 2049 .. 6144 entries are the mid class where the plain product ranks them)
    assert gen.row_bins([3000], 700_001).tolist() == [gen.RANK_BIN] and gen.masked_row_bins([3000], [3000], 700_001).tolist() == [gen.MID_BIN]
    assert gen.expected_bin_caps(700_001, rank_cap=0)[gen.RANK_BIN] == 2048 and gen.expected_bin_caps(700_001)[gen.RANK_BIN] == 6144
