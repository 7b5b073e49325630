"""The products of tests/test_gpu_small_path.py, checked without a GPU: every shape really holds the case it is named for
(tests/gen.py small_model derives what csrc/small.hip will do with it), and the reference those tests compare with
(gen.small_reference: np.unique per row) equals the CPU oracle wherever the oracle can go (up to 6e8 columns).
"""
import numpy as np
import pytest

import gen
from oracle import oracle as O

LADDER, FIT, TILE = gen.small_ladder_cases(), gen.small_fit_cases(), gen.small_tile_cases()
KEY_SIZES = (16, 17, 2047, 2048)


def _model(s, r0=0, r1=None):
    return gen.small_model(s["a_rp"], s["a_ci"], s["b_rp"], r0, r1)


def _nnz_rows(s, r0=0, r1=None):
    return np.diff(gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], r0, r1)[0])


def _check_reference(s, r0=0, r1=None):
    """small_reference == the oracle; sorted rows without repeats"""
    r1 = s["a_rp"].size - 1 if r1 is None else r1
    rp, ci = gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], r0, r1)
    assert rp.dtype == np.int64 and ci.dtype == np.int32 and rp.size == r1 - r0 + 1 and rp[-1] == ci.size
    inner = np.ones(ci.size, bool)
    inner[rp[:-1][rp[:-1] < ci.size]] = False
    assert np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0)
    if s["ncols"] <= 600_000_000:
        erp, eci = O.spgemm_rows(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], s["ncols"], r0, r1)
        assert np.array_equal(rp, erp) and np.array_equal(ci, eci)
    return rp, ci


def _operands_unsorted(s):
    """A and B hold rows out of order (unless no row of theirs has two different entries)"""
    for rp, ci in ((s["a_rp"], s["a_ci"]), (s["b_rp"], s["b_ci"])):
        inner = np.ones(ci.size, bool)
        inner[rp[:-1][rp[:-1] < ci.size]] = False
        d = np.diff(ci.astype(np.int64))[inner[1:]]
        assert np.any(d < 0) or not np.any(d != 0)


def _rows_with_split(s, m, split):
    """the rows whose A-entries are split as `split` says, from A and B themselves"""
    a_rp, a_ci, blen = s["a_rp"].astype(np.int64), s["a_ci"], np.diff(s["b_rp"].astype(np.int64))
    per = blen[a_ci]
    cs = np.concatenate([[0], np.cumsum(per == 0)])
    holes = cs[a_rp[1:]] - cs[a_rp[:-1]]
    if split == "one":                                   # ... on a single B row of F entries
        return (m["alen"] == 1) & (m["F"] > 0)
    if split == "ones":
        return (m["alen"] == m["F"]) & (holes == 0) & (m["F"] > 0)
    if split in ("s64", "s65"):
        return (m["alen"] == int(split[1:])) & (m["F"] > 0)
    if split == "holes":
        first = np.minimum(a_rp[:-1], max(per.size - 1, 0))
        return (holes > 0) & (m["F"] > 0) & (m["alen"] != 64) & (m["alen"] != 65) & (per[first] == 0)
    assert split == "repeat"
    return np.array([a_rp[i + 1] - a_rp[i] > 1 and np.unique(a_ci[a_rp[i]:a_rp[i + 1]]).size <= 2 for i in range(m["R"])])


@pytest.mark.parametrize("name", list(LADDER))
def test_ladder_shape(name):
    s = LADDER[name]()
    m = _model(s)
    F = m["F"]
    assert m["fits"] and int(s["a_rp"][-1]) <= gen.SMALL_MAX_NNZ_A and m["R"] <= gen.SMALL_MAX_ROWS
    assert F.sum() == s["reps"] * 10116 + 2 * 136 and sum(gen.SMALL_LADDER) == 10116
    for f in gen.SMALL_LADDER:                             # every size, `reps` times (1 .. 16 twice more)
        assert (F == f).sum() == s["reps"] + (2 if f <= 16 else 0), f
    assert np.all(m["lane"] == (F <= 16)) and np.all(m["wave"] == (F > 16))
    # the padding N on both sides of every power of two, and N == F at each
    for f, n in ((17, 64), (63, 64), (64, 64), (65, 128), (128, 128), (129, 256), (256, 256), (257, 512), (512, 512), (513, 1024),
                 (1024, 1024), (1025, 2048), (2047, 2048), (2048, 2048)):
        assert np.all(m["N"][F == f] == n), (f, n)
    # lane-rows and wave-rows share the 64-row batches of the list
    batches = [m["lane"][m["list"][k:k + 64]] for k in range(0, m["list"].size, 64)]
    assert sum(1 for b in batches if b.any() and not b.all()) >= 2
    _operands_unsorted(s)
    nnz = _nnz_rows(s)
    want = {"distinct": F, "edges": F, "same": np.ones_like(F), "pairs": np.maximum(1, F // 2), "to16": np.minimum(F, 16),
            "to17": np.minimum(F, 17)}[s["content"]]
    assert np.array_equal(nnz, want)
    if s["content"] == "to16":                             # sorted by the wave in k_small_rows, moved by a lane in k_small_copy
        assert np.all(nnz[m["wave"]] == 16) and m["wave"].sum() == 19 * s["reps"]
    if s["content"] == "to17":                             # ... and one entry more: moved by the wave
        assert np.all(nnz[m["wave"]] == 17)
    if s["content"] == "edges":
        ref = gen.small_reference(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"])
        big = np.flatnonzero(F >= 2)
        assert np.all(ref[1][ref[0][big]] == 0) and np.all(ref[1][ref[0][big + 1] - 1] == s["ncols"] - 1)
    if s["content"] == "distinct":                         # gathered in descending order
        i = int(np.flatnonzero(F == 2048)[0])
        blen = np.diff(s["b_rp"])
        got = np.concatenate([s["b_ci"][s["b_rp"][j]:s["b_rp"][j] + blen[j]] for j in s["a_ci"][s["a_rp"][i]:s["a_rp"][i + 1]]])
        assert got.size == 2048 and np.all(np.diff(got.astype(np.int64)) < 0)
    splits = [x for x in gen.SMALL_SPLITS[:-1] if x != "repeat" or s["content"] not in ("distinct", "edges")] if s["split"] == "mixed" else [s["split"]]
    for sp in splits:
        rows = _rows_with_split(s, m, sp)
        sizes = KEY_SIZES if s["split"] != "mixed" else ()
        for f in sizes:
            if sp == "repeat" and f <= gen._small_distinct(s["content"], f):
                continue                                   # (a row of distinct columns is one reference; same x repeat has it)
            assert np.any(rows & (F == f)), (sp, f)
        assert np.any(rows & m["wave"]) and (np.any(rows & m["lane"]) or (sp == "repeat" and s["content"] in ("to16", "to17"))), sp
    if "ones" in splits:                                   # 2048 one-entry sources: 32 trips of the gather loop
        assert np.any((m["steps"] == 32) & (F == 2048) & (m["alen"] == 2048))
    if "s65" in splits:
        assert np.any((m["steps"] == 2) & (m["alen"] == 65))
    if "s64" in splits:
        assert np.any((m["steps"] == 1) & (m["alen"] == 64) & m["wave"])
    if "one" in splits:                                    # a single B row of 2048 entries
        i = np.flatnonzero((F == 2048) & (m["alen"] == 1))
        assert i.size and np.diff(s["b_rp"])[s["a_ci"][s["a_rp"][i[0]]]] == 2048
    _check_reference(s)


def test_ladder_covers_contents_and_splits():
    """every content and every split is there at 6000 and at 6e8 columns; the sentinel case at 2^31 - 1"""
    plan = gen.SMALL_LADDER_PLAN
    for cols in (6000, 600_000_000):
        assert {p[0] for p in plan if p[2] == cols} == set(gen.SMALL_CONTENTS)
    assert {p[1] for p in plan} == set(gen.SMALL_SPLITS)
    assert [p for p in plan if p[2] > 600_000_000] == [("edges", "mixed", 2**31 - 1, 6)]
    s = LADDER["ladder_edges_mixed_%d" % (2**31 - 1)]()
    assert s["small_only"] and int(s["b_ci"].max()) == 2**31 - 2


def test_fit_limit_shapes():
    exp = lambda s, flow, small, m: gen.small_expected(flow, small, m["R"], int(s["a_rp"][-1]), int(s["b_rp"][-1]), s["b_rp"].size - 1, m["F"])
    for total in (65535, 65536, 65537):
        s = FIT["fit_total_%d" % total]()
        m = _model(s)
        assert m["R"] == 1 << 17 and m["F"].sum() == total and s["a_rp"][-1] == 32768 and m["list"].size == 32768
        assert m["fits"] == (total <= 65536) and exp(s, "upper-bound", 1, m) == (total <= 65536)
        assert m["F"][0] > 0 and m["F"][-1] > 0 and m["plan_trips"] == 16
        rp, ci = _check_reference(s)
        assert ci.size == total                            # all distinct: C.col_idx full to the last entry at 65536
    for big in (2048, 2049):
        s = FIT["fit_row_%d" % big]()
        m = _model(s)
        r = s["big_row"]
        assert m["F"][r] == big == m["F"].max() and r // 32 >= 256 and m["plan_trips"] == 2 and m["mx32"][r // 32] == big
        assert np.delete(m["F"], r).max() <= 3 and m["F"].sum() <= 65536 and m["fits"] == (big == 2048)
        assert exp(s, "upper-bound", 1, m) == (big == 2048) and s["a_rp"][-1] <= 32768
        _check_reference(s)
    s = FIT["fit_nnz_a_32769"]()
    m = _model(s)
    assert s["a_rp"][-1] == 32769 and m["fits"] and not exp(s, "upper-bound", 1, m) and m["R"] == 1 << 17
    _check_reference(s)
    s = FIT["fit_rows_131073"]()
    m = _model(s)
    assert m["R"] == (1 << 17) + 1 and m["fits"] and s["a_rp"][-1] <= 32768 and not exp(s, "upper-bound", 1, m)
    _check_reference(s)
    at, above = FIT["fit_auto_at_limit"](), FIT["fit_auto_above_limit"]()
    m = _model(at)
    assert at["a_rp"][-1] == 4096 and at["b_rp"][-1] == 512 and at["b_rp"].size == 65 and m["F"].sum() == 32768 and m["fits"]
    assert at["a_ci"].max() <= 62 and above["b_rp"][-1] == 513 and np.array_equal(at["a_ci"], above["a_ci"])
    assert exp(at, "auto", -1, m) and not exp(above, "auto", -1, _model(above)) and exp(above, "auto", 1, _model(above))
    assert not exp(at, "exact", 1, m)
    a, b = _check_reference(at), _check_reference(above)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("R", gen.SMALL_TILE_ROWS)
def test_tile_edge_shape(R):
    s = TILE["tile_rows_%d" % R]()
    m = _model(s)
    F = m["F"]
    assert m["R"] == R and m["fits"] and s["a_rp"][-1] <= 32768
    for r in (0, 31, 32, 255, 256, 257, 8191, 8192, R - 1):
        if r < R:
            assert F[r] > 0, r
    assert m["list"].size == s["nonempty"] and (R not in gen.SMALL_TILE_NONEMPTY or m["list"].size == gen.SMALL_TILE_NONEMPTY[R])
    if R > 3:
        assert m["list"].size > len(s["edge"])            # random ones too
    dead = (m["alen"] > 0) & (F == 0)                      # A-entries on empty B rows only: no product, not listed
    if R >= 31:
        assert dead.any() and np.all(np.diff(s["b_rp"])[s["a_ci"]][np.repeat(dead, m["alen"])] == 0)
        assert m["lane"].any() and m["wave"].any()
    assert not np.isin(np.flatnonzero(dead), m["list"]).any()
    # the scans: 32-row sums, 256-row sums and what lies before each workgroup
    assert m["f32"].size == -(-R // 32) and m["f32"].sum() == F.sum() and m["nz32"].sum() == m["list"].size
    assert m["f256"].size == -(-R // 256) and np.array_equal(m["before256"], [F[:256 * k].sum() for k in range(m["f256"].size)])
    if R > 256:
        assert m["before256"][1] > 0                       # k_small_plan's `k < 8 * blockIdx.x` adds something
    if R == 65537:
        assert m["plan_trips"] == 9 and (m["list"] // 32 >= 256).any() and m["nz32"][256:].sum() > 0
    if R in (8193, 65537):
        assert m["plan_trips"] >= 2 and F[8192] > 0
    _check_reference(s)


def test_row_range_shape():
    s = gen.small_range_case()
    _operands_unsorted(s)
    assert [r1 - r0 for r0, r1 in s["ranges"]] == [1, 33, 257]
    for r0, r1 in s["ranges"]:
        m = _model(s, r0, r1)
        assert r0 % 32 != 0 and m["fits"] and m["F"][0] > 0 and m["F"][-1] > 0
        if r1 - r0 > 1:
            assert m["lane"].any() and m["wave"].any() and ((m["alen"] > 0) & (m["F"] == 0)).any() and (m["alen"] == 0).any()
        _check_reference(s, r0, r1)
    assert _model(s, 5, 6)["F"][0] == 600


def test_model_on_a_hand_made_product():
    """small_model and small_reference on a product small enough to write down"""
    a_rp = np.array([0, 2, 2, 3, 5], np.int32)
    a_ci = np.array([1, 0, 2, 2, 1], np.int32)
    b_rp = np.array([0, 2, 3, 3], np.int32)
    b_ci = np.array([9, 4, 4], np.int32)
    m = gen.small_model(a_rp, a_ci, b_rp)
    assert m["F"].tolist() == [3, 0, 0, 1] and m["list"].tolist() == [0, 3] and m["lane"].tolist() == [True, False, False, True]
    assert m["f32"].tolist() == [4] and m["nz32"].tolist() == [2] and m["mx32"].tolist() == [3] and m["fits"]
    rp, ci = gen.small_reference(a_rp, a_ci, b_rp, b_ci)
    assert rp.tolist() == [0, 2, 2, 2, 3] and ci.tolist() == [4, 9, 4]
    rp, ci = gen.small_reference(a_rp, a_ci, b_rp, b_ci, 1, 4)
    assert rp.tolist() == [0, 0, 0, 1] and ci.tolist() == [4]
    t = np.array([17, 0, -1, 2048, 16])
    a = gen.small_rows_case(t, "to16", "s65", 6000, 1)
    m = gen.small_model(*a[:3])
    assert m["F"].tolist() == [17, 0, 0, 2048, 16] and m["N"].tolist() == [64, 0, 0, 2048, 0] and m["alen"].tolist() == [65, 0, 2, 65, 65]
    assert m["steps"].tolist() == [2, 0, 0, 2, 0] and not gen.small_fits(np.array([2049])) and not gen.small_fits(np.array([2048] * 33))
