"""The cases of tests/test_gpu_transpose_edges.py and tests/test_gpu_canonical_check.py, checked without a GPU: the
constants that tests/transpose_ref.py mirrors are the ones in the sources, every named transpose case really holds the
kernel edge it is named for (transpose_ref.plan derives what csrc/transpose.hip will do with it), every base operand of
the check cases is canonical, every defect changed exactly what it says, and every control is canonical although it
looks like a defect to a check that forgot the row boundary.
"""
import numpy as np
import pytest

import setop_ref
import transpose_ref as T


def _plan(name):
    c = T.transpose_case(name)
    return c, T.plan(c["rp"], c["ci"], c["cols"])


def _fills(p, kind=None):
    return [f for f in p["fills"] if kind is None or f["kind"] == kind]


# ---------------------------------------------------------------- the mirror, the reference, the model ---------------
def test_constants_are_the_sources():
    src = T.source_constants()
    assert src == {k: getattr(T, k) for k in src}
    assert (T.TR_TILE, T.TR_WAVE, T.TR_ITEMS, T.DIGIT_BITS, T.TR_STAGE_SPAN, T.FILL_WIDE) == (4096, 1024, 16, 8, 8192, 8)
    assert (T.SEL_TILE, T.SEL_WAVE, T.SEL_STEP, T.SEL_STAGE) == (4096, 1024, 256, 4096)


def test_reference_on_a_hand_made_operand():
    rp, ci = np.array([0, 3, 3, 6], np.int32), np.array([2, 0, 2, 1, 2, 1], np.int32)      # rows {0, 2}, {}, {1, 2}
    t_rp, t_ci = T.ref_transpose(rp, ci, 4)
    assert t_rp.tolist() == [0, 1, 2, 4, 4] and t_ci.tolist() == [0, 2, 0, 2]
    c_rp, c_ci = T.ref_canonical(rp, ci, 4)
    assert c_rp.tolist() == [0, 2, 2, 4] and c_ci.tolist() == [0, 2, 1, 2]
    assert not T.is_canonical(rp, ci) and T.is_canonical(c_rp, c_ci) and T.is_canonical(t_rp, t_ci)
    p = T.plan(rp, ci, 4)
    assert (p["bits"], p["passes"], p["nbits"]) == (2, 1, [2]) and p["tiles"] == [(0, 2, 3, True)]
    assert p["keys"].tolist() == [0, 1, 1, 2, 2, 2] and p["vals"].tolist() == [0, 2, 2, 0, 0, 2]
    assert p["runs"] == [(1, 2), (3, 4)] and p["last_thread"] == "scalar"
    assert [(f["pos"], f["empty"], f["kind"]) for f in p["fills"]] == [(0, 0, "leading"), (1, 0, "inner"), (3, 0, "inner"),
                                                                      (6, 1, "trailing")]


@pytest.mark.parametrize("name", list(T.TRANSPOSE_CASES))
def test_reference_agrees_with_the_set_model(name):
    """two independent references: the lexsort of transpose_ref and the key sets of setop_ref"""
    c = T.transpose_case(name)
    (t_rp, t_ci), (c_rp, c_ci) = T.transpose_expected(name)
    s_rp, s_ci = setop_ref.transpose_ref(c["rp"], c["ci"], c["rows"], c["cols"])
    assert np.array_equal(t_rp, s_rp) and np.array_equal(t_ci, s_ci)
    s_rp, s_ci = setop_ref.canonical_ref(c["rp"], c["ci"], c["rows"], c["cols"])
    assert np.array_equal(c_rp, s_rp) and np.array_equal(c_ci, s_ci)
    assert c["ci"].size <= 20000 and c["ci"].min() >= 0 and c["ci"].max() < c["cols"]


# ---------------------------------------------------------------- the transpose cases --------------------------------
@pytest.mark.parametrize("E", T.ENTRY_COUNTS)
def test_entry_counts(E):
    c, p = _plan("entries%d" % E)
    assert p["E"] == E and p["passes"] == 1 and c["cols"] == 200
    assert len(p["tiles"]) == (E + 4095) // 4096
    assert p["last_thread"] == ("vector" if E in (16, 4096, 8192) else "scalar")
    if E > 100:
        assert not T.is_canonical(c["rp"], c["ci"]) and p["runs"]


@pytest.mark.parametrize("span", T.WINDOW_SPANS)
@pytest.mark.parametrize("kind", T.WINDOW_KINDS)
def test_row_window(kind, span):
    c, p = _plan("window_%s%d" % (kind, span))
    lens = np.diff(c["rp"])
    if kind == "second":
        assert c["ci"].size == 4096 + 300
        assert p["tiles"] == [(0, 15, 16, True), (15, 15 + span - 1, span, span < 8192)]
        assert c["rp"][15] < 4096 < c["rp"][16]                          # the seam lies inside row 15
    else:
        assert c["ci"].size == 300
        head = 0 if kind == "edge" else 400
        assert p["tiles"] == [(head, head + span - 1, span, span < 8192)]
        assert c["rows"] == (span if kind == "edge" else 9000)
    if kind != "inner":
        assert lens[0] > 0 and lens[-1] > 0                              # entries in row 0 and in the last row
    else:
        assert lens[0] == 0 and lens[-1] == 0
    assert [t[3] for t in p["tiles"]][-1] == (span == 8191)
    assert 50 < np.count_nonzero(lens[p["tiles"][-1][0] + 1:p["tiles"][-1][1]]) < 200
    assert not T.is_canonical(c["rp"], c["ci"]) and p["runs"]


@pytest.mark.parametrize("cols", [1, 2])
def test_few_columns(cols):
    c, p = _plan("cols%d" % cols)
    assert (p["bits"], p["passes"], p["nbits"]) == (cols - 1, 1, [cols - 1])
    for r in range(c["rows"]):                                           # every row holds a repeat
        row = c["ci"][c["rp"][r]:c["rp"][r + 1]]
        assert row.size > np.unique(row).size
    assert len(p["tiles"]) >= 2


@pytest.mark.parametrize("which", T.THREE_PASS)
def test_three_passes(which):
    c, p = _plan("three_passes_%s" % which)
    assert c["cols"] == 65537 and (p["bits"], p["passes"], p["nbits"]) == (17, 3, [8, 8, 1])
    keys = np.unique(p["keys"])
    digits = [np.unique((keys >> s) & 255).size for s in (0, 8, 16)]
    expect = {"low": (7, 1, 1), "middle": (1, 7, 1), "top": (1, 1, 2)}
    if which in expect:
        assert tuple(digits) == expect[which]
    else:
        assert min(digits[:2]) >= 7 and digits[2] == 2
    rows_per_key = [np.unique(p["vals"][p["keys"] == k]).size for k in keys]
    assert min(rows_per_key) > 100 and p["runs"]                        # every key in many rows, with repeats


@pytest.mark.parametrize("pos", T.DUP_PAIR_AT)
def test_dup_pair(pos):
    c, p = _plan("dup_pair%d" % pos)
    assert p["E"] == 5000 and p["runs"] == [(pos - 1, pos)]
    assert p["thread_runs"] == [(pos - 1, pos)]
    assert p["wave_runs"] == ([(pos - 1, pos)] if pos % 1024 == 0 else [])
    assert p["tile_runs"] == ([(pos - 1, pos)] if pos % 4096 == 0 else [])
    assert not T.is_canonical(c["rp"], c["ci"])                          # the rows were shuffled


def test_dup_run40():
    _, p = _plan("dup_run40")
    assert p["E"] == 5000 and p["runs"] == [(2053, 2092)]
    assert p["threads_keep_nothing"] == [2064 // 16] and p["tiles_keep_nothing"] == []


def test_dup_row9000():
    c, p = _plan("dup_row9000")
    assert np.count_nonzero((p["keys"] == 7) & (p["vals"] == 1)) == 9000
    assert p["tiles_keep_nothing"] == [1, 2] and len(p["tiles"]) == 3
    assert len(p["threads_keep_nothing"]) > 500 and len(p["tile_runs"]) == 1
    (t_rp, t_ci), _ = T.transpose_expected("dup_row9000")
    assert t_ci[t_rp[7]:t_rp[8]].tolist() == [0, 1]                      # column 7 counts row 1 once
    assert p["fills"][-1]["wide"] and (p["E"] - 1) // 16 in p["threads_keep_nothing"]


@pytest.mark.parametrize("lead,trail", T.GAP_ENDS)
def test_gaps(lead, trail):
    c, p = _plan("gaps_lead%d_trail%d" % (lead, trail))
    assert p["E"] == 5200 and not p["runs"]
    inner = _fills(p, "inner")
    assert sorted(set(f["empty"] for f in inner)) == sorted(T.GAPS)
    assert all(f["wide"] == (f["empty"] >= 8) for f in p["fills"])
    assert [f["empty"] for f in _fills(p, "leading")] == [lead] and [f["empty"] for f in _fills(p, "trailing")] == [trail]
    # three wide fills of three lanes in one fill_rows call of the first wave, a narrow one beside them
    first_wave = [f for f in inner if f["pos"] < 1024 and f["wide"]]
    assert p["wide_per_wave"][0] >= 4 + (lead >= 8) and p["wide_same_call"] >= 3
    assert len({f["pos"] // 16 for f in first_wave if f["pos"] % 16 == 5}) == 3
    seam = [f for f in inner if f["seam"]]
    assert [(f["pos"], f["empty"], f["wide"]) for f in seam] == [(4096, 200, True)]


def test_gap_ends_cover_the_issue():
    assert {a for a, _ in T.GAP_ENDS} == {0, 8, 9, 100} and {b for _, b in T.GAP_ENDS} == {0, 1, 8, 9, 1000}


def test_hub_column():
    c, p = _plan("hub_column")
    assert c["rows"] == 9000 and np.all(np.diff(c["rp"]) == 2)
    hub = np.flatnonzero(p["keys"] == 7)
    assert hub.size >= 9000 and len({int(q) // 4096 for q in hub}) == 3  # the key's pairs run through three tiles
    (t_rp, _), _ = T.transpose_expected("hub_column")
    assert t_rp[8] - t_rp[7] == 9000


# ---------------------------------------------------------------- the check cases ------------------------------------
@pytest.mark.parametrize("E", T.CHECK_E)
def test_check_base_and_defects(E):
    x = T.check_base(E)
    rp, ci = x["rp"], x["ci"]
    assert ci.size == E and x["rows"] == x["cols"] and T.is_canonical(rp, ci)
    assert [t[3] for t in T.check_plan(rp, E)] == [True, True]
    assert int(np.diff(rp).max()) < x["rows"]                            # shorter than the full row it is paired with
    classes = {}
    for p in T.check_positions(E):
        for kind in ("repeat", "descent"):
            d = T.with_defect(rp, ci, p, kind)
            changed = np.flatnonzero(d != ci).tolist()
            assert changed == ([p] if kind == "repeat" else [p - 1, p])
            assert d[p] == ci[p - 1] and (kind == "repeat" or d[p - 1] == ci[p])
            # exactly one pair of neighbours in one row is out of order, the one in front of p
            r = int(np.searchsorted(rp, p, side="right")) - 1
            bad = [q for q in range(rp[r] + 1, rp[r + 1]) if d[q] <= d[q - 1]]
            assert bad == [p] and not T.is_canonical(rp, d)
            assert d.min() >= 0 and d.max() < x["cols"]
        classes[p] = T.position_class(p, E)
    assert {c["k"] for c in classes.values()} == {0, 1, 2, 3}
    for seam, at in (("step", 256), ("wave", 1024), ("tile", 4096)):
        assert classes[at][seam] and not classes[at - 1][seam] and not classes[at + 1][seam]
    assert classes[E - 1]["scalar"] == (E % 4 != 0) and classes[E - 1]["k"] == (E - 1) % 4
    with pytest.raises(AssertionError):
        T.with_defect(rp, ci, int(rp[3]), "repeat")                      # the first entry of a row is no place for one


@pytest.mark.parametrize("E", T.CHECK_E)
def test_check_control(E):
    x = T.check_control(E)
    rp, ci = x["rp"], x["ci"]
    assert ci.size == E and x["rows"] == x["cols"] and T.is_canonical(rp, ci)
    assert ci.min() >= 0 and ci.max() < x["cols"]
    starts = set(rp[:-1].tolist())
    equal = below = 0
    for p in T.check_positions(E):
        assert p in starts and ci[p] <= ci[p - 1]
        equal += ci[p] == ci[p - 1]
        below += ci[p] < ci[p - 1]
    assert equal >= 5 and below >= 5


@pytest.mark.parametrize("control", [False, True])
def test_check_unstaged(control):
    x, p = T.check_unstaged(control)
    rp, ci = x["rp"], x["ci"]
    assert T.is_canonical(rp, ci) and ci.size == 500
    (rb, rl, span, staged), = T.check_plan(rp, ci.size)
    assert (rb, rl) == (0, x["rows"] - 1) and span > 4096 and not staged and (x["rows"], x["cols"]) == (4250, 64)
    lens = np.diff(rp)
    assert np.all(lens[30:4230] == 0) and rp[30] == 300 and p >= 300     # p lies behind the run of empty rows
    if control:
        assert p == rp[4230] and ci[p] == ci[p - 1]
    else:
        assert T.position_class(p, ci.size)["k"] == 0 and rp[4230] < p < rp[4231]


@pytest.mark.parametrize("role", [0, 1, 2])
def test_dot_operands_make_every_entry_count(role):
    """a defect that the check missed would change the product: see the docstring of dot_operands"""
    import dot_ref
    x = T.check_base(4200)
    n = x["rows"]
    args = T.dot_operands((x["rp"], x["ci"]), x["cols"], role)
    a, b, f = args[:3]
    for m, rows in ((a, args[3]), (b, args[4]), (f, args[3])):
        assert len(m[0]) == rows + 1 and m[0][-1] == len(m[1]) and T.is_canonical(*m)
    rp, ci, val = dot_ref.dot_ref(*args)
    lens = np.diff(x["rp"])
    if role == 0:
        assert np.array_equal(val, lens) and np.array_equal(np.diff(rp), np.ones(n))
        assert np.all(lens < np.diff(b[0])[0])                           # the row of x is the shorter one
    elif role == 1:
        assert np.array_equal(val, lens) and ci.tolist() == list(range(n))
        assert np.all(lens < np.diff(a[0])[0])
    else:
        assert np.array_equal(rp, x["rp"]) and np.array_equal(ci, x["ci"]) and np.all(val == 1)


@pytest.mark.parametrize("E", T.CHECK_E)
def test_check_partner(E):
    x, y = T.check_base(E), T.check_partner(E)
    assert (y["rows"], y["cols"]) == (x["rows"], x["cols"]) and T.is_canonical(y["rp"], y["ci"])
    both = setop_ref.setop_ref(x["rp"], x["ci"], y["rp"], y["ci"], x["rows"], x["cols"], "and")[1].size
    assert E // 4 < both < 3 * E // 4 and y["ci"].size - both > E // 4   # every set operation has work on either side
