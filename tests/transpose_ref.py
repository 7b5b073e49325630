"""The host side of the kernel-edge tests of the operand transpose (csrc/transpose.hip) and of the canonical-form check
(k_set_flags of csrc/setop.hip): the reference transpose, a model of what the kernels will do with an input (`plan`,
`check_plan`), the named cases of tests/test_gpu_transpose_edges.py and tests/test_gpu_canonical_check.py, and the
defects the check has to find.  numpy only; nothing here touches the GPU.  tests/test_transpose_shapes.py proves with
the models that every case holds the property it is named for.

CSR everywhere as (row_ptr int32, col_idx int32); a case is a dict {rp, ci, rows, cols}, built once and read-only.
"""
import functools
import os
import re

import numpy as np

# ---- the constants of csrc/transpose.hip that the cases are built around -------------------------------------------
TR_THREADS = 256         # kTrThreads: four waves
TR_ITEMS = 16            # kTrItems: consecutive sorted pairs per thread of the dedup kernels
TR_TILE = 4096           # kTrTile = kTrThreads * kTrItems: entries per workgroup
TR_WAVE = 1024           # kTrWaveSpan: consecutive entries of one wave
DIGIT_BITS = 8           # kDigitBits
TR_STAGE_SPAN = 8192     # k_tr_scatter<true> stages the tile's row_ptr window iff the tile's rows span fewer than this
FILL_WIDE = 8            # fill_rows is wide iff hi - lo >= 8, that is, iff 8 or more empty rows precede the key's row
# ---- ... and of the check: csrc/sel_rows.hpp, csrc/kernels.hpp ------------------------------------------------------
SEL_TILE = 4096          # kSelTile (= kRowWorkTile)
SEL_STEP = 256           # kSelGroup: entries of one wave step, four per lane
SEL_STEPS = 4            # kSelSteps
SEL_WAVE = 1024          # kSelWaveSpan
SEL_STAGE = 4096         # kSelStage: the window is staged iff the tile spans at most this many rows

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "binary-spgemm_amd", "csrc")


def source_constants():
    """the same constants read from the sources, under the names above (the CPU tests compare the two)"""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def const(src, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))

    tr, sel, ker = text("transpose.hip"), text("sel_rows.hpp"), text("kernels.hpp")
    out = {"TR_THREADS": const(tr, "kTrThreads"), "TR_ITEMS": const(tr, "kTrItems"), "DIGIT_BITS": const(tr, "kDigitBits"),
           "SEL_STEP": const(sel, "kSelGroup"), "SEL_STEPS": const(sel, "kSelSteps"), "SEL_STAGE": const(sel, "kSelStage"),
           "SEL_TILE": const(ker, "kRowWorkTile")}
    out["TR_TILE"] = out["TR_THREADS"] * out["TR_ITEMS"]
    out["TR_WAVE"] = out["TR_TILE"] // 4
    out["SEL_WAVE"] = out["SEL_STEP"] * out["SEL_STEPS"]
    assert "constexpr int kTrTile = kTrThreads * kTrItems;" in tr and "constexpr int kTrWaveSpan = kTrTile / 4;" in tr
    assert "constexpr int kSelTile = kRowWorkTile;" in ker and "kSelWaveSpan = kSelSteps * kSelGroup;" in sel
    assert "staged = span < 2 * kTrTile;" in tr
    out["TR_STAGE_SPAN"] = 2 * out["TR_TILE"]
    out["FILL_WIDE"] = int(re.search(r"const bool wide = hi - lo >= (\d+);", tr).group(1))
    assert "t.staged = t.span <= kSelStage;" in sel and "if (vec && e + 3 < E)" in sel
    return out


# ---- the reference --------------------------------------------------------------------------------------------------
def ref_transpose(rp, ci, cols):
    """(row_ptr int32[cols+1], col_idx int32) of pattern(A)^T: the unique (k, i) pairs in lexicographic order"""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)[rp[0]:rp[-1]]
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    o = np.lexsort((rows, ci))
    k, i = ci[o], rows[o]
    keep = np.ones(k.size, bool)
    keep[1:] = (k[1:] != k[:-1]) | (i[1:] != i[:-1])
    k, i = k[keep], i[keep]
    out = np.zeros(cols + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(k, minlength=cols))
    return out.astype(np.int32), i.astype(np.int32)


def ref_canonical(rp, ci, cols):
    """rows ascending, repeats dropped: what two transposes leave"""
    t_rp, t_ci = ref_transpose(rp, ci, cols)
    return ref_transpose(t_rp, t_ci, len(rp) - 1)


def is_canonical(rp, ci):
    """every row strictly ascending"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    if ci.size < 2:
        return True
    inner = np.ones(ci.size, bool)
    inner[rp[:-1][rp[:-1] < ci.size]] = False            # the first entry of every row
    return bool(np.all(np.diff(ci)[inner[1:]] > 0))


def _row_of(rp, e):
    """largest r with rp[r] <= e: row_of of the kernels"""
    return int(np.searchsorted(rp, e, side="right")) - 1


# ---- the plan of a transpose ----------------------------------------------------------------------------------------
def plan(rp, ci, cols):
    """what bspgemm_matrix_transpose will do with A = (rp, ci) of `cols` columns, E = nnz(A) > 0:
         bits, passes, nbits   bits(cols - 1), radix passes and the digit bits of every pass
         tiles                 per first-pass tile (r_lo, r_hi, span, staged)
         keys, vals            the sorted pair list (k, i) that the dedup kernels read
         runs                  (first, last) sorted positions of every run of two or more equal pairs
         thread_runs, wave_runs, tile_runs   the runs that straddle a boundary of 16, 1024, 4096 sorted positions
         threads_keep_nothing, tiles_keep_nothing   threads (tiles) that hold pairs and keep none of them
         last_thread           "vector" | "scalar": the load_items path of the thread that owns the last pair
         fills                 per key change, in order: {pos, empty, wide, kind, seam}; pos = the sorted position of the
                               new key's first pair (E for the trailing fill), empty = the empty AT rows in front of it,
                               kind "leading" | "inner" | "trailing", seam = the left key is the last pair of the tile before
         wide_per_wave         the number of wide inner / leading fills per wave of 1024 pairs (only waves that have any)
         wide_same_call        the largest number of wide fills that one fill_rows call of one wave sees (same item index)
    """
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    rows, E = rp.size - 1, int(ci.size)
    assert E > 0 and rp[0] == 0 and rp[-1] == E and ci.min() >= 0 and ci.max() < cols
    bits = 0
    while bits < 31 and (1 << bits) < cols:
        bits += 1
    passes = 1 if bits <= DIGIT_BITS else (bits + DIGIT_BITS - 1) // DIGIT_BITS
    nbits = [min(DIGIT_BITS, bits - p * DIGIT_BITS) for p in range(passes)]
    tiles = []
    for t0 in range(0, E, TR_TILE):
        t1 = min(t0 + TR_TILE, E)
        lo, hi = _row_of(rp, t0), _row_of(rp, t1 - 1)
        lo, hi = min(lo, rows - 1), min(hi, rows - 1)
        tiles.append((lo, hi, hi - lo + 1, hi - lo + 1 < TR_STAGE_SPAN))
    i = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    o = np.argsort(ci, kind="stable")                    # the LSD sort is a stable sort by k of the CSR order
    keys, vals = ci[o], i[o]
    same = (keys[1:] == keys[:-1]) & (vals[1:] == vals[:-1])
    keep = np.concatenate([[True], ~same])
    starts = np.flatnonzero(keep)
    ends = np.concatenate([starts[1:], [E]]) - 1
    runs = [(int(a), int(b)) for a, b in zip(starts, ends) if b > a]

    def straddle(unit):
        return [r for r in runs if r[0] // unit != r[1] // unit]

    def keep_nothing(unit):
        return [u for u in range((E + unit - 1) // unit) if not keep[u * unit:(u + 1) * unit].any()]

    newkey = np.concatenate([[True], keys[1:] != keys[:-1]])
    fills = []
    for p in np.flatnonzero(newkey):
        p = int(p)
        pk = int(keys[p - 1]) if p else -1
        empty = int(keys[p]) - pk - 1
        fills.append({"pos": p, "empty": empty, "wide": empty >= FILL_WIDE, "kind": "inner" if p else "leading",
                      "seam": p > 0 and p % TR_TILE == 0})
    trailing = cols - int(keys[-1]) - 1
    fills.append({"pos": E, "empty": trailing, "wide": trailing >= FILL_WIDE, "kind": "trailing", "seam": False})
    wide_per_wave, same_call = {}, {}
    for f in fills[:-1]:
        if f["wide"]:
            w = f["pos"] // TR_WAVE
            wide_per_wave[w] = wide_per_wave.get(w, 0) + 1
            same_call[(w, f["pos"] % TR_ITEMS)] = same_call.get((w, f["pos"] % TR_ITEMS), 0) + 1
    return {"E": E, "bits": bits, "passes": passes, "nbits": nbits, "tiles": tiles, "keys": keys, "vals": vals, "runs": runs,
            "thread_runs": straddle(TR_ITEMS), "wave_runs": straddle(TR_WAVE), "tile_runs": straddle(TR_TILE),
            "threads_keep_nothing": keep_nothing(TR_ITEMS), "tiles_keep_nothing": keep_nothing(TR_TILE),
            "last_thread": "vector" if E % TR_ITEMS == 0 else "scalar", "fills": fills, "wide_per_wave": wide_per_wave,
            "wide_same_call": max(same_call.values()) if same_call else 0}


# ---- building cases -------------------------------------------------------------------------------------------------
def _case(rp, ci, rows, cols):
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    assert rp.size == rows + 1 and rp[0] == 0 and rp[-1] == ci.size
    rp.setflags(write=False)
    ci.setflags(write=False)
    return {"rp": rp, "ci": ci, "rows": rows, "cols": cols}


def _from_pairs(i, k, rows, cols, rng):
    """the CSR that holds the entries (i, k), repeats kept, every row in shuffled order"""
    i, k = np.asarray(i, np.int64), np.asarray(k, np.int64)
    o = np.lexsort((rng.random(i.size), i))
    rp = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=rows))])
    return _case(rp, k[o], rows, cols)


def _from_rows(rows_of_cols, cols):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows_of_cols])])
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows_of_cols]) if len(rows_of_cols) else np.zeros(0, np.int64)
    return _case(rp, ci, len(rows_of_cols), cols)


ENTRY_COUNTS = (1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193)


def case_entry_count(E):
    """E random entries of a 50 x 200 operand, unsorted with repeats: one pass"""
    rng = np.random.default_rng(9100 + E)
    return _from_pairs(rng.integers(0, 50, E), rng.integers(0, 200, E), 50, 200, rng)


WINDOW_SPANS = (8191, 8192, 8193)
WINDOW_KINDS = ("edge", "inner", "second")


def case_row_window(span, kind):
    """a tile of 300 entries whose rows span `span` rows (first and last included), the entries in between spread over
    80 rows of the window with one to three entries each, unsorted with repeats.
      edge    A has `span` rows: the tile begins in row 0 and ends in A's last row
      inner   A has 9000 rows, the window begins in row 400: empty rows before and behind it
      second  a first tile of 4096 entries in 16 rows; its last row runs 44 entries into the second tile, whose window is
              the one above, so A's row 0 lies in the staged tile and A's last row ends the unstaged one"""
    rng = np.random.default_rng(9200 + span + 7 * WINDOW_KINDS.index(kind))
    cols = 500
    head = {"edge": 0, "inner": 400, "second": 15}[kind]
    rows = {"edge": span, "inner": 9000, "second": 15 + span}[kind]
    first, last = head, head + span - 1
    mid = np.sort(rng.choice(np.arange(first + 1, last), 80, replace=False))
    lens = np.zeros(rows, np.int64)
    lens[mid] = rng.integers(1, 4, mid.size)
    lens[last] = 2
    lens[first] = 300 - int(lens.sum())                  # the window's first row takes what is left of the 300
    if kind == "second":
        lens[:15] = 270
        lens[15] += TR_TILE - 15 * 270                   # 46 entries that end the first tile
    i = np.repeat(np.arange(rows), lens)
    k = rng.integers(0, 40, i.size)                      # few distinct columns: repeats in most rows
    k[rng.integers(0, i.size, 30)] = cols - 1
    return _from_pairs(i, k, rows, cols, rng)


def case_few_columns(cols):
    """cols = 1 (no digit bit at all) or 2: 3000 rows of cols + 1 .. cols + 3 entries, so every row holds repeats"""
    rng = np.random.default_rng(9300 + cols)
    rows = 3000
    lens = rng.integers(cols + 1, cols + 4, rows)
    i = np.repeat(np.arange(rows), lens)
    return _from_pairs(i, rng.integers(0, cols, i.size), rows, cols, rng)


THREE_PASS = ("low", "middle", "top", "mixed")


def case_three_passes(which):
    """cols = 2^16 + 1: three passes of 8, 8 and 1 bits.  The keys differ only in the low digit, only in the middle one,
    only in the top one (0 and 2^16), or in any of them; every key is held by many of the 700 rows, with repeats, so the
    order of AT's col_idx is decided by the stability of every pass"""
    rng = np.random.default_rng(9400 + THREE_PASS.index(which))
    cols, rows = (1 << 16) + 1, 700
    low = np.array([0, 1, 2, 127, 128, 254, 255])
    pool = {"low": 0x3300 + low, "middle": (low << 8) + 0x5a, "top": np.array([0, 1 << 16]),
            "mixed": np.concatenate([low, low << 8, (low << 8) + low, [1 << 16]])}[which]
    E = 9000
    return _from_pairs(rng.integers(0, rows, E), rng.choice(pool, E), rows, cols, rng)


def _distinct_sorted_pairs(rng, n, rows, cols):
    code = np.sort(rng.choice(rows * cols, n, replace=False))
    return code // rows, code % rows                     # (k, i) in lexicographic order


DUP_PAIR_AT = (16, 1024, 4096)


def case_dup_pair(pos):
    """5000 sorted pairs, all distinct but those at the sorted positions pos - 1 and pos"""
    rng = np.random.default_rng(9500 + pos)
    rows, cols = 300, 200
    k, i = _distinct_sorted_pairs(rng, 4999, rows, cols)
    k, i = np.insert(k, pos - 1, k[pos - 1]), np.insert(i, pos - 1, i[pos - 1])
    return _from_pairs(i, k, rows, cols, rng)


def case_dup_run40():
    """5000 sorted pairs with one run of 40 equal ones at the positions 2053 .. 2092: the thread of the positions
    2064 .. 2079 keeps nothing"""
    rng = np.random.default_rng(9540)
    rows, cols = 300, 200
    k, i = _distinct_sorted_pairs(rng, 4961, rows, cols)
    k, i = np.insert(k, 2053, [k[2053]] * 39), np.insert(i, 2053, [i[2053]] * 39)
    return _from_pairs(i, k, rows, cols, rng)


def case_dup_row9000():
    """row 1 of a 3 x 50 operand holds column 7 nine thousand times (and 3 once); rows 0 and 2 hold a few columns, none
    behind (7, 1): the second and the third tile of sorted pairs keep nothing, and the thread that owns the last pair,
    which fills AT's trailing rows, keeps nothing either"""
    rng = np.random.default_rng(9550)
    i = np.concatenate([np.full(9001, 1), [0, 0, 2, 2]])
    k = np.concatenate([np.full(9000, 7), [3], [2, 7, 5, 5]])
    return _from_pairs(i, k, 3, 50, rng)


GAPS = (0, 1, 7, 8, 9, 63, 64, 65, 200)
GAP_ENDS = ((0, 0), (8, 1), (9, 8), (100, 9), (0, 1000))       # (leading, trailing) empty columns
# (empty columns in front of the key, sorted position of its first pair): the wide gaps at 53, 149 and 325 belong to the
# lanes 3, 9 and 20 of the first wave, each as the lane's sixth pair, so one fill_rows call sees all three; the one at
# 4096 has its left key in the tile before
_GAP_SPEC = ((0, 3), (1, 10), (7, 20), (8, 53), (9, 149), (63, 325), (64, 700), (65, 1500), (200, 4096), (8, 4100), (7, 5000))


def case_gaps(lead, trail):
    """5200 distinct sorted pairs whose keys leave the runs of empty AT rows of _GAP_SPEC between them, `lead` empty
    columns in front of the first key and `trail` behind the last"""
    rng = np.random.default_rng(9600 + lead + trail)
    E, rows = 5200, 3000
    key, keys, first = lead, [lead], [0]
    for gap, pos in _GAP_SPEC:
        key += gap + 1
        keys.append(key)
        first.append(pos)
    counts = np.diff(first + [E])
    k = np.repeat(keys, counts)
    i = np.concatenate([np.sort(rng.choice(rows, c, replace=False)) for c in counts])
    return _from_pairs(i, k, rows, key + 1 + trail, rng)


def case_hub_column():
    """9000 rows that each hold column 7 and one random other column of 300: the pairs of key 7 run through three tiles
    of the sorted list and fill whole waves of the scatter with one digit"""
    rng = np.random.default_rng(9700)
    rows, cols = 9000, 300
    i = np.repeat(np.arange(rows), 2)
    k = np.stack([np.full(rows, 7), rng.integers(0, cols, rows)], axis=1).ravel()
    return _from_pairs(i, k, rows, cols, rng)


TRANSPOSE_CASES = {}
for _e in ENTRY_COUNTS:
    TRANSPOSE_CASES["entries%d" % _e] = functools.partial(case_entry_count, _e)
for _kind in WINDOW_KINDS:
    for _s in WINDOW_SPANS:
        TRANSPOSE_CASES["window_%s%d" % (_kind, _s)] = functools.partial(case_row_window, _s, _kind)
for _c in (1, 2):
    TRANSPOSE_CASES["cols%d" % _c] = functools.partial(case_few_columns, _c)
for _w in THREE_PASS:
    TRANSPOSE_CASES["three_passes_%s" % _w] = functools.partial(case_three_passes, _w)
for _p in DUP_PAIR_AT:
    TRANSPOSE_CASES["dup_pair%d" % _p] = functools.partial(case_dup_pair, _p)
TRANSPOSE_CASES["dup_run40"] = case_dup_run40
TRANSPOSE_CASES["dup_row9000"] = case_dup_row9000
for _lead, _trail in GAP_ENDS:
    TRANSPOSE_CASES["gaps_lead%d_trail%d" % (_lead, _trail)] = functools.partial(case_gaps, _lead, _trail)
TRANSPOSE_CASES["hub_column"] = case_hub_column


@functools.lru_cache(maxsize=None)
def transpose_case(name):
    return TRANSPOSE_CASES[name]()


@functools.lru_cache(maxsize=None)
def transpose_expected(name):
    """(AT, canonical A) of the named case, each (row_ptr, col_idx); computed once and read-only"""
    c = transpose_case(name)
    out = ref_transpose(c["rp"], c["ci"], c["cols"]), ref_canonical(c["rp"], c["ci"], c["cols"])
    for pair in out:
        for a in pair:
            a.setflags(write=False)
    return out


# ---- the canonical-form check ---------------------------------------------------------------------------------------
def check_plan(rp, E):
    """per tile of k_set_flags over an operand of E entries: (rb, rl, span, staged)"""
    rp = np.asarray(rp, np.int64)
    rows = rp.size - 1
    first = [_row_of(rp, t0) for t0 in range(0, E, SEL_TILE)]
    out = []
    for t, rb in enumerate(first):
        rl = rows - 1 if (t + 1) * SEL_TILE >= E else first[t + 1]
        out.append((rb, rl, rl - rb + 1, rl - rb + 1 <= SEL_STAGE))
    return out


def position_class(p, E):
    """where the check of the pair (p - 1, p) happens: the lane's entry index k (0: the left neighbour is before[j]), and
    whether p begins a wave step, a wave, a tile; scalar: the lane's load4 takes the entry-by-entry path even when col_idx
    is 16-byte aligned (fewer than four entries remain)"""
    return {"k": p % 4, "step": p % SEL_STEP == 0, "wave": p % SEL_WAVE == 0, "tile": p % SEL_TILE == 0,
            "scalar": p - p % 4 + 3 >= E}


CHECK_E = (4200, 4201)                                   # E % 4 == 0, and E % 4 == 1: the last lane loads one entry


def check_positions(E):
    return (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, E - 1)


def _ascending_rows(rng, lens, cols):
    return [np.sort(rng.choice(cols, int(n), replace=False)) for n in lens]


@functools.lru_cache(maxsize=None)
def check_base(E):
    """a canonical square operand of E entries in rows of 6 .. 14 (the last one may be longer), no row beginning at any of
    check_positions(E): every such entry is interior to its row"""
    rng = np.random.default_rng(9800 + E)
    avoid = set(check_positions(E))
    lens, at = [], 0
    while E - at > 20:
        n = int(rng.integers(6, 15))
        while at + n in avoid:
            n += 1
        lens.append(n)
        at += n
    lens.append(E - at)
    n = len(lens)
    assert n > max(lens)
    return _from_rows(_ascending_rows(rng, lens, n), n)


@functools.lru_cache(maxsize=None)
def check_control(E):
    """a canonical square operand of E entries in which every position of check_positions(E) begins a row whose first
    column equals (every other one: is one below) the last column of the row before"""
    rng = np.random.default_rng(9850 + E)
    starts = sorted(check_positions(E))
    lens, at = [], 0
    for s in starts + [E]:
        while s - at > 14:
            lens.append(int(rng.integers(6, 12)))
            at += lens[-1]
        if s > at:
            lens.append(s - at)
            at = s
    n = len(lens)
    rp = np.concatenate([[0], np.cumsum(lens)])
    rows, q = [], 0
    for r, m in enumerate(lens):
        if r > 0 and int(rp[r]) in starts:
            first = int(rows[-1][-1]) - q % 2
            q += 1
            rest = np.sort(rng.choice(np.arange(first + 1, n), m - 1, replace=False))
            rows.append(np.concatenate([[first], rest]).astype(np.int64))
        else:                                            # (the lower half: room for the row behind it to ascend)
            rows.append(np.sort(rng.choice(np.arange(5, n // 2), m, replace=False)))
    assert q == len(starts)
    return _from_rows(rows, n)


def with_defect(rp, ci, p, kind):
    """a copy of col_idx with one defect at the interior entry p: "repeat" ci[p] = ci[p - 1], "descent" the two swapped"""
    rp = np.asarray(rp, np.int64)
    r = _row_of(rp, p)
    assert rp[r] < p < rp[r + 1], "entry %d is not interior to its row" % p
    out = np.array(ci, np.int32)
    if kind == "repeat":
        out[p] = out[p - 1]
    elif kind == "descent":
        out[p - 1], out[p] = ci[p], ci[p - 1]
    else:
        raise ValueError(kind)
    return out


@functools.lru_cache(maxsize=None)
def check_partner(E):
    """a canonical operand of the shape of check_base(E) that shares about half of every row with it"""
    x = check_base(E)
    rng = np.random.default_rng(9870 + E)
    n, rows = x["rows"], []
    for r in range(n):
        row = x["ci"][x["rp"][r]:x["rp"][r + 1]]
        rows.append(np.union1d(row[rng.random(row.size) < 0.5], rng.choice(n, 4, replace=False)))
    return _from_rows(rows, n)


@functools.lru_cache(maxsize=None)
def check_unstaged(control):
    """a 4250 x 64 operand: 300 entries in 30 rows, 4200 empty rows, then 200 entries in 20 rows -- one tile that spans
    more than 4096 rows.  Returns (case, p): p = an entry behind the run of empty rows, interior to its row and the first
    of its lane's four -- or (control) the first entry of the first row behind the run, whose column equals the last
    column in front of the run"""
    rng = np.random.default_rng(9900 + int(control))
    lens = [10] * 30 + [0] * 4200 + [10] * 20
    cols = 64
    rows = _ascending_rows(rng, lens, cols)
    if not control:
        return _from_rows(rows, cols), 300 + 4
    v = 30
    rows[29] = np.concatenate([np.sort(rng.choice(v, 9, replace=False)), [v]])
    rows[4230] = np.concatenate([[v], np.sort(rng.choice(np.arange(v + 1, cols), 9, replace=False))])
    return _from_rows(rows, cols), 300


def dot_operands(x, cols, role):
    """(a, b, f, a_rows, b_rows, cols, f_cols), the arguments of dot_ref.dot_ref, of a masked dot product in which the
    operand x = (rp, ci) of n rows and `cols` columns plays `role` (0: A, 1: B, 2: F) and every entry of x decides a value
    of the result:
      A or B   the other side is one full row, longer than any row of x, and the mask pairs it with every row of x, so
               C holds the length of every row of x: a column walked twice, or skipped behind a larger one, changes it
      F        A_i n B_j = {0} for every pair: C holds x's pattern with ones, once per entry and in ascending order"""
    rp, ci = x
    n = len(rp) - 1
    full = (np.array([0, cols], np.int32), np.arange(cols, dtype=np.int32))
    if role == 0:
        return x, full, (np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32)), n, 1, cols, 1
    if role == 1:
        return full, x, (np.array([0, n], np.int32), np.arange(n, dtype=np.int32)), 1, n, cols, n
    a = (2 * np.arange(n + 1, dtype=np.int32), np.tile(np.array([0, 2], np.int32), n))
    b = (2 * np.arange(cols + 1, dtype=np.int32), np.tile(np.array([0, 1], np.int32), cols))
    return a, b, x, n, cols, 3, cols
