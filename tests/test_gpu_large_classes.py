"""The one-wave kernel's capacity classes of 10 to 32 chunks (csrc/wave_rows.inc), and the ONE slot buffer that holds every
ranked level of a row in turn: a level is built in the words its parent was read from, and the buffer must be all zero
again on every way out of a row -- sparse, few shared slots, mask level, the count pass settled by its hash filter or by
the sweeps.  A word left set shows up in the next row of the same wave.

Per column count (one per LEVELS value the library compiles: 1 .. 5) and per class, 16 hand-built rows ("templates"), each
its own 1 .. 3 rows of B:
  - at the class's lowest and at its highest product count, in this order: a row that takes the mask level (several columns
    per 32-column slot, repeated columns within and across chunks, column 0 and the last column), a sparse row, a row with
    exactly 4 products more than slots (shared_max of 10 and 12 chunks), one with 5, and a mask-level row again;
  - off a multiple of 64 products: rows with 16 and 17 products more than slots (the setter's maximum and one more), a
    mask-level row and a sparse row, and rows with 8 and 9 more (shared_max of 14 and 16 chunks, and one more).
  With too few columns for F slots (4096 columns: one level, no ranked level at all) every row is a mask-level row.
test_large_classes_templates multiplies the templates as they are (16 rows per class: one row per wave) in both flows,
through the complemented mask and the accumulating product, and with shared_slots forced to 0 and to its maximum.
test_large_classes_runs gives every class 2560 rows, each a template drawn at random, so that every wave owns two rows
(launch_cfg: rows per wave = ceil(rows / 2048)) and every ordered pair of row kinds meets in many waves, whatever order the
prepass lists the rows in; the expected product is the oracle's row of the template.  Everything is compared bit for bit
with the CPU oracle."""
import numpy as np
import pytest

import gen

W = gen.WAVE_CHUNKS
CLASSES = (10, 12, 14, 16, 20, 24, 28, 32)        # chunks
COLS = (4096, 131072, 4194304, 16777217, 268435457)
LEVELS = {4096: 1, 131072: 2, 4194304: 3, 16777217: 4, 268435457: 5}
RUN_ROWS = 2560                                   # per class: two rows per wave, 1280 waves
KINDS = ("mask", "sparse", "few4", "few5", "mask")


def _distinct(rng, n, hi):
    """n distinct integers of [0, hi), in random order"""
    if hi <= 4 * n:
        return rng.permutation(hi)[:n].astype(np.int64)
    got = np.unique(rng.integers(0, hi, size=2 * n + 8))
    assert got.size >= n
    return rng.permutation(got)[:n].astype(np.int64)


def _row(rng, kind, F, cols):
    """the products of one row, in product order"""
    nst = cols // 32                                                    # whole 32-column slots
    if kind != "mask" and nst < 2 * F:
        kind = "mask"
    if kind == "mask":
        G = max(1, min(F // 3, nst))
        slots = _distinct(rng, G, nst)
        prods = 32 * slots[rng.integers(0, G, size=F)] + rng.integers(0, 32, size=F)
        prods[0], prods[1] = 0, cols - 1
        prods[3] = prods[2]                                             # a repeat within a chunk
        prods[F - 1] = prods[4]                                         # ... and across the row's chunks
        return prods
    e = {"sparse": 0}.get(kind) if kind == "sparse" else int(kind[3:])
    slots = _distinct(rng, F - e, nst)
    off = rng.integers(0, 31, size=F - e)
    prods = np.concatenate([32 * slots + off, 32 * slots[:e] + off[:e] + 1])   # e slots of two columns
    assert prods.size == F and np.unique(prods >> 5).size == F - e and np.unique(prods).size == F
    return prods[rng.permutation(F)]


def build_templates(cols, seed):
    rng = np.random.default_rng(seed)
    b_rp, b_ci, t_rows, t_class, t_kind = [0], [], [], [], []
    for ch in CLASSES:
        lo, hi = 64 * W[W.index(ch) - 1] + 1, 64 * ch
        plan = [(k, lo) for k in KINDS] + [(k, hi) for k in KINDS]
        plan += [("few16", hi - 27), ("few17", hi - 27), ("mask", hi - 27), ("sparse", hi - 91), ("few8", lo + 70), ("few9", hi - 1)]
        assert len(plan) == 16
        for kind, F in plan:
            prods = _row(rng, kind, F, cols)
            parts = int(rng.integers(1, 4))
            cuts = np.sort(rng.integers(0, F + 1, size=parts - 1))
            mine = []
            for piece in np.split(prods, cuts):
                mine.append(len(b_rp) - 1)
                b_ci.append(piece)
                b_rp.append(b_rp[-1] + piece.size)
            t_rows.append(mine)
            t_class.append(ch)
            t_kind.append(kind)
    b_ci = np.concatenate(b_ci)
    assert b_ci.min() >= 0 and b_ci.max() < cols
    return {"b_rp": np.asarray(b_rp, np.int32), "b_ci": b_ci.astype(np.int32), "t_rows": t_rows, "t_class": t_class,
            "t_kind": t_kind, "cols": cols}


def _a_of(s, picks):
    """A whose row i is template picks[i]"""
    a_ci = [s["t_rows"][t] for t in picks]
    a_rp = np.concatenate([[0], np.cumsum([len(x) for x in a_ci])]).astype(np.int32)
    return a_rp, np.concatenate(a_ci).astype(np.int32)


_CASES = {}


def case(cols):
    """the templates, their A and the oracle's product for a column count, built once"""
    if cols not in _CASES:
        from oracle import oracle as O
        s = build_templates(cols, seed=9300 + COLS.index(cols))
        s["a_rp"], s["a_ci"] = _a_of(s, range(len(s["t_rows"])))
        s["F"] = gen.row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, s["a_rp"].size - 1)
        s["want"] = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
        _CASES[cols] = s
    return _CASES[cols]


def _keys(rp, ci):
    rp = np.asarray(rp, np.int64)
    return (np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp)) << 32) | np.asarray(ci, np.int64)


def _csr(keys, R):
    counts = np.bincount((keys >> 32).astype(np.int64), minlength=R)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), (keys & 0xffffffff).astype(np.int32)


def _compare(tag, got, want, failures):
    crp, cci = got
    erp, eci = want
    if not np.array_equal(crp, erp):
        bad = np.flatnonzero(crp != erp)[:5] if crp.shape == erp.shape else "shape"
        failures.append("%s: row_ptr differs (first at %s)" % (tag, bad))
    elif not np.array_equal(cci, eci):
        failures.append("%s: col_idx differs (first at %s)" % (tag, np.flatnonzero(cci != eci)[:5]))


# ---------------------------------------------------------------- without a GPU -----------------------------------
@pytest.mark.parametrize("cols", COLS)
def test_large_classes_templates_cover(cols):
    """every class of 10 .. 32 chunks holds its 16 rows, at both ends of the class; with columns enough, rows with exactly
    0, 4, 5, 8, 9, 16 and 17 products more than slots and mask-level rows with repeats; the instance is the one named"""
    s = build_templates(cols, seed=9300 + COLS.index(cols))
    assert gen.wave_levels(cols) == LEVELS[cols]
    a_rp, a_ci = _a_of(s, range(len(s["t_rows"])))
    F = gen.row_products(a_rp, a_ci, s["b_rp"], 0, a_rp.size - 1)
    bins = gen.row_bins(F, cols)
    b_rp, b_ci = s["b_rp"].astype(np.int64), s["b_ci"].astype(np.int64)
    for ch in CLASSES:
        rows = np.flatnonzero(bins == W.index(ch) + 1)
        assert rows.size == 16 and [s["t_class"][i] for i in rows] == [ch] * 16
        assert F[rows].min() == 64 * W[W.index(ch) - 1] + 1 and F[rows].max() == 64 * ch
        extra, repeats = [], []
        for i in rows:
            c = b_ci[b_rp[a_ci[a_rp[i]]]:b_rp[a_ci[a_rp[i + 1] - 1] + 1]]
            assert c.size == F[i]
            extra.append(c.size - np.unique(c >> 5).size)
            repeats.append(c.size - np.unique(c).size)
        assert max(repeats) > 0 and max(extra) > 40
        if cols // 32 >= 2 * 64 * ch:
            assert [extra[k] for k in (1, 2, 3, 6, 7, 8, 10, 11, 13, 14, 15)] == [0, 4, 5, 0, 4, 5, 16, 17, 0, 8, 9], (ch, extra)


# ---------------------------------------------------------------- on the GPU ---------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import bspgemm
    c = bspgemm.Context(0)
    c.set_option("small_path", 0)
    yield c
    c.set_option("shared_slots", -1)
    c.set_flow("auto")
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cols", COLS)
def test_large_classes_templates(ctx, cols):
    """16 rows per class, one per wave: both flows with shared_slots at the per-class table, forced off and forced to its
    maximum (three equal results); then the complemented mask and the accumulating product over the same rows"""
    s = case(cols)
    R = s["F"].size
    rng = np.random.default_rng(500 + COLS.index(cols))
    wk = _keys(*s["want"])
    # Drop: a third of every row's columns and as many others
    mk = np.unique(np.concatenate([wk[rng.random(wk.size) < 0.33],
                                   (rng.integers(0, R, size=wk.size // 3) << 32) | rng.integers(0, cols, size=wk.size // 3)]))
    f_rp, f_ci = _csr(mk, R)
    want_drop = _csr(np.setdiff1d(wk, mk), R)
    # Insert: per row a column next to a product's (same slot), a product's own column, others, and one beyond B's columns
    pick = wk[rng.random(wk.size) < 0.01]
    near = np.minimum((pick & ~np.int64(31)) | rng.integers(0, 32, size=pick.size), (pick & ~np.int64(0xffffffff)) | (cols - 1))
    rows = rng.integers(0, R, size=4 * R).astype(np.int64)
    dk = np.unique(np.concatenate([near, wk[rng.random(wk.size) < 0.01], (rows << 32) | rng.integers(0, cols, size=rows.size)]))
    d_rp, d_ci = _csr(np.sort(np.concatenate([dk, (np.arange(R, dtype=np.int64) << 32) | (cols + 7)])), R)
    order = np.concatenate([rng.permutation(np.arange(d_rp[i], d_rp[i + 1])) for i in range(R)])      # D's rows unsorted
    want_ins = _csr(np.union1d(wk, dk), R)
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    Fm = ctx.upload(f_rp, f_ci, cols)
    D = ctx.upload(d_rp.astype(np.int32), d_ci[order], cols)
    failures = []
    try:
        for opt in (-1, 0, 16):
            ctx.set_option("shared_slots", opt)
            for flow in ("upper-bound", "exact"):
                ctx.set_flow(flow)
                C = ctx.multiply(A, B)
                st = ctx.stats()
                got = C.download()
                C.free()
                _compare("shared_slots %d, %s flow" % (opt, flow), got, s["want"], failures)
                assert st["small_path"] == 0 and st["rows_per_bin"] == gen.expected_bins(s["F"], cols)
            ctx.set_flow("auto")
            C = ctx.multiply_masked(A, B, Fm, complement=True)
            got = C.download()
            C.free()
            _compare("shared_slots %d, complemented mask" % opt, got, want_drop, failures)
            C = ctx.multiply_accumulate(A, B, D)
            got = C.download()
            C.free()
            _compare("shared_slots %d, accumulate" % opt, got, want_ins, failures)
    finally:
        ctx.set_flow("auto")
        ctx.set_option("shared_slots", -1)
        for m in (A, B, Fm, D):
            m.free()
    assert not failures, "%d columns (LEVELS %d):\n  %s" % (cols, LEVELS[cols], "\n  ".join(failures))


@pytest.mark.gpu
@pytest.mark.parametrize("cols", COLS)
def test_large_classes_runs(ctx, cols):
    """two rows per wave, templates drawn at random: a word that a row leaves set in the slot buffer, the top bitmap or the
    starts words is in the way of the row after it"""
    s = case(cols)
    T = len(s["t_rows"])
    rng = np.random.default_rng(700 + COLS.index(cols))
    picks = np.concatenate([rng.integers(16 * k, 16 * k + 16, size=RUN_ROWS) for k in range(len(CLASSES))])
    picks = picks[rng.permutation(picks.size)]
    assert T == 16 * len(CLASSES) and all(gen.wave_rpw(RUN_ROWS, ch) == 2 for ch in CLASSES)
    a_rp, a_ci = _a_of(s, picks)
    wrp, wci = s["want"]
    n = np.diff(wrp)[picks]
    erp = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    eci = wci[np.repeat(wrp[:-1][picks] - erp[:-1], n) + np.arange(erp[-1])]     # row i of the product: template picks[i]'s
    A = ctx.upload(a_rp, a_ci, s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    failures = []
    try:
        for flow in ("upper-bound", "exact"):
            ctx.set_flow(flow)
            C = ctx.multiply(A, B)
            st = ctx.stats()
            got = C.download()
            C.free()
            _compare("%s flow" % flow, got, (erp, eci), failures)
            assert st["small_path"] == 0 and st["rows_per_bin"] == gen.expected_bins(s["F"][picks], cols)
    finally:
        ctx.set_flow("auto")
        A.free()
        B.free()
    assert not failures, "%d columns (LEVELS %d):\n  %s" % (cols, LEVELS[cols], "\n  ".join(failures))
