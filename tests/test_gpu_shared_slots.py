"""The one-wave kernel's emit for rows of few shared slots (csrc/wave_rows.inc, BSPGEMM_OPT_SHARED_SLOTS): a row with
1 .. shared_max products more than 32-column slots is put in order from its columns alone, without the mask level.

Hand-built rows, a few hundred per capacity class of 1, 2, 5, 8 and 16 chunks (the path exists) and of 20 chunks (it does
not), at the column counts that give LEVELS 2 to 5 and the wide top of three levels.  Every row is a sparse row -- each
product alone in its slot -- but for the slots named by its pattern:
  - one slot of 2, 3 and 32 distinct columns, first, last and inside the row, two of its products next to each other in a
    chunk or in the first and the last chunk;
  - 2 .. 17 slots of two columns: exactly shared_max and shared_max + 1 for the forced values 1, 4, 16 and the per-class
    values 8 and 4;
  - a shared slot and, elsewhere, a column two or three times alone in its slot;
  - a column twice inside a shared slot; a plain sparse row; a row far above every shared_max;
  - F at both ends of the class and off a multiple of 64 (tail lanes); column 0 and the last column.
Each product is compared bit for bit with the CPU oracle under option 0, the per-class table (-1) and forced 1, 4 and 16, in
both flows; one shape each goes through the complemented mask (Drop) and the accumulating product (Insert)."""
import numpy as np
import pytest

import gen

W = gen.WAVE_CHUNKS
CLASSES = (1, 2, 5, 8, 16, 20)                    # chunks
COLS = (131072, 4194304, 16777216, 16777217, 268435457)
INSTANCE = {131072: (2, 2), 4194304: (3, 2), 16777216: (3, 8), 16777217: (4, 2), 268435457: (5, 2)}   # (LEVELS, TWP)
OPTIONS = (0, -1, 1, 4, 16)
PAIRS = (2, 3, 4, 5, 8, 9, 16, 17)                # slots of two columns in one row


def patterns():
    """(groups, where, place): groups = the offsets' labels of every slot that is not one product alone (equal labels: the
    same column); where the first group sits among the row's slots; where two of its products sit among the products"""
    out = []
    for m in (2, 3, 32):
        for where in ("first", "last", "mid"):
            for place in ("same", "diff"):
                out.append(([list(range(m))], where, place))
    for k in PAIRS:
        out.append(([[0, 1]] * k, "mid", "any"))
    out.append(([[0, 1, 2]] * 4, "first", "any"))                       # 8 more products than slots in 4 slots
    out.append(([[0, 1, 2, 3, 4]] * 2 + [[0, 1]], "last", "diff"))      # 9 in 3
    for place in ("same", "diff"):
        out.append(([[0, 1], [5, 5]], "mid", place))                    # a repeat alone in its slot beside a shared slot
        out.append(([[7, 7, 7], [0, 1, 2]], "first", place))
        for g in ([0, 0, 1], [0, 1, 1], [0, 0, 1, 1], [0, 1, 2, 2, 2]):  # a repeat inside a shared slot
            out.append(([g], "mid", place))
            out.append(([g, [0, 1]], "last", place))
    out.append(([], "mid", "any"))                                      # sparse
    out.append(([[0, 1]] * 40, "mid", "any"))                           # above every shared_max
    return out


def _row(rng, F, cols, groups, where, place, col0, col_last):
    """the products of one row, in product order"""
    nslot_total = (cols + 31) // 32
    last_valid = (cols - 1) % 32 + 1                                    # columns of the last slot
    groups = [list(g) for g in groups]
    singles = F - sum(map(len, groups))
    assert singles >= 0
    nitems = len(groups) + singles
    slots = np.unique(rng.integers(0, nslot_total - 1, size=2 * nitems + 8))
    slots = np.sort(rng.permutation(slots)[:nitems])
    assert slots.size == nitems
    # which item (slot of the row, ascending) every group takes
    fixed = {"first": 0, "last": nitems - 1}.get(where) if groups else None
    free = [int(i) for i in rng.permutation(nitems) if i != fixed]
    at = [fixed if gi == 0 and fixed is not None else free.pop() for gi in range(len(groups))]
    item_group = dict(zip(at, groups))
    if col0:
        slots[0] = 0
    if col_last and len(set(item_group.get(nitems - 1, [0]))) <= last_valid:
        slots[-1] = nslot_total - 1
    else:
        col_last = False
    prods, tagged = [], []
    for it in range(nitems):
        s = int(slots[it])
        valid = last_valid if s == nslot_total - 1 else 32
        g = item_group.get(it)
        if g is None:
            off = [int(rng.integers(0, valid))]
            if col0 and it == 0:
                off = [0]
            if col_last and it == nitems - 1:
                off = [valid - 1]
        else:
            labels = sorted(set(g))
            offs = sorted(int(x) for x in rng.permutation(valid)[:len(labels)])
            if col0 and it == 0:
                offs[0] = 0
            if col_last and it == nitems - 1:
                offs[-1] = valid - 1
            assert len(set(offs)) == len(labels)
            off = [offs[labels.index(x)] for x in g]
            if at and it == at[0]:
                tagged = [len(prods), len(prods) + 1]
        prods.extend(32 * s + o for o in off)
    prods = np.asarray(prods, np.int64)
    assert prods.size == F and prods.min() >= 0 and prods.max() < cols
    perm = rng.permutation(F)                                           # order[k] = prods[perm[k]]
    if tagged and place in ("same", "diff") and F >= 4:
        n = F
        if place == "same":
            c = int(rng.integers(0, (n + 63) // 64))
            lo, hi = 64 * c, min(64 * c + 64, n)
            t = int(rng.integers(lo, max(hi - 1, lo + 1)))
            want = [t, min(t + 1, n - 1)]
        else:
            want = [int(rng.integers(0, min(64, n - 1))), int(rng.integers(max(64 * ((n - 1) // 64), 1), n))]
        for src, dst in zip(tagged, want):
            p = int(np.flatnonzero(perm == src)[0])
            perm[[p, dst]] = perm[[dst, p]]
    return prods[perm]


def build_case(cols, seed):
    """A (one row per hand-built row, 1 .. 3 nonzeros) and B (the rows' products, split over that many B rows)"""
    rng = np.random.default_rng(seed)
    a_rp, a_ci, b_rp, b_ci, rows_F = [0], [], [0], [], []
    for ch in CLASSES:
        prev = W[W.index(ch) - 1] if W.index(ch) > 0 else 0
        Fs = (37, 57, 64) if ch == 1 else (64 * prev + 1, 64 * ch - 27, 64 * ch)
        k = 0
        for groups, where, place in patterns():
            for F in Fs + Fs:
                if sum(map(len, groups)) > F:
                    continue
                k += 1
                prods = _row(rng, F, cols, groups, where, place, col0=k % 4 in (1, 3), col_last=k % 4 in (2, 3))
                parts = int(rng.integers(1, 4))
                cuts = np.sort(rng.integers(0, prods.size + 1, size=parts - 1))
                for piece in np.split(prods, cuts):
                    a_ci.append(len(b_rp) - 1)
                    b_ci.append(piece)
                    b_rp.append(b_rp[-1] + piece.size)
                a_rp.append(len(a_ci))
                rows_F.append(prods.size)
    return {"a_rp": np.asarray(a_rp, np.int32), "a_ci": np.asarray(a_ci, np.int32), "b_rp": np.asarray(b_rp, np.int32),
            "b_ci": np.concatenate(b_ci).astype(np.int32), "F": np.asarray(rows_F, np.int64), "cols": cols}


_CASES = {}


def case(cols):
    """the operands and the oracle's product for a column count, built once"""
    if cols not in _CASES:
        from oracle import oracle as O
        s = build_case(cols, seed=9100 + COLS.index(cols))
        s["want"] = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols)
        _CASES[cols] = s
    return _CASES[cols]


def _keys(rp, ci):
    rp = np.asarray(rp, np.int64)
    return (np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp)) << 32) | np.asarray(ci, np.int64)


def _csr(keys, R):
    counts = np.bincount((keys >> 32).astype(np.int64), minlength=R)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), (keys & 0xffffffff).astype(np.int32)


# ---------------------------------------------------------------- without a GPU -----------------------------------
def test_shared_slots_cases_cover():
    """the generator builds what the module promises: per class a few hundred rows inside the class, rows with exactly 1,
    2, 4, 5, 8, 9, 16, 17 products more than slots, repeats, column 0 and the last column"""
    cols = COLS[0]
    s = build_case(cols, seed=9100)
    F = s["F"]
    bins = gen.row_bins(F, cols)
    a_rp, b_rp, b_ci = s["a_rp"], s["b_rp"].astype(np.int64), s["b_ci"].astype(np.int64)
    extra, repeats, has0, has_last = [], [], [], []
    for i in range(F.size):
        lo, hi = b_rp[s["a_ci"][a_rp[i]]], b_rp[s["a_ci"][a_rp[i + 1] - 1] + 1]
        c = b_ci[lo:hi]
        assert c.size == F[i]
        extra.append(c.size - np.unique(c >> 5).size)
        repeats.append(c.size - np.unique(c).size)
        has0.append((c == 0).any())
        has_last.append((c == cols - 1).any())
    extra, repeats = np.asarray(extra), np.asarray(repeats)
    for ch in CLASSES:
        rows = bins == W.index(ch) + 1
        assert 200 <= rows.sum() <= 400, (ch, int(rows.sum()))
        assert (F[rows] % 64 != 0).any() and (F[rows] % 64 == 0).any()
        for e in (0, 1, 2, 4, 5, 8, 9, 16, 17, 31) + ((40,) if ch > 1 else ()):
            assert (extra[rows] == e).any(), (ch, e)
        assert ((repeats > 0) & (extra > repeats) & rows).any() and (np.asarray(has0) & rows).any()
        assert (np.asarray(has_last) & rows).any()


# ---------------------------------------------------------------- on the GPU ---------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import bspgemm
    c = bspgemm.Context(0)
    c.set_option("small_path", 0)
    yield c
    c.set_option("shared_slots", -1)
    c.close()


def _compare(tag, got, want, failures):
    crp, cci = got
    erp, eci = want
    if not np.array_equal(crp, erp):
        bad = np.flatnonzero(crp != erp)[:5] if crp.shape == erp.shape else "shape"
        failures.append("%s: row_ptr differs (first at %s)" % (tag, bad))
    elif not np.array_equal(cci, eci):
        failures.append("%s: col_idx differs (first at %s)" % (tag, np.flatnonzero(cci != eci)[:5]))


@pytest.mark.gpu
@pytest.mark.parametrize("cols", COLS)
def test_shared_slots_product(ctx, cols):
    s = case(cols)
    assert (gen.wave_levels(cols), gen.wave_top_words(cols)) == INSTANCE[cols]
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    failures = []
    try:
        for opt in OPTIONS:
            ctx.set_option("shared_slots", opt)
            assert ctx.get_option("shared_slots") == opt
            for flow in ("upper-bound", "exact"):
                ctx.set_flow(flow)
                C = ctx.multiply(A, B)
                st = ctx.stats()
                got = C.download()
                C.free()
                _compare("shared_slots %d, %s flow" % (opt, flow), got, s["want"], failures)
                assert st["small_path"] == 0 and st["rows_per_bin"] == gen.expected_bins(s["F"], cols)
    finally:
        ctx.set_flow("auto")
        A.free()
        B.free()
    assert not failures, "%d columns:\n  %s" % (cols, "\n  ".join(failures))


@pytest.mark.gpu
def test_shared_slots_complement(ctx):
    """Drop: a third of every row's columns and as many others are masked out of the rows the new emit staged"""
    cols = 4194304
    s = case(cols)
    rng = np.random.default_rng(77)
    R = s["F"].size
    wk = _keys(*s["want"])
    mk = np.unique(np.concatenate([wk[rng.random(wk.size) < 0.33],
                                   (rng.integers(0, R, size=wk.size // 3) << 32) | rng.integers(0, cols, size=wk.size // 3)]))
    f_rp, f_ci = _csr(mk, R)
    want = _csr(np.setdiff1d(wk, mk), R)
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    Fm = ctx.upload(f_rp, f_ci, cols)
    failures = []
    try:
        for opt in OPTIONS:
            ctx.set_option("shared_slots", opt)
            C = ctx.multiply_masked(A, B, Fm, complement=True)
            got = C.download()
            C.free()
            _compare("shared_slots %d" % opt, got, want, failures)
    finally:
        for m in (A, B, Fm):
            m.free()
    assert not failures, "\n  ".join(failures)


@pytest.mark.gpu
def test_shared_slots_accumulate(ctx):
    """Insert: D's rows bring columns into the products' slots (new shared slots), repeat columns of the product, and
    hold columns outside [0, cols) that are dropped"""
    cols = 131072
    s = case(cols)
    rng = np.random.default_rng(78)
    R = s["F"].size
    wk = _keys(*s["want"])
    pick = wk[rng.random(wk.size) < 0.01]
    near = (pick & ~np.int64(31)) | rng.integers(0, 32, size=pick.size)      # another column of a product's slot
    same = wk[rng.random(wk.size) < 0.01]
    rows = rng.integers(0, R, size=2 * R).astype(np.int64)
    far = (rows << 32) | rng.integers(0, cols, size=rows.size)
    dk = np.concatenate([near, same, same[::2], far])
    d_rows = np.concatenate([dk >> 32, rows[:R]])
    d_cols = np.concatenate([dk & 0xffffffff, rng.integers(cols, cols + 1000, size=R)])   # beyond B's columns: dropped
    perm = rng.permutation(d_rows.size)
    d_rows, d_cols = d_rows[perm], d_cols[perm]
    order = np.argsort(d_rows, kind="stable")
    d_rp = np.concatenate([[0], np.cumsum(np.bincount(d_rows, minlength=R))]).astype(np.int32)
    d_ci = d_cols[order].astype(np.int32)
    want = _csr(np.union1d(wk, dk), R)
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    D = ctx.upload(d_rp, d_ci, cols)
    failures = []
    try:
        for opt in OPTIONS:
            ctx.set_option("shared_slots", opt)
            C = ctx.multiply_accumulate(A, B, D)
            got = C.download()
            C.free()
            _compare("shared_slots %d" % opt, got, want, failures)
    finally:
        for m in (A, B, D):
            m.free()
    assert not failures, "\n  ".join(failures)
