"""The tuning knobs change no result, only which kernels produce it (include/bspgemm.h, bspgemm_set_option): every
combination of flow x PADDED_ROWS x BLOCKED_EXTENTS x SMALL_PATH x CHECK x CLASS_STREAMS (3 x 2 x 2 x 3 x 2 x 2 = 144) on the
shapes where the kernels have special cases, compared bit for bit with the CPU oracle, and the masked product over its 16.

Every combination also asserts the path that ran (bspgemm_stats, bspgemm_matrix_uses_*), derived from the knobs and the
shape the way csrc/multiply.hip decides it, so that a knob the library ignored fails instead of passing vacuously:
  small-product path  flow not exact, SMALL_PATH != 0, 0 < R <= 2^17, nnz(A) <= 32768 (the whole A), for -1 also
                      nnz(A) x B's mean row length <= 32768 -- and the product fits on the device (<= 65536 products,
                      <= 2048 in every row; otherwise it bails to the general flow)
  general flow        flow 2 for exact, 1 otherwise (auto does not fall back at these sizes); padded iff PADDED_ROWS = 1
                      and nnz(B) > 0; prepass kernel = BLOCKED_EXTENTS; checked = CHECK; class streams = CLASS_STREAMS;
                      rows per capacity class exactly as the host computes them from F_i
Each combination starts from a fresh operand (uploaded again, or every other time invalidated), because padding and the
blocked table are decided on first use as B; every result is freed before the next multiply, so results come from the
context's cache, and shapes with an interior row range alternate a full and a smaller product of varying size.

A caller's stream (bspgemm_set_stream) with the class launches forked over three streams behind it is tested last.
"""
import itertools
import os

import numpy as np
import pytest

import bspgemm
import gen
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FLOW_ID = {"upper-bound": 1, "exact": 2, "auto": 1}              # bspgemm_stats.flow (auto runs upper-bound here)
KNOBS = list(itertools.product(("upper-bound", "exact", "auto"), (0, 1), (0, 1), (-1, 0, 1), (0, 1), (1, 3)))
MASKED_KNOBS = list(itertools.product((0, 1), (0, 1), (0, 1), (1, 3)))
# csrc/kernels.hpp: the class layout; the small-product path's limits and the model of which products take it: tests/gen.py
RANK_BIN, MID_BIN, DENSE_BIN = gen.RANK_BIN, gen.MID_BIN, gen.DENSE_BIN
row_products, expected_bins, small_expected = gen.row_products, gen.expected_bins, gen.small_expected


@pytest.fixture(scope="module")
def ctx():
    """one context for the whole file: its result cache carries buffers from shape to shape"""
    c = bspgemm.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- host-side model of the path ---------------
def padded_misreads(b_rp, b_ci):
    """{B row: the columns the heavy-row gather read for it} for the rows it read wrong from the padded copy of B.col_idx
    while it sized that array by B.nnz: under four entries it took scalar loads of the array's first three entries as if
    every quad began at 0 (csrc/dense_rows.hip gather_sweep).  Used to check that each shape would expose that read."""
    b_rp, b_ci = np.asarray(b_rp, np.int64), np.asarray(b_ci, np.int64)
    nnz, lens = int(b_rp[-1]), np.diff(b_rp)
    if nnz == 0 or nnz >= 4:
        return {}
    plen = (lens + 15) & ~15
    start = np.concatenate([[0], np.cumsum(plen)])
    pad = np.concatenate([np.concatenate([b_ci[b_rp[j]:b_rp[j + 1]], np.full(plen[j] - lens[j], b_ci[b_rp[j + 1] - 1])])
                          for j in range(lens.size) if lens[j] > 0])
    scalar = [pad[0], pad[1] if nnz > 1 else 0, pad[2] if nnz > 2 else 0, 0]
    out = {}
    for j, L in enumerate(lens):
        got = set()
        for q in range((int(L) + 3) // 4):
            qs = start[j] + 4 * q
            b = max(qs if qs < start[j] + L - 4 else start[j] + L - 4, 0)
            got |= {int(scalar[k]) for k in range(4) if qs <= b + k < start[j] + L}
        if got != set(b_ci[b_rp[j]:b_rp[j + 1]].tolist()):
            out[j] = sorted(got)
    return out


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.array([c for r in rows for c in r], dtype=np.int32)


def _with_row(rp, ci, j, cols):
    rows = [list(ci[rp[i]:rp[i + 1]]) for i in range(rp.size - 1)]
    rows[j] = list(cols)
    return _csr(rows)


def check_misreads_change_c(s, heavy_only):
    """each B row the unfixed gather misreads must change C -- in the heavy rows (plain: only they take that gather) or
    anywhere (masked over more than 2^24 columns: every row does) -- or the shape would not expose it"""
    mis = padded_misreads(s["b_rp"], s["b_ci"])
    rows = np.flatnonzero(row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, s["a_rp"].size - 1) > 2048) if heavy_only else None
    for j, got in mis.items():
        brp, bci = _with_row(s["b_rp"], s["b_ci"], j, got)
        if "f_rp" in s:
            want, wrong = (O.spgemm_masked(s["a_rp"], s["a_ci"], x, y, s["ncols"], s["f_rp"], s["f_ci"])
                           for x, y in ((s["b_rp"], s["b_ci"]), (brp, bci)))
        else:
            want, wrong = (O.spgemm(s["a_rp"], s["a_ci"], x, y, s["ncols"]) for x, y in ((s["b_rp"], s["b_ci"]), (brp, bci)))
        if rows is not None:
            want, wrong = ([sorted(w[1][w[0][i]:w[0][i + 1]].tolist()) for i in rows] for w in (want, wrong))
            assert want != wrong, "B row %d read as %s would not change the heavy rows of C" % (j, got)
        else:
            assert not (np.array_equal(want[0], wrong[0]) and np.array_equal(want[1], wrong[1])), (j, got)
    return mis


# ---------------------------------------------------------------- shapes ------------------------------------
def _tiny_b_heavy(nnzb, b_cols):
    a_rp, a_ci, b_rp, b_ci = gen.tiny_b_heavy(nnzb, b_cols)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=11, heavy=nnzb >= 2)


W40 = 40_000_000


def _tiny_b_wide(nnzb):
    """B of 2 or 3 nonzeros over 40 M columns (four bitmap levels: the masked product takes the dense-row kernel for every
    row); A row 0 has 5000 repeated entries (a heavy row), the others 1-3; the mask admits every column of B, the 0 the
    scalar path fills in, and others"""
    b_rows = {2: [[W40 - 1], [], [3]], 3: [[W40 - 2], [4, W40 - 1], []]}[nnzb]
    b_rp, b_ci = _csr(b_rows)
    rng = np.random.default_rng(1100 + nnzb)
    a_rows = [list(rng.integers(0, 3, size=5000))] + [[2], [1], [0, 2], [1, 2, 0], [], [2, 2], [1]]
    a_rp, a_ci = _csr(a_rows)
    admit = sorted(set(b_ci.tolist()) | {0, 6, 20_000_000, W40 - 3})
    f_rp, f_ci = _csr([admit] * (a_rp.size - 1))
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=W40, heavy=True, f_rp=f_rp, f_ci=f_ci)


def _pad_boundaries():
    """B rows of 0, 1, 15, 16, 17, 31, 32, 33, 255, 256 and 700 entries (padded lengths 0, 16, 16, 16, 32, ...), unsorted,
    with duplicates; rectangular A (400 x 600) != B (600 x 20000)"""
    rng = np.random.default_rng(971)
    nb, ncols = 600, 20000
    lens = rng.integers(0, 40, size=nb)
    for r, L in enumerate((0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 700)):
        lens[r] = L
    lens[nb - 1] = 15
    b_rows = np.repeat(np.arange(nb), lens)
    b_cols = np.where(rng.random(b_rows.size) < 0.3, rng.integers(0, 64, size=b_rows.size), rng.integers(0, ncols, size=b_rows.size))
    b_rp, b_ci = gen._csr_from_pairs(b_rows, b_cols, nb, dedup=False, sort=False)
    a_rows = np.repeat(np.arange(400), rng.integers(0, 12, size=400))
    a_cols = rng.integers(0, nb, size=a_rows.size)
    a_cols[:33] = np.arange(33) % 11
    a_rp, a_ci = gen._csr_from_pairs(a_rows, a_cols, 400, dedup=False, sort=False)
    f_rows = np.repeat(np.arange(400), rng.integers(0, 200, size=400))
    f_cols = np.where(rng.random(f_rows.size) < 0.5, rng.integers(0, 64, size=f_rows.size), rng.integers(0, ncols, size=f_rows.size))
    f_rp, f_ci = gen._csr_from_pairs(f_rows, f_cols, 400)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols, interior=True, f_rp=f_rp, f_ci=f_ci)


def _class_boundaries():
    a_rp, a_ci, b_rp, b_ci = gen.class_boundary_rows(repeat=1, seed=1301)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=6000, need=list(range(1, 17)) + [MID_BIN, DENSE_BIN])


def _rank_700k():
    """rows of 2049, 4097, 6144 (rank class), 6145 (the small heavy shape) products; row 4 from 1-3-entry sources only
    (masked quads), row 5 from 5000 one-entry sources (more than 4096 quads: several tiles of the gather plan)"""
    a_rp, a_ci, b_rp, b_ci = gen.rank_rows(700_001, [2049, 4097, 6144, 6145, 3000, 5000], short_rows=(4,), ones_rows=(5,),
                                           seed=7001, counts=(6000, 1000, 100))
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=700_001, need=[RANK_BIN, MID_BIN])


def _validity():
    rp, ci, _, n = bspgemm.readCOO(os.path.join(GOLDEN, "validity_test.mtx"))
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, square=True, fits_small=True)


def _small_bails():
    """40 A-nonzeros (the host calls it small) but a row of 40 x 200 = 8000 products: the device bails"""
    rng = np.random.default_rng(1942)
    a_rp = np.array([0, 40, 41, 41], np.int32)
    a_ci = np.concatenate([np.arange(40), [3]]).astype(np.int32)
    b_rows = np.repeat(np.arange(50), 200)
    b_rp, b_ci = gen._csr_from_pairs(b_rows, rng.integers(0, 100_000, size=b_rows.size), 50)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=100_000, heavy=True)


def _empty_a_rows():
    b_rp, b_ci = gen.uniform_rect(50, 300, 4, seed=1401)
    return dict(a_rp=np.zeros(65, np.int32), a_ci=np.zeros(0, np.int32), b_rp=b_rp, b_ci=b_ci, ncols=300)


def _empty_b():
    a_rp, a_ci = gen.uniform_rect(80, 50, 5, seed=1402)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=np.zeros(51, np.int32), b_ci=np.zeros(0, np.int32), ncols=300)


def _empty_range():
    rp, ci, n = gen.uniform(500, 5, 1403)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, square=True, ranges=[(100, 100)])


def _empty_rows_both():
    """every third A row empty, every other B row empty, A entries on both kinds of B row"""
    rng = np.random.default_rng(1404)
    b_rows = [[] if j % 2 == 0 else list(rng.integers(0, 700, size=int(rng.integers(1, 21)))) for j in range(200)]
    a_rows = [[] if i % 3 == 0 else list(rng.integers(0, 200, size=int(rng.integers(1, 9)))) for i in range(300)]
    b_rp, b_ci = _csr(b_rows)
    a_rp, a_ci = _csr(a_rows)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=700)


def _five_levels():
    ncols = 300_000_000
    a_rp, a_ci = gen.uniform_rect(300, 400, 5, seed=1501)
    rng = np.random.default_rng(1502)
    rows = np.repeat(np.arange(400), 20)
    cols = np.concatenate([rng.integers(0, ncols, size=4000), rng.integers(ncols - 3000, ncols, size=4000)])
    b_rp, b_ci = gen._csr_from_pairs(rows, cols, 400)
    return dict(a_rp=a_rp, a_ci=a_ci, b_rp=b_rp, b_ci=b_ci, ncols=ncols)


def _rmat_skewed():
    rp, ci, n = gen.rmat(13, 16, (0.57, 0.19, 0.19, 0.05), 1601)
    return dict(a_rp=rp, a_ci=ci, b_rp=rp, b_ci=ci, ncols=n, square=True, interior=True, f_rp=rp, f_ci=ci,
                need=list(range(1, 17)) + [MID_BIN])


SHAPES = {
    **{"tiny_b_heavy_nnz%d" % k: (lambda k=k: _tiny_b_heavy(k, (7, 0, 10, 3, 4))) for k in (1, 2, 3, 5)},
    **{"tiny_b_heavy_off0_nnz%d" % k: (lambda k=k: _tiny_b_heavy(k, (7, 3, 10, 4, 5))) for k in (1, 2, 3, 5)},
    "tiny_b_wide_nnz2": lambda: _tiny_b_wide(2),
    "tiny_b_wide_nnz3": lambda: _tiny_b_wide(3),
    "pad_boundaries": _pad_boundaries,
    "class_boundaries": _class_boundaries,
    "rank_700k": _rank_700k,
    "small_fits_validity": _validity,
    "small_bails_on_device": _small_bails,
    "empty_a_rows": _empty_a_rows,
    "empty_b": _empty_b,
    "empty_range": _empty_range,
    "empty_rows_next_to_empty_rows": _empty_rows_both,
    "five_levels_300M": _five_levels,
    "rmat13_skewed": _rmat_skewed,
}
MASKED_SHAPES = ["tiny_b_wide_nnz2", "tiny_b_wide_nnz3", "pad_boundaries", "rmat13_skewed"]


def _ranges(s, k):
    """the row ranges of combination k: the whole A, and for `interior` shapes an interior range whose size varies with k"""
    R = s["a_rp"].size - 1
    if "ranges" in s:
        return s["ranges"]
    if not s.get("interior"):
        return [(0, R)]
    return [(0, R), (7 + (13 * k) % (R // 4), R - (29 * k) % (R // 3))]


class Operands:
    """A and B on the device, fresh for every combination: uploaded again on even k, invalidated on odd k"""

    def __init__(self, ctx, s):
        self.ctx, self.s, self.A, self.B = ctx, s, None, None

    def fresh(self, k):
        s = self.s
        if self.A is None or k % 2 == 0:
            self.free()
            self.A = self.ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
            self.B = self.A if s.get("square") else self.ctx.upload(s["b_rp"], s["b_ci"], s["ncols"])
        else:
            self.A.invalidate()
            if self.B is not self.A:
                self.B.invalidate()
        assert self.B.uses_padded_rows == -1 and self.B.uses_blocked_table == -1

    def free(self):
        for h in (self.A, self.B):
            if h is not None:
                h.free()
        self.A = self.B = None


def _expect(s, want, r0, r1):
    return want[0][r0:r1 + 1] - want[0][r0], want[1][want[0][r0]:want[0][r1]]


def _compare(C, s, want, r0, r1):
    crp, cci = C.download()
    erp, eci = _expect(s, want, r0, r1)
    if crp.shape != erp.shape or not np.array_equal(crp, erp):
        return "row_ptr differs (first rows %s)" % (np.flatnonzero(crp != erp)[:5] if crp.shape == erp.shape else "shape")
    if not np.array_equal(cci, eci):
        return "col_idx differs (first at %s)" % np.flatnonzero(cci != eci)[:5] if cci.shape == eci.shape else "nnz %d != %d" % (cci.size, eci.size)
    return None


@pytest.mark.parametrize("shape", list(SHAPES))
def test_knob_matrix(ctx, shape):
    s = SHAPES[shape]()
    s["a_rp"], s["b_rp"] = np.asarray(s["a_rp"], np.int32), np.asarray(s["b_rp"], np.int32)
    nnz_a, nnz_b, b_rows = int(s["a_rp"][-1]), int(s["b_rp"][-1]), s["b_rp"].size - 1
    if shape.startswith("tiny_b"):
        mis = check_misreads_change_c(s, heavy_only=True)
        assert bool(mis) == (shape in ("tiny_b_heavy_nnz3", "tiny_b_heavy_off0_nnz2", "tiny_b_heavy_off0_nnz3")
                             or shape.startswith("tiny_b_wide")), (shape, mis)
    want = O.spgemm(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], s["ncols"])
    R_all = s["a_rp"].size - 1
    F_all = row_products(s["a_rp"], s["a_ci"], s["b_rp"], 0, R_all)
    if s.get("heavy"):
        assert F_all.max() > 2048
    if "need" in s:
        bins = expected_bins(F_all, s["ncols"])
        assert all(bins[b] > 0 for b in s["need"]), bins
    ops = Operands(ctx, s)
    failures, runs = [], 0
    try:
        for k, (flow, pad, blk, small, chk, cs) in enumerate(KNOBS):
            ctx.set_flow(flow)
            for name, v in (("padded_rows", pad), ("blocked_extents", blk), ("small_path", small), ("check", chk), ("class_streams", cs)):
                ctx.set_option(name, v)
            ops.fresh(k)
            for n_run, (r0, r1) in enumerate(_ranges(s, k)):
                tag = "flow=%s padded_rows=%d blocked_extents=%d small_path=%d check=%d class_streams=%d rows=[%d,%d)" % (
                    flow, pad, blk, small, chk, cs, r0, r1)
                R = r1 - r0
                F = F_all[r0:r1]
                try:
                    C = ctx.multiply(ops.A, ops.B, r0, r1)
                except bspgemm.BspgemmError as e:
                    failures.append("%s: %s" % (tag, e))
                    if e.status == 3:                   # BSPGEMM_ERR_HIP: nothing more on this device
                        raise
                    continue
                runs += 1
                st = ctx.stats()
                bad = _compare(C, s, want, r0, r1)
                C.free()
                if bad:
                    failures.append("%s: %s" % (tag, bad))
                if R == 0:
                    continue
                got = {k2: st[k2] for k2 in ("small_path", "flow", "prepass_kernel", "padded_rows", "checked", "class_streams")}
                if small_expected(flow, small, R, nnz_a, nnz_b, b_rows, F):
                    exp = dict(small_path=1, prepass_kernel=2, padded_rows=0, checked=0)
                    flags = (-1, -1)                        # the small path derives no table from B
                else:
                    exp = dict(small_path=0, flow=FLOW_ID[flow], prepass_kernel=blk, padded_rows=int(pad == 1 and nnz_b > 0),
                               checked=chk, class_streams=cs)
                    flags = (exp["padded_rows"], blk)
                    if st["rows_per_bin"] != expected_bins(F, s["ncols"]):
                        failures.append("%s: rows per class %s, expected %s" % (tag, st["rows_per_bin"], expected_bins(F, s["ncols"])))
                diff = {k2: (got[k2], v) for k2, v in exp.items() if got[k2] != v}
                if diff:
                    failures.append("%s: path %s (stats, expected)" % (tag, diff))
                if n_run == 0 and (ops.B.uses_padded_rows, ops.B.uses_blocked_table) != flags:
                    failures.append("%s: B.uses_padded_rows, B.uses_blocked_table = %s, expected %s" % (
                        tag, (ops.B.uses_padded_rows, ops.B.uses_blocked_table), flags))
    finally:
        ops.free()
    assert runs > 0
    assert not failures, "%s: %d of %d runs wrong:\n  %s" % (shape, len(failures), runs, "\n  ".join(failures))


@pytest.mark.parametrize("shape", ["masked_" + m for m in MASKED_SHAPES])
def test_masked_knob_matrix(ctx, shape):
    """C = F .* (A*B) has one flow: padded_rows x blocked_extents x check x class_streams against spgemm_masked"""
    s = SHAPES[shape[len("masked_"):]]()
    s["a_rp"], s["b_rp"] = np.asarray(s["a_rp"], np.int32), np.asarray(s["b_rp"], np.int32)
    if shape.startswith("masked_tiny_b"):
        assert check_misreads_change_c(s, heavy_only=False)
    want = O.spgemm_masked(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], s["ncols"], s["f_rp"], s["f_ci"])
    nnz_b = int(s["b_rp"][-1])
    ctx.set_flow("auto")
    ctx.set_option("small_path", -1)
    Fm = ctx.upload(s["f_rp"], s["f_ci"], s["ncols"])
    ops = Operands(ctx, s)
    failures, runs = [], 0
    try:
        for k, (pad, blk, chk, cs) in enumerate(MASKED_KNOBS):
            for name, v in (("padded_rows", pad), ("blocked_extents", blk), ("check", chk), ("class_streams", cs)):
                ctx.set_option(name, v)
            ops.fresh(k)
            for n_run, (r0, r1) in enumerate(_ranges(s, k)):
                tag = "padded_rows=%d blocked_extents=%d check=%d class_streams=%d rows=[%d,%d)" % (pad, blk, chk, cs, r0, r1)
                C = ctx.multiply_masked(ops.A, ops.B, Fm, r0, r1)
                runs += 1
                st = ctx.stats()
                bad = _compare(C, s, want, r0, r1)
                C.free()
                if bad:
                    failures.append("%s: %s" % (tag, bad))
                exp = dict(small_path=0, flow=1, prepass_kernel=blk, padded_rows=int(pad == 1 and nnz_b > 0), checked=chk,
                           class_streams=cs)
                diff = {k2: (st[k2], v) for k2, v in exp.items() if st[k2] != v}
                if diff:
                    failures.append("%s: path %s (stats, expected)" % (tag, diff))
                if n_run == 0 and (ops.B.uses_padded_rows, ops.B.uses_blocked_table) != (exp["padded_rows"], blk):
                    failures.append("%s: B flags %s" % (tag, (ops.B.uses_padded_rows, ops.B.uses_blocked_table)))
    finally:
        ops.free()
        Fm.free()
    assert not failures, "%s: %d of %d runs wrong:\n  %s" % (shape, len(failures), runs, "\n  ".join(failures))


# ---------------------------------------------------------------- a caller's stream ---------------------------
def test_callers_stream_orders_every_launch():
    """bspgemm_set_stream: the library's work -- its derived tables, the prepass, the class launches it forks over two more
    streams (CLASS_STREAMS = 3) and joins -- must queue behind what the caller put on that stream before.  The operands'
    col_idx arrays are written there, behind a long sleep, and multiplied with no host synchronisation in between: a launch
    out of order reads the zeros they held before (row_ptr is written and synchronised first: a half-written row_ptr would
    not be a CSR).  Both flows, with and without the padded copy (built from col_idx), and the masked product whose mask is
    written the same way; then back on the context's own stream (set_stream(None)) for the same product."""
    import torch
    dev = torch.device("cuda", 0)
    rp, ci, n = gen.rmat(12, 16, (0.57, 0.19, 0.19, 0.05), 1701)          # skewed: wave classes and heavy rows
    want = O.spgemm(rp, ci, rp, ci, n)
    want_m = O.spgemm_masked(rp, ci, rp, ci, n, rp, ci)
    nnz = int(rp[-1])
    h_ci = torch.from_numpy(np.asarray(ci, np.int32)).pin_memory()
    keep = [h_ci]
    ctx = bspgemm.Context(0)
    stream = torch.cuda.Stream(device=dev)
    failures = []
    try:
        ctx.set_stream(stream.cuda_stream)
        ctx.set_option("class_streams", 3)
        ctx.set_option("small_path", 0)

        def late_operand():
            d_rp = torch.from_numpy(np.asarray(rp, np.int32)).to(dev)
            d_ci = torch.zeros(nnz, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            keep.extend((d_rp, d_ci))
            with torch.cuda.stream(stream):
                torch.cuda._sleep(100_000_000)
                d_ci.copy_(h_ci, non_blocking=True)
            return ctx.wrap_device(n, n, nnz, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci))

        A = None
        for flow, pad in itertools.product(("upper-bound", "exact"), (0, 1)):
            ctx.set_flow(flow)
            ctx.set_option("padded_rows", pad)
            A = late_operand()
            C = ctx.multiply(A, A)
            st = ctx.stats()
            got = C.download()
            C.free()
            if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                failures.append("%s flow, padded_rows=%d: not the product of the operand written on the caller's stream" % (flow, pad))
            if (st["flow"], st["class_streams"], st["padded_rows"], st["small_path"]) != (FLOW_ID[flow], 3, pad, 0):
                failures.append("%s flow, padded_rows=%d: stats %s" % (flow, pad, st))
            A.free()
        ctx.set_option("padded_rows", 1)
        A, M = late_operand(), late_operand()
        C = ctx.multiply_masked(A, A, M)
        got = C.download()
        C.free()
        if not (np.array_equal(got[0], want_m[0]) and np.array_equal(got[1], want_m[1])):
            failures.append("masked: not the product of the operands written on the caller's stream")
        M.free()
        stream.synchronize()
        ctx.set_stream(None)
        C = ctx.multiply(A, A)
        got = C.download()
        C.free()
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            failures.append("back on the context's own stream: wrong product")
        A.free()
    finally:
        ctx.close()
        torch.cuda.synchronize()
    del keep
    assert not failures, "\n".join(failures)
