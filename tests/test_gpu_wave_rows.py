"""The one-wave kernel (csrc/wave_rows.inc, k_wave_rows) at its edges, on purpose rather than by chance.

It is compiled as 16 capacity classes x 10 (LEVELS, top-bitmap words per lane) shapes x {emit, count}.  One product per
shape, at or next to the column counts where launch_wave_rows switches instance (4096/4097, 131072/131073, 2^22/2^22+1,
2^24/2^24+1, 268435456 = 2^28 / 2^28+1), built by gen.wave_rows_case so that in every shape
  - every class holds more than 2048 rows: several rows per wave (rpw >= 2) and a partial last wave; across the shapes
    every class reaches its rpw cap (16, 8 from 16 chunks up);
  - every class mixes rows of every kind: more than 64 A-nonzeros (extents in several trips), empty B rows between
    others, sources on chunk boundaries, a chunk of 64 one-entry sources, a source over every chunk; sparse rows
    (every product alone in its 32-column slot), F - 1 slots, full slots, column 0 and the last column; repeats within
    and across chunks; 0, 12 and 13 ambiguous products of the count pass's hash filter, collisions of distinct columns
    and a column whose hash bit another column set first, repeated in a later chunk;
  - C's first 4096-output chunks and its size exercise the compaction's table path: one-shift chunks, a shift change
    inside a chunk, hole rows that end on a chunk boundary, a chunk over more than 4096 rows with holes in it, and
    nnz(C) = 0 mod 4096 or 1, 2, 3 mod 4.
Each product is compared bit for bit with the CPU oracle under the upper-bound and the exact flow, and the launch
(bspgemm_stats flow, bin_cap, rows_per_bin) is asserted against the host model (gen.wave_model), so that a shape that
landed in another instance fails.  test_wave_rows_coverage checks the same coverage without a GPU.
"""
import os

import numpy as np
import pytest

import gen

W = gen.WAVE_CHUNKS
BASE, INTERIOR_BASE, CAP16, CAP8 = 2051, 2701, 30725, 14341     # rows per class: rpw 2, 2, 16, 8; never a full last wave


def _plan(caps, base=BASE):
    return {b: (CAP8 if W[b - 1] >= 16 else CAP16) if b in caps else base for b in range(1, 17)}


# (columns, classes at their rpw cap, nnz(C) residue (modulus, value), interior row range)
SHAPES = [
    (4096, (11, 1), (4096, 0), False),          # L1, TWP 2
    (4097, (16, 2), (4, 1), False),             # L1, TWP 4
    (131072, (15, 3), (4, 2), False),           # L2, TWP 2
    (131073, (10, 4), (4, 3), True),            # L2, TWP 4
    (4194304, (14, 5), (4096, 0), False),       # L3, TWP 2
    (4194305, (9, 6), (4, 1), False),           # L3, TWP 4
    (16777216, (13, 7), (4, 2), False),         # L3, TWP 8 (the wide top)
    (16777217, (12, 8), (4, 3), False),         # L4, TWP 2
    (268435456, (), (4096, 0), False),          # L4, TWP 4: 2^28, the instance <4, *, 4>
    (268435457, (), (4, 3), False),             # L5, TWP 2
]
INSTANCES = [(1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (3, 4), (3, 8), (4, 2), (4, 4), (5, 2)]
STRIDE = 4                                       # rows whose products the host model analyses: i % STRIDE == 0
MAX_PRODUCTS, MAX_TOTAL = 60_000_000, 450_000_000


def _case(k):
    cols, caps, residue, interior = SHAPES[k]
    return gen.wave_rows_case(cols, _plan(caps, INTERIOR_BASE if interior else BASE), seed=4100 + k, residue=residue)


def _interior(s):
    R = s["a_rp"].size - 1
    return R // 16, R - R // 16


def wave_coverage(m):
    """what every shape must carry, from the host model: a list of what is missing"""
    bad = []
    cols, levels = m["cols"], m["levels"]
    if (m["bins"] > 16).any():
        bad.append("heavy rows")
    ana = m["analysed"]
    for b in range(1, 17):
        ch, c = W[b - 1], m["classes"][b]
        hb = gen.wave_hash_bits(ch)
        if c["rpw"] < 2 or c["last"] >= c["rpw"]:
            bad.append("class %d: %s (rpw >= 2 and a partial last wave wanted)" % (b, c))
        rows = m["bins"] == b
        ra = rows & ana
        F = m["F"]
        want = {"more than 64 A-nonzeros": m["multi_trip"], "an empty source between others": m["zero_between"],
                "a source over every chunk": m["spans_all"], "a chunk of 64 one-entry sources": m["ones_chunk"],
                "a column three times": m["dup3"], "a repeat within a chunk": m["repeat_within"],
                "column 0": m["col0"], "the last column": m["col_last"], "a full 32-column slot": m["full_slot"],
                "no ambiguous product": m["ambiguous"] == 0, "12 ambiguous products": m["ambiguous"] == gen.MAX_AMBIGUOUS,
                "13 ambiguous products": m["ambiguous"] == gen.MAX_AMBIGUOUS + 1}
        if ch >= 2:
            want["a source starting on a chunk boundary"] = m["starts_on_chunk"]
            want["a repeat across chunks"] = m["repeat_across"]
        if levels >= 2:
            want["a sparse row (nslots0 == F)"] = m["nslots0"] == F
            want["a dense row"] = (m["nslots0"] != F) & ana
            want["F - 1 slots, no repeat"] = (m["nslots0"] == F - 1) & (m["nnz_row"] == F)
        if cols >> hb >= 2:                      # distinct columns can share a hash
            want["a collision of distinct columns"] = m["collision"]
            if ch >= 3:
                want["a repeat every copy of which is ambiguous, in a row the filter settles"] = (
                    m["late_repeat"] & (m["ambiguous"] <= gen.MAX_AMBIGUOUS))
        for what, flag in want.items():
            if not (flag & ra).any():
                bad.append("class %d (%d chunks): no row with %s" % (b, ch, what))
    return bad


def compact_model(rp, placed):
    """the compaction's table path (csrc/dense_rows.hip k_compact) over C.row_ptr `rp`, rows placed at prefix(placed):
    chunk k covers outputs [4096k, 4096k + 4096); rf holds its first output, rl the output ceil(o1 / 4096) * 4096 (the
    last output at the end, as chunk_row); shift(r) = placed prefix - row_ptr"""
    rp = np.asarray(rp, np.int64)
    nnz = int(rp[-1])
    shift = np.concatenate([[0], np.cumsum(placed)])[:-1] - rp[:-1]
    K = -(-nnz // gen.COMPACT_GRAN)
    o0 = gen.COMPACT_GRAN * np.arange(K, dtype=np.int64)
    o1 = np.minimum(o0 + gen.COMPACT_GRAN, nnz)

    def row_of(o):
        return np.searchsorted(rp, o, side="right") - 1

    rf = row_of(o0)
    rl = row_of(np.minimum(-(-o1 // gen.COMPACT_GRAN) * gen.COMPACT_GRAN, nnz - 1))
    moves = shift[row_of(o1 - 1)] != shift[rf]           # a row with outputs in the chunk has another shift than rf
    one = shift[rf] == shift[rl]
    searched = ~one & (rl - rf > gen.COMPACT_SPARSE_ROWS)
    n = np.diff(rp)
    hole = (np.asarray(placed) > n) & (n > 0)
    return {"one-shift chunks": int(one.sum()), "general chunks": int((~one & ~searched).sum()),
            "searched chunks": int(searched.sum()), "general chunks with a shift change": int((~one & ~searched & moves).sum()),
            "searched chunks with a shift change": int((searched & moves).sum()),
            "hole rows ending a chunk": int((hole & (rp[1:] % gen.COMPACT_GRAN == 0)).sum()),
            "hole rows whose last output starts a chunk": int((hole & ((rp[1:] - 1) % gen.COMPACT_GRAN == 0)).sum())}


def _check_launch_model(k, s, m):
    cols = SHAPES[k][0]
    assert (m["levels"], m["twp"]) == INSTANCES[k], (cols, m["levels"], m["twp"])
    bad = wave_coverage(m)
    assert not bad, "shape %d (%d columns):\n  %s" % (k, cols, "\n  ".join(bad))
    assert int(m["F"].sum()) <= MAX_PRODUCTS


# ---------------------------------------------------------------- without a GPU -----------------------------------
def test_wave_rows_coverage():
    """the generator still builds every cell: classes, rpw, waves, sources, ambiguous counts, per shape; every class at
    its rpw cap in some shape; the compaction patterns of the tail rows; the product budget"""
    at_cap, total = set(), 0
    for k in range(len(SHAPES)):
        s = _case(k)
        m = gen.wave_model(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], SHAPES[k][0], stride=STRIDE)
        _check_launch_model(k, s, m)
        total += int(m["F"].sum())
        at_cap |= {b for b, c in m["classes"].items() if c["rpw"] == (8 if W[b - 1] >= 16 else 16)}
        if SHAPES[k][3]:
            r0, r1 = _interior(s)
            mi = gen.wave_model(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], SHAPES[k][0], r0, r1, products=False)
            assert all(c["n"] > 2048 for c in mi["classes"].values()), mi["classes"]
        # the tail rows alone (their outputs are the first of C): |C_i| from the model
        t = s["tail"]
        mt = gen.wave_model(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], SHAPES[k][0], 0, t)
        cm = compact_model(np.concatenate([[0], np.cumsum(mt["nnz_row"])]), mt["F"])
        assert all(v > 0 for v in cm.values()), cm
    assert at_cap == set(range(1, 17)), sorted(set(range(1, 17)) - at_cap)
    assert total <= MAX_TOTAL, total


# ---------------------------------------------------------------- on the GPU ---------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import bspgemm
    c = bspgemm.Context(0)
    yield c
    c.close()


def _oracle(s, cols):
    from oracle import oracle as O
    R = s["a_rp"].size - 1
    threads = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")), 8 if cols > (1 << 24) else 16)   # a flag byte per column each
    return O.spgemm_omp(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols, -(-R // threads), threads)


FLOW_ID = {"upper-bound": 1, "exact": 2}


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["cols%d" % sh[0] for sh in SHAPES])
def test_wave_rows_shape(ctx, k):
    cols, _, (mod, res), interior = SHAPES[k]
    s = _case(k)
    m = gen.wave_model(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols, stride=STRIDE)
    _check_launch_model(k, s, m)
    want = _oracle(s, cols)
    assert int(want[0][-1]) == s["nnz_c"] and s["nnz_c"] % mod == res, (int(want[0][-1]), s["nnz_c"], mod, res)
    cm = compact_model(want[0], np.minimum(m["F"], cols))
    assert all(v > 0 for v in cm.values()), cm
    ranges = [(0, m["R"])]
    if interior:
        r0, r1 = _interior(s)
        mi = gen.wave_model(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols, r0, r1, products=False)
        assert all(c["n"] > 2048 for c in mi["classes"].values()), mi["classes"]
        ranges.append((r0, r1))
    ctx.set_option("small_path", 0)
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    failures = []
    try:
        for flow in ("upper-bound", "exact"):
            ctx.set_flow(flow)
            for r0, r1 in ranges:
                C = ctx.multiply(A, B, r0, r1)
                st = ctx.stats()
                crp, cci = C.download()
                C.free()
                erp = want[0][r0:r1 + 1] - want[0][r0]
                eci = want[1][want[0][r0]:want[0][r1]]
                tag = "%s flow, rows [%d, %d)" % (flow, r0, r1)
                if not np.array_equal(crp, erp):
                    bad = np.flatnonzero(crp != erp)[:5] if crp.shape == erp.shape else "shape"
                    failures.append("%s: row_ptr differs (first at %s)" % (tag, bad))
                elif not np.array_equal(cci, eci):
                    failures.append("%s: col_idx differs (first at %s)" % (tag, np.flatnonzero(cci != eci)[:5]))
                F = m["F"][r0:r1]
                got = (st["flow"], st["small_path"], st["bin_cap"], st["rows_per_bin"])
                exp = (FLOW_ID[flow], 0, gen.expected_bin_caps(cols), gen.expected_bins(F, cols))
                if got != exp:
                    failures.append("%s: (flow, small_path, bin_cap, rows_per_bin) = %s, expected %s" % (tag, got, exp))
    finally:
        A.free()
        B.free()
    assert not failures, "%d columns (LEVELS %d, TWP %d):\n  %s" % (cols, m["levels"], m["twp"], "\n  ".join(failures))
