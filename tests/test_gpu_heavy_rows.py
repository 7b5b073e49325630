"""The heavy-row kernels (csrc/dense_rows.hip k_rank_rows, k_dense_rows, k_dense_rows_count over csrc/heavy_gather.hpp) at
their edges, on purpose rather than by chance.

Two families of products at four column counts (gen.HEAVY_COLS: 6000, 2^18 + 1, 2^20 + 1, 3 * 2^20 + 777; the readout family
also at 2^19 + 1, where the rank kernel without spans has two top words per thread):
  gather   rows of exact (sources, quads): every threshold of the tile's last step on both sides, plans kept and not kept by one
           source or one quad, batches without a non-empty source, sources on and across tile boundaries, a tile without a
           start, source lengths 1 .. 8, B row 0 of two entries, B's last row, unsorted B rows with repeats, rows whose upper
           windows receive products in lanes 1 to 3 only (gen.heavy_gather_case);
  readout  rows whose OUTPUT is prescribed per 256-word step of the window read-out -- none, one, exactly stage_cap,
           stage_cap + 1, a full step, direct steps with words of 1, 2, 3, 11, 12, 13, 63 and 64 outputs, the columns around every
           window boundary, the last column, empty windows -- and rank rows of 70 .. 6000 slots (gen.heavy_readout_case);
with a mask F and a D per case built from the product pattern (gen.heavy_masks).  gen.heavy_model derives on the host which
kernel takes every row and which cells it reaches there; test_heavy_rows_coverage asserts, without a GPU, that every kernel
reaches every reachable cell in some case.  On the GPU every case runs as the plain product (both flows; the gather cases
also over the padded copy of B), C = F .* (A*B), C = !F .* (A*B), C = D | (A*B) and the counting product, each compared bit
for bit with the CPU oracle and its launch (bspgemm_stats) with the model.
"""
import functools
import os
import time

import numpy as np
import pytest

import gen

FAMILIES = {"gather": gen.heavy_gather_case, "readout": gen.heavy_readout_case}
RANK_WIDE = (1 << 19) + 1                       # one rank span of two top words per thread (topw 1024), kept rows held: only in (2^19, 2^20]
CASES = [(fam, cols) for fam in FAMILIES for cols in gen.HEAVY_COLS] + [("readout", RANK_WIDE)]
INTERIOR = ("gather", (1 << 20) + 1)            # the case that also runs over a row range that starts and ends inside the heavy rows
MAX_TOTAL = 20_000_000                          # products of all the cases together (19.3 M; tests/test_gpu_wave_rows.py spends 450 M)
KERNELS = ("rank", "rank spans", "win512", "win1024", "keep", "count")

# ---- the cells every kernel must reach (strings of gen.heavy_model) ---------------------------------------------------------------
GATHER = (["g:left=" + x for x in gen.HEAVY_LEFTS] + ["g:nu=%d/4" % k for k in (1, 2, 3, 4)] + ["g:len%d" % k for k in range(1, 9)]
          + ["g:plan kept", "g:plan not kept", "g:plan kept and used", "g:T sources, QB == tile", "g:T+1 sources", "g:QB == tile+1",
             "g:empty batch first", "g:empty batch middle", "g:empty batch last", "g:several batches", "g:several tiles",
             "g:start on quad 0 of a later tile", "g:start on the last quad of a tile", "g:source crosses a tile boundary",
             "g:tile without a start", "g:B row 0 of 1-3 entries", "g:quad clamped to 0", "g:B's last row", "g:quad ends at nnzB",
             "g:words not ascending", "g:equal words apart"])
READOUT = (["r:direct pop %d" % k for k in gen.HEAVY_POPS]
           + ["r:column %s a boundary %s" % (w, x) for w in ("below", "at", "above") for x in ("set", "clear")]
           + ["r:empty window", "r:several windows with outputs", "r:idle waves", "r:step skipped", "r:step staged", "r:step direct",
              "r:outputs == 1", "r:outputs == stage_cap", "r:outputs == stage_cap+1", "r:full step", "r:tail staged", "r:tail direct",
              "r:tail skipped", "r:tail outputs == stage_cap", "r:tail outputs == stage_cap+1", "r:last column",
              "r:last window of one column"])
RANK = ["k:spt %d" % k for k in range(1, 13)] + ["k:skip > 0", "k:full top word", "k:full slot"]
MASK = ["f:column at or beyond cols", "f:column in a window without a product", "f:column in a window with products",
        "f:column that is a product"]
COUNT = ["c:window skipped", "c:window narrowed", "c:first sweep in a later window", "c:swept window with products",
         "c:swept window without a product", "f:column at or beyond cols"]
# What a kernel cannot reach, and the bound that rules it out.  A rank row has at most 6144 products, so a batch of at most
# 512 sources has at most (6144 + 3 * 512) / 4 = 1920 quads:
RANK_OUT = {"g:left=step",                                  # 2048 quads in a batch: less than a full step
            "g:T sources, QB == tile", "g:QB == tile+1", "g:several tiles", "g:start on quad 0 of a later tile",
            "g:start on the last quad of a tile", "g:source crosses a tile boundary", "g:tile without a start"}   # 4096 quads: less than a tile
UNREACHABLE = {
    # one span: a kept plan has at most 1920 quads, one step, so the row is held and never reads its plan again; the span has
    # products, so no column of F or D lies in a span without one
    "rank": RANK_OUT | {"g:plan kept and used", "f:column in a window without a product"},
    "rank spans": RANK_OUT | {"g:held"},                      # held: only without spans (k_rank_rows: if (!kSpans) held = ...)
    # the 512-thread window has a tail step only below 2^18 columns, where the window's words are no multiple of 256: of the
    # column counts only 6000, whose one window is ONE step, so no step beside the tail can hold the row's outputs
    "win512": {"r:tail skipped"},
    "win1024": set(), "keep": set(), "count": set(),
}


def required(kernel, mode):
    """the cells `kernel` must reach under `mode`"""
    if kernel == "count":
        return set(GATHER + COUNT)
    want = set(GATHER)
    if kernel.startswith("rank"):
        want |= set(RANK) | {"g:not held"}
        # (one or two top words per thread: without spans 2^18 + 1 and 2^19 + 1 columns; with spans a span is 2^20 columns: always two)
        want |= {"g:held", "k:topw 512", "k:topw 1024"} if kernel == "rank" else {"k:topw 1024", "k:span without a product", "k:last span of one column"}
        if kernel == "rank spans" and mode == "insert":
            want.add("k:span without a product, D reaches it")
    else:
        want |= set(READOUT)
    if mode != "none":
        want |= set(MASK)
    if mode == "drop" and kernel in ("win512", "win1024"):
        want.add("f:dropped product in a window fed by lanes 1-3 only")
    return want - UNREACHABLE[kernel]


@functools.lru_cache(maxsize=None)
def _case(fam, cols):
    return gen.heavy_masks(FAMILIES[fam](cols, 6100 + 10 * list(FAMILIES).index(fam) + (gen.HEAVY_COLS + (RANK_WIDE,)).index(cols)), seed=6200 + cols % 1000)


def _operand(s, mode):
    return None if mode == "none" else (s["d_rp"], s["d_ci"]) if mode == "insert" else (s["f_rp"], s["f_ci"])


def _model(s, mode, r0=0, r1=None):
    r1 = s["a_rp"].size - 1 if r1 is None else r1
    return gen.heavy_model(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], s["ncols"], mode, r0, r1, _operand(s, mode))


def _interior(s):
    """a range that starts and ends inside the heavy rows (the light rows lie in the middle)"""
    R = s["a_rp"].size - 1
    return 3, R - 2


# ---------------------------------------------------------------- without a GPU -----------------------------------
def test_heavy_rows_coverage():
    """every kernel reaches every reachable cell in some case, under every mode that runs it; nothing is reached that is
    not required (listed as unreachable or in no list); every case has two rows or more in the last class and heavy rows on both sides of the interior range; the
    product budget"""
    t0 = time.time()
    reached, total = {}, 0
    for fam, cols in CASES:
        s = _case(fam, cols)
        for mode in gen.HEAVY_MODES:
            m = _model(s, mode)
            for r in m["rows"].values():
                reached.setdefault((r["kernel"], mode), set()).update(r["cells"])
            if mode == "none":
                total += int(m["F"].sum())
                assert int((m["bins"] == gen.DENSE_BIN).sum()) >= 2, (fam, cols, np.bincount(m["bins"]))
                assert s["b_rp"][1] - s["b_rp"][0] == 2 and (np.diff(s["b_rp"]) == 0).any()
        if (fam, cols) == INTERIOR:
            r0, r1 = _interior(s)
            heavy = _model(s, "none")["bins"] > 16
            assert heavy[:r0].any() and heavy[r0] and heavy[r1 - 1] and heavy[r1:].any()
    bad = []
    for kernel in KERNELS:
        modes = ("keep",) if kernel == "keep" else ("count",) if kernel == "count" else ("none", "drop", "insert")
        for mode in modes:
            got = reached.get((kernel, mode), set())
            for c in sorted(required(kernel, mode) - got):
                bad.append("%s, mode %s: never reaches %s" % (kernel, mode, c))
            for c in sorted(got - required(kernel, mode)):      # (so the lists cannot fall behind the model)
                bad.append("%s, mode %s: reaches %s, which is %s" % (kernel, mode, c, "listed as unreachable" if c in UNREACHABLE[kernel] else "not required"))
    assert not bad, "\n  " + "\n  ".join(bad)
    assert total <= MAX_TOTAL, total
    print("heavy rows: %d products in %d cases, %.1f s" % (total, len(CASES), time.time() - t0))


# ---------------------------------------------------------------- on the GPU ---------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import bspgemm
    c = bspgemm.Context(0)
    yield c
    for k, v in (("small_path", -1), ("padded_rows", -1)):
        c.set_option(k, v)
    c.set_flow("auto")
    c.close()


@functools.lru_cache(maxsize=None)
def _product(fam, cols):
    """the oracle's A * B of a case, computed once and shared by the modes: (row_ptr, col_idx), read-only"""
    from oracle import oracle as O
    s = _case(fam, cols)
    R = s["a_rp"].size - 1
    threads = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
    rp, ci = O.spgemm_omp(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], cols, -(-R // threads), threads)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci


def _keys(rp, ci, r0):
    rows = np.repeat(np.arange(r0, r0 + rp.size - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    return (rows << 32) | np.asarray(ci, np.int64)


def _expected(want, mode, f, cols, r0, r1):
    """rows [r0, r1) of the oracle's product under `mode`: the set difference with F (drop), the union with D's columns
    below `cols` (insert), the intersection with F (keep); (row_ptr int64 slice-local, col_idx int32)"""
    rp, ci = want
    wk = _keys(rp[r0:r1 + 1], ci[rp[r0]:rp[r1]], r0)
    if mode != "none":
        f_rp = np.asarray(f[0], np.int64)
        fc = np.asarray(f[1][f_rp[r0]:f_rp[r1]], np.int64)
        fk = _keys(f_rp[r0:r1 + 1], fc, r0)
        if mode == "insert":
            wk = np.union1d(wk, fk[(fc >= 0) & (fc < cols)])
        else:
            inside = np.isin(wk, fk)
            wk = wk[inside if mode == "keep" else ~inside]
    counts = np.bincount((wk >> 32) - r0, minlength=r1 - r0)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), (wk & 0xFFFFFFFF).astype(np.int32)


FLOW_ID = {"upper-bound": 1, "exact": 2}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", gen.HEAVY_MODES)
@pytest.mark.parametrize("fam,cols", CASES, ids=["%s-cols%d" % c for c in CASES])
def test_heavy_rows(ctx, fam, cols, mode):
    import bspgemm
    s = _case(fam, cols)
    want = _product(fam, cols)
    R = s["a_rp"].size - 1
    f = _operand(s, mode)
    ranges = [(0, R)] + ([_interior(s)] if (fam, cols) == INTERIOR else [])
    flows = ("upper-bound", "exact") if mode == "none" else ("upper-bound",)
    pads = (0, 1) if fam == "gather" else (0,)
    ctx.set_option("small_path", 0)
    A = ctx.upload(s["a_rp"], s["a_ci"], s["b_rp"].size - 1)
    B = ctx.upload(s["b_rp"], s["b_ci"], cols)
    # (D may not be wider than B: its columns at or beyond B.cols are stored all the same; a mask may be of any width)
    Fm = ctx.upload(f[0], f[1], cols if mode == "insert" else gen.INT_MAX) if f is not None else None
    failures = []
    try:
        for r0, r1 in ranges:
            m = _model(s, mode, r0, r1)
            assert m["rows"], "no heavy row"
            if mode == "count":
                from test_gpu_masked_count import count_ref
                exp = count_ref(s["a_rp"], s["a_ci"], s["b_rp"], s["b_ci"], f[0], f[1], cols, r0, r1)
                keep = _expected(want, "keep", f, cols, r0, r1)
                assert np.array_equal(exp[0], keep[0]) and np.array_equal(exp[1], keep[1]), "count_ref and the oracle disagree"
            else:
                exp = _expected(want, mode, f, cols, r0, r1)
            exp_stats = dict(small_path=0, bin_cap=gen.expected_bin_caps(cols, rank_cap=0 if mode in ("keep", "count") else None),
                             rows_per_bin=np.bincount(m["bins"], minlength=gen.NUM_BINS).tolist())
            for pad in pads:
                ctx.set_option("padded_rows", pad)
                B.invalidate()                              # (the tables derived from B follow the option at B's next use)
                for flow in flows:
                    ctx.set_flow(flow)
                    t0 = time.time()
                    try:
                        if mode == "none":
                            C = ctx.multiply(A, B, r0, r1)
                        elif mode == "insert":
                            C = ctx.multiply_accumulate(A, B, Fm, r0, r1)
                        elif mode == "count":
                            C = ctx.multiply_masked_count(A, B, Fm, r0, r1)
                        else:
                            C = ctx.multiply_masked(A, B, Fm, r0, r1, complement=mode == "drop")
                    except bspgemm.BspgemmError as e:
                        if e.status == 3:                   # BSPGEMM_ERR_HIP: nothing more on this device
                            pytest.exit("%s, %d columns, mode %s, %s flow, padded_rows=%d: %s" % (fam, cols, mode, flow, pad, e), 3)
                        raise
                    st = ctx.stats()
                    crp, cci = C.download()
                    vals = C.download_values() if mode == "count" else None
                    C.free()
                    tag = "%s flow, padded_rows=%d, rows [%d, %d)" % (flow, pad, r0, r1)
                    print("%s %s %d columns, %s: %.3f s, nnz(C) %d" % (mode, fam, cols, tag, time.time() - t0, cci.size))
                    if not np.array_equal(crp, exp[0]):
                        bad = (np.flatnonzero(np.diff(crp) != np.diff(exp[0]))[:5] + r0) if crp.shape == exp[0].shape else "shape"
                        names = [s["names"][i] for i in bad] if not isinstance(bad, str) else ""
                        failures.append("%s: row_ptr differs (first rows %s: %s)" % (tag, bad, names))
                    elif not np.array_equal(cci, exp[1]):
                        at = np.flatnonzero(cci != exp[1])[:5]
                        rows = np.searchsorted(exp[0], at, side="right") - 1 + r0
                        failures.append("%s: col_idx differs (first at %s, rows %s: %s)" % (tag, at, rows, [s["names"][i] for i in rows]))
                    elif vals is not None and not np.array_equal(vals, exp[2]):
                        at = np.flatnonzero(vals != exp[2])[:5]
                        failures.append("%s: counts differ (first at %s: %s, expected %s)" % (tag, at, vals[at], exp[2][at]))
                    got = {k: st[k] for k in ("flow", "padded_rows", *exp_stats)}
                    e = dict(flow=FLOW_ID[flow], padded_rows=pad, **exp_stats)
                    if got != e:
                        failures.append("%s: stats %s, expected %s" % (tag, got, e))
    finally:
        for x in (A, B, Fm):
            if x is not None:
                x.free()
    assert not failures, "%s, %d columns, mode %s:\n  %s" % (fam, cols, mode, "\n  ".join(failures))
