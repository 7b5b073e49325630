#!/usr/bin/env python3
"""What the device-resident fixed-point PageRank (bspgemm_pagerank) costs on an MI355X, in whole and in parts, beside the
only way to get the ranks without it: download the operand and run a float64 power iteration on the host.
    python tools/pagerank_time.py [--graphs rmat22 skew18 uniform20] [--iterations 20] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls, which end synchronised and with the ranks on the host (16 n bytes cross the link).

Graphs: rmatS = the benchmark's R-MAT (0.30, 0.25, 0.25), seed 1, scale S, edge factor 16; skewS = the Graph500-skew R-MAT
(0.57, 0.19, 0.19); uniformS = 2^S vertices with 16 entries per row.  Per graph, --iterations iterations, tolerance 0:
    variants  PULL with AT given, PULL with AT NULL (the call transposes), PUSH: the whole call, ms per iteration from the
              difference to the same call with max_iter 0 (which pays the checks, the transpose, the lists and the read-out),
              and the effective bytes per second of an iteration against the bytes it must move: 4 nnz for the column indices
              + 8 nnz for the gathered (PULL) or added (PUSH) 64-bit words + 36 n for row_ptr, r, c_in, c_out and the lists
    classes   PULL with AT given under BSPGEMM_OPT_PR_MIN_CLASS 0 .. 3, with the vertices per class
    parts     PULL (AT given, and AT NULL) and PUSH on a second context created under BSPGEMM_PR_TIMING, which synchronises
              behind every class's launch and prints its own host-clock sums by stage and class
    baseline  A.download() + a scipy float64 power iteration on the host (the transposed scipy CSR built once, then an
              SpMV per iteration), once
--check compares the device's ranks with the numpy model of the definition (graphs of up to --numpy-max entries) and the
variants with each other.  No threshold: the numbers are the result."""
import argparse
import sys
import time

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import show, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm
import pagerank_ref as P


def generate(name):
    kind, scale = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    if kind == "rmat":
        return "R-MAT scale %d, edge factor 16, (0.30, 0.25, 0.25), seed 1" % scale, bspgemm.gen_rmat(scale, 16, (0.30, 0.25, 0.25), seed=1)
    if kind == "skew":
        return "Graph500-skew R-MAT scale %d, edge factor 16, (0.57, 0.19, 0.19), seed 1" % scale, \
            bspgemm.gen_rmat(scale, 16, (0.57, 0.19, 0.19), seed=1)
    assert kind == "uniform", name
    return "uniform n = 2^%d, 16 entries per row, seed 1" % scale, bspgemm.gen_uniform(1 << scale, 16, seed=1)


def host_iteration(rp, ci, n, damping, iterations):
    """the float64 power iteration of tests/pagerank_ref.py on a canonical CSR as downloaded, without its np.unique"""
    from scipy.sparse import csr_matrix
    d = P.constants(n, damping)[1] / 4294967296.0
    outdeg = np.diff(rp).astype(np.float64)
    dangling = outdeg == 0
    M = csr_matrix((np.ones(ci.size), ci, rp), shape=(n, n)).T.tocsr()
    r = np.full(n, 1.0 / n)
    for _ in range(iterations):
        c = np.where(dangling, 0.0, r / np.where(dangling, 1.0, outdeg))
        r = (1.0 - d) / n + d * (M @ c + r[dangling].sum() / n)
    return r


def measure(ctx, ctx_timed, title, rp, ci, n, args):
    K = args.iterations
    A = ctx.upload(rp, ci, n)
    AT = ctx.transpose(A)
    At = ctx_timed.upload(rp, ci, n)
    ATt = ctx_timed.transpose(At)
    nnz = A.nnz
    must = 12 * nnz + 36 * n
    print("%s: n = %d, nnz = %d, %d iterations; an iteration must move %.1f MB" % (title, n, nnz, K, must / 1e6), flush=True)
    show("    transpose alone", wall_ms(ctx, lambda: ctx.transpose(A).free(), args.reps))
    ok, ranks, whole = True, {}, {}
    for what, at, method in (("PULL, AT given", AT, bspgemm.PR_PULL), ("PULL, AT NULL", None, bspgemm.PR_PULL),
                             ("PUSH", None, bspgemm.PR_PUSH)):
        ms = show("    %s, %d iterations (whole call)" % (what, K), wall_ms(ctx, lambda: (ctx.pagerank(A, at, method, 0.85, K), None)[1], args.reps))
        ms0 = show("    %s, 0 iterations (checks, transpose, lists, read-out)" % what,
                   wall_ms(ctx, lambda: (ctx.pagerank(A, at, method, 0.85, 0), None)[1], args.reps))
        per = (ms - ms0) / K
        print("      per iteration %.3f ms: %.0f GB/s against the %.1f MB" % (per, must / per / 1e6 if per > 0 else 0, must / 1e6),
              flush=True)
        whole[what] = ms
        ranks[what] = ctx.pagerank(A, at, method, 0.85, K)
        info = ranks[what][2]
        print("      dangling %d, delta %d, mass %d, classes %s" % (info["dangling"], info["delta"], info["mass"],
                                                                     info["class_vertices"]), flush=True)
    for min_class in (0, 1, 2, 3):
        ctx.set_option("pr_min_class", min_class)
        show("    PULL, AT given, PR_MIN_CLASS %d" % min_class, wall_ms(ctx, lambda: (ctx.pagerank(A, AT, bspgemm.PR_PULL, 0.85, K), None)[1], args.reps))
        got = ctx.pagerank(A, AT, bspgemm.PR_PULL, 0.85, K)
        print("      classes %s" % got[2]["class_vertices"], flush=True)
        if args.check:
            same = np.array_equal(got[0], ranks["PULL, AT given"][0])
            ok &= same
            print("      check against PR_MIN_CLASS 0: %s" % ("equal" if same else "DIFFERENT"), flush=True)
    ctx.set_option("pr_min_class", 0)
    for what, at, method in (("PULL, AT given", ATt, bspgemm.PR_PULL), ("PULL, AT NULL", None, bspgemm.PR_PULL),
                             ("PUSH", None, bspgemm.PR_PUSH)):
        stderr_of(lambda: ctx_timed.pagerank(At, at, method, 0.85, K))   # warm-up: workspaces
        for ln in stderr_of(lambda: ctx_timed.pagerank(At, at, method, 0.85, K)).splitlines():
            print("      parts, %s: %s" % (what, ln.strip()), flush=True)
    t = time.perf_counter()
    h_rp, h_ci = A.download()
    t_down = (time.perf_counter() - t) * 1e3
    f = host_iteration(h_rp, h_ci, n, 0.85, K)
    ms = (time.perf_counter() - t) * 1e3
    print("    baseline: download %.3f ms + scipy float64 power iteration on the host = %.3f ms (once)" % (t_down, ms), flush=True)
    for what in whole:
        print("      %-16s %10.3f ms: the baseline is %.1f x" % (what, whole[what], ms / whole[what]), flush=True)
    dev = float((np.abs(ranks["PULL, AT given"][1] - f) / f).max())
    print("      largest relative deviation of the fixed-point ranks from the host's float64 ones: %.3g" % dev, flush=True)
    if args.check:
        same = all(np.array_equal(r[0], ranks["PUSH"][0]) for r in ranks.values())
        ok &= same
        print("      check of the variants against each other: %s" % ("equal" if same else "DIFFERENT"), flush=True)
        if nnz <= args.numpy_max:
            exp = P.pagerank(h_rp, h_ci, n, 0.85, K)
            info = ranks["PUSH"][2]
            same = np.array_equal(ranks["PUSH"][0], exp["fixed"]) and (info["mass"], info["delta"]) == (exp["mass"], exp["delta"])
            ok &= same
            print("      check against the numpy model of the definition: %s" % ("equal" if same else "DIFFERENT"), flush=True)
    for h in (ATt, At, AT, A):
        h.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="*", default=["rmat22", "skew18", "uniform20"])
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=5_000_000, help="largest nnz for the numpy model of the definition")
    ap.add_argument("--check", action="store_true", help="compare the ranks with the numpy model and between the variants")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_PR_TIMING")
    ok = True
    for name in args.graphs:
        title, (rp, ci, n) = generate(name)
        ok &= measure(ctx, ctx_timed, title, rp, ci, n, args)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
