#!/usr/bin/env python3
"""What the on-device submatrix extraction (bspgemm_matrix_extract, bspgemm_matrix_extract_rows_of) costs on an MI355X, beside
the ways to cut a piece out of a graph without it: two products with selector matrices, or download + scipy + upload.
    python tools/extract_time.py [--graphs rmat22 g500_18] [--reps 5] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum, median and maximum printed: the spread
of the baseline is what a difference has to be read against).  Times are wall times around whole calls that end
synchronised; freeing the results is outside.

Graphs: rmat<scale> is the benchmark's R-MAT (0.30, 0.25, 0.25), g500_<scale> the Graph500-skew R-MAT (0.57, 0.19, 0.19),
both edge factor 16, seed 1, symmetrized without the diagonal on the device (S).  Per graph:
    1  KEEP_SHAPE on the vertices of core number >= k, k half the degeneracy, the list read on the device (a diagonal
       selector from matrix_from_result_where, ri = rj = -1), beside D_k * S * D_k: two products and two matrix_from_result
       copies, what bspgemm_kcore runs for its answer
    2  a seeded random half of the vertices, ascending, relabelled (host lists), beside P_I * S * P_J^T from public calls and
       beside download + scipy S[I][:, J] + upload
    3  the degree-descending permutation (a column list that is not ascending: the sort classes), beside download + scipy +
       upload; triangle_count and local_clustering on S and on the relabelled graph
    then the stage split of the three on a second context created under BSPGEMM_EXTRACT_TIMING, and the EXTRACT_LANES sweep
--check verifies first that the routes give equal operands (always done for 1 and 2's product routes; --check adds scipy's).
No threshold: the numbers are the result."""
import argparse
import statistics
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import stderr_of, timed_context, wall_ms
import numpy as np
from scipy.sparse import csr_matrix
import bspgemm


def show(name, ms):
    print("    %-64s min %10.3f  median %10.3f  max %10.3f ms" % (name, min(ms), statistics.median(ms), max(ms)), flush=True)
    return statistics.median(ms)


def same_operand(ctx, X, Y):
    if (X.rows, X.cols, X.nnz) != (Y.rows, Y.cols, Y.nnz) or not ctx.matrix_equal(X, Y):
        return False
    return np.array_equal(X.download()[1], Y.download()[1])


def products(ctx, L, S, R, cols):
    """L * S * R through two products and two copies: (operand, the handles to free)"""
    r1 = ctx.multiply(L, S)
    m1 = ctx.matrix_from_result(r1, S.cols)
    r2 = ctx.multiply(m1, R)
    m2 = ctx.matrix_from_result(r2, cols)
    return m2, [r1, m1, r2]


def scipy_route(ctx, S, I, J):
    rp, ci = S.download()
    M = csr_matrix((np.ones(ci.size, np.int8), ci, rp), shape=(S.rows, S.cols))
    X = M[I][:, J]
    X.sort_indices()
    return ctx.upload(X.indptr.astype(np.int32), X.indices.astype(np.int32), X.shape[1])


def measure(ctx, ctx_timed, name, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    S = ctx.symmetrize(A, drop_diagonal=True)
    A.free()
    srp = S.download()[0]
    deg = np.diff(srp)
    print("%s: n = %d, nnz(S) = %d, longest row %d" % (name, n, S.nnz, int(deg.max())), flush=True)
    ok = True
    reps = args.reps
    big = S.nnz > args.scipy_max

    # ---- 1. the k-core's vertex set, KEEP_SHAPE, device list
    cores, top, _ = ctx.core_numbers(S)
    k = max(top // 2, 1)
    sel = ctx.matrix_from_result_where(cores, n, ">=", k)
    X, info = ctx.extract_rows_of(S, sel, -1, sel, -1, keep_shape=True)
    Y, tmp = products(ctx, sel, S, sel, n)
    same = same_operand(ctx, X, Y)
    ok &= same
    print("  1 k-core vertex set, k = %d of degeneracy %d: %d vertices, kept %d of %d scanned, %d hub chunks; routes %s"
          % (k, top, sel.nnz, info["kept"], info["scanned"], info["hub_chunks"], "equal" if same else "DIFFERENT"), flush=True)
    for h in [X, Y] + tmp:
        h.free()
    e1 = show("extract_rows_of, KEEP_SHAPE", wall_ms(ctx, lambda: [ctx.extract_rows_of(S, sel, -1, sel, -1, keep_shape=True)[0]], reps))

    def two_products():
        m, hs = products(ctx, sel, S, sel, n)
        return [m] + hs

    b1 = show("baseline: D_k * S * D_k, two products and two copies", wall_ms(ctx, two_products, reps))
    print("    extract / baseline = %.3f" % (e1 / b1), flush=True)

    # ---- 2. a random half, ascending, relabelled
    rng = np.random.default_rng(1)
    V = np.sort(rng.permutation(n)[:n // 2]).astype(np.int32)
    P = ctx.upload(np.arange(V.size + 1, dtype=np.int32), V, n)
    PT = ctx.transpose(P)
    X, info = ctx.extract(S, V, V)
    Y, tmp = products(ctx, P, S, PT, V.size)
    same = same_operand(ctx, X, Y)
    ok &= same
    print("  2 random half relabelled: %d vertices, kept %d of %d scanned, monotone %d; routes %s"
          % (V.size, info["kept"], info["scanned"], info["cols_monotone"], "equal" if same else "DIFFERENT"), flush=True)
    if args.check and not big:
        Z = scipy_route(ctx, S, V, V)
        same = same_operand(ctx, X, Z)
        ok &= same
        print("    check against scipy: %s" % ("equal" if same else "DIFFERENT"), flush=True)
        Z.free()
    for h in [X, Y] + tmp:
        h.free()
    e2 = show("extract, host lists", wall_ms(ctx, lambda: [ctx.extract(S, V, V)[0]], reps))

    def perm_products():
        m, hs = products(ctx, P, S, PT, V.size)
        return [m] + hs

    b2 = show("baseline: P_I * S * P_J^T, two products and two copies", wall_ms(ctx, perm_products, reps))
    sreps = 1 if big else reps
    s2 = show("baseline: download + scipy S[I][:, J] + upload (%d run%s)" % (sreps, "" if sreps == 1 else "s"),
              wall_ms(ctx, lambda: [scipy_route(ctx, S, V, V)], sreps, 0 if big else 1))
    print("    extract / products = %.3f, extract / scipy = %.4f" % (e2 / b2, e2 / s2), flush=True)
    P.free()
    PT.free()

    # ---- 3. the degree-descending permutation
    p = np.argsort(-deg, kind="stable").astype(np.int32)
    X, info = ctx.extract(S, p, p)
    print("  3 degree-descending permutation: kept %d, monotone %d, sorted by %d, %d hub chunks"
          % (info["kept"], info["cols_monotone"], info["sorted_by"], info["hub_chunks"]), flush=True)
    if args.check and not big:
        Z = scipy_route(ctx, S, p, p)
        same = same_operand(ctx, X, Z)
        ok &= same
        print("    check against scipy: %s" % ("equal" if same else "DIFFERENT"), flush=True)
        Z.free()
    e3 = show("extract, host lists", wall_ms(ctx, lambda: [ctx.extract(S, p, p)[0]], reps))
    s3 = show("baseline: download + scipy S[p][:, p] + upload (%d run%s)" % (sreps, "" if sreps == 1 else "s"),
              wall_ms(ctx, lambda: [scipy_route(ctx, S, p, p)], sreps, 0 if big else 1))
    print("    extract / scipy = %.4f" % (e3 / s3), flush=True)
    t0, t1 = ctx.triangle_count(S), ctx.triangle_count(X)
    ok &= t0 == t1
    print("    triangles: %d original, %d relabelled" % (t0, t1), flush=True)
    show("triangle_count, original", wall_ms(ctx, lambda: (ctx.triangle_count(S), [])[1], reps))
    show("triangle_count, relabelled", wall_ms(ctx, lambda: (ctx.triangle_count(X), [])[1], reps))
    show("local_clustering, original", wall_ms(ctx, lambda: [ctx.local_clustering(S)[0]], reps))
    show("local_clustering, relabelled", wall_ms(ctx, lambda: [ctx.local_clustering(X)[0]], reps))
    X.free()

    # ---- the stage split and the lanes sweep
    St = ctx_timed.upload(*S.download(), n)
    selt = ctx_timed.matrix_from_result_where(ctx_timed.core_numbers(St)[0], n, ">=", k)
    cases = (("1 k-core", lambda c, M, sl: c.extract_rows_of(M, sl, -1, sl, -1, keep_shape=True)[0]),
             ("2 half", lambda c, M, sl: c.extract(M, V, V)[0]),
             ("3 permutation", lambda c, M, sl: c.extract(M, p, p)[0]))
    for label, fn in cases:
        stderr_of(lambda: fn(ctx_timed, St, selt).free())       # warm-up: the workspace
        for ln in stderr_of(lambda: fn(ctx_timed, St, selt).free()).splitlines():
            print("    parts, %s: %s" % (label, ln.strip()), flush=True)
    selt.free()
    St.free()
    for lanes in (0, 4, 16, 64):
        ctx.set_option("extract_lanes", lanes)
        for label, fn in cases:
            show("EXTRACT_LANES %2d, %s" % (lanes, label), wall_ms(ctx, lambda: [fn(ctx, S, sel)], reps))
    ctx.set_option("extract_lanes", 0)
    for h in (sel, cores, S):
        h.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="*", default=["rmat22", "g500_18"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-max", type=int, default=40_000_000, help="above this nnz the scipy baseline runs once, unchecked")
    ap.add_argument("--check", action="store_true", help="compare with scipy's result too (graphs up to --scipy-max)")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_EXTRACT_TIMING")
    ok = True
    for g in args.graphs:
        if g.startswith("rmat") and g[4:].isdigit():
            scale = int(g[4:])
            name, abc = "R-MAT %d, edge factor 16, (0.30, 0.25, 0.25)" % scale, (0.30, 0.25, 0.25)
        elif g.startswith("g500_") and g[5:].isdigit():
            scale = int(g[5:])
            name, abc = "Graph500-skew R-MAT %d, edge factor 16, (0.57, 0.19, 0.19)" % scale, (0.57, 0.19, 0.19)
        else:
            sys.exit("unknown graph %s: rmat<scale> or g500_<scale>" % g)
        ok &= measure(ctx, ctx_timed, name, *bspgemm.gen_rmat(scale, 16, abc, seed=1), args)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
