#!/usr/bin/env python3
"""What the device-resident multi-source BFS (bspgemm_bfs) costs on an MI355X, beside the only way to get levels without
it: the loop assembled from public calls, with the frontier downloaded every level and the levels stamped on the host.
    python tools/bfs_time.py [--scale 18] [--ef 16] [--sources 64] [--reps 6] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the results is outside.

Two graphs that the other measurements use: the benchmark's mild-skew R-MAT --scale, edge factor --ef, (0.45, 0.15, 0.15),
seed 1, and the Graph500-skew R-MAT of the same size, (0.57, 0.19, 0.19), seed 1; --sources sources drawn without
replacement (default_rng(9)).
    bfs       Context.bfs(A, sources): everything stays on the device
    baseline  per level  N = multiply_masked(F, A, V, complement)       the same product
                         N.download(), level[row, col] = d on the host  the frontier over the link
                         F = matrix_from_result(N)                      the same copy
                         V = setop(V, F, "or")                          the general union
--check compares the two results entry for entry first.  Also printed: per level the complement product's ms_total (its
HIP events) and, for the whole call, what is left of the wall time beside the products -- matrix_from_result, the merge,
the frees and the host's turn-arounds -- which bounds the merge's share from above."""
import argparse
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import show, wall_ms
import numpy as np
import bspgemm


def baseline(ctx, A, n, sources):
    """(level S x n int32 with -1 for unreached, depth) by the public calls of the parent commit"""
    S = len(sources)
    level = np.full((S, n), -1, np.int32)
    level[np.arange(S), sources] = 0
    V = ctx.upload(np.arange(S + 1, dtype=np.int32), np.asarray(sources, np.int32), n)
    F, d = V, 0
    while True:
        N = ctx.multiply_masked(F, A, V, complement=True)
        if N.nnz == 0:
            N.free()
            break
        d += 1
        rp, ci = N.download()
        level[np.repeat(np.arange(S), np.diff(rp)), ci] = d
        Nm = ctx.matrix_from_result(N, n)
        N.free()
        U = ctx.setop(V, Nm, "or")
        if F is not V:
            F.free()
        V.free()
        F, V = Nm, U
    if F is not V:
        F.free()
    V.free()
    return level, d


def bfs_dense(ctx, A, n, sources):
    R, depth, complete = ctx.bfs(A, sources)
    rp, ci = R.download()
    v = R.download_values()
    R.free()
    level = np.full((len(sources), n), -1, np.int32)
    level[np.repeat(np.arange(len(sources)), np.diff(rp)), ci] = v
    return level, depth, complete


def measure(ctx, name, rp, ci, n, args):
    sources = np.random.default_rng(9).choice(n, size=args.sources, replace=False).astype(np.int32)
    A = ctx.upload(rp, ci, n)
    print("%s: n = %d, nnz = %d, %d sources" % (name, n, A.nnz, sources.size), flush=True)
    if args.check:
        got, depth, complete = bfs_dense(ctx, A, n, sources)
        exp, b_depth = baseline(ctx, A, n, sources)
        same = np.array_equal(got, exp) and depth == b_depth and complete
        print("    check %s (%d reached entries, depth %d)" % ("equal" if same else "DIFFERENT", int((got >= 0).sum()), depth), flush=True)
        if not same:
            sys.exit(1)
    res = {}

    def run_bfs():
        R, res["depth"], _ = ctx.bfs(A, sources)
        res["nnz"] = R.nnz
        return [R]

    def run_baseline():
        baseline(ctx, A, n, sources)
        return []

    new = show("bfs (whole call)", wall_ms(ctx, run_bfs, args.reps))
    # the products of the last call: ages depth (level 1) .. 0 (the product that came back empty, or the last one)
    products = [ctx.stats(age)["ms_total"] for age in range(min(res["depth"], 15), -1, -1)]
    print("    depth %d, %d reached entries; complement products, ms_total per level: %s" %
          (res["depth"], res["nnz"], " ".join("%.3f" % p for p in products)), flush=True)
    print("    products %.3f ms of %.3f ms: %.1f %%; matrix_from_result + merge + frees + host: at most %.1f %%" %
          (sum(products), new, 100 * sum(products) / new, 100 * (new - sum(products)) / new), flush=True)
    old = show("baseline (public calls, host levels)", wall_ms(ctx, run_baseline, args.reps))
    print("    bfs %.3f ms against %.3f ms: %s" % (new, old, "no slower" if new <= old else "SLOWER"), flush=True)
    A.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--check", action="store_true", help="compare the two results entry for entry first")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    measure(ctx, "R-MAT %d, edge factor %d, (0.45, 0.15, 0.15)" % (args.scale, args.ef),
            *bspgemm.gen_rmat(args.scale, args.ef, (0.45, 0.15, 0.15), seed=1), args)
    measure(ctx, "Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (args.scale, args.ef),
            *bspgemm.gen_rmat(args.scale, args.ef, (0.57, 0.19, 0.19), seed=1), args)
    ctx.close()


if __name__ == "__main__":
    main()
