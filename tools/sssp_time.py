#!/usr/bin/env python3
"""What the device-resident shortest paths (bspgemm_sssp) cost on an MI355X, in whole and in parts, under every bucket width of
the sweep behind BSPGEMM_SSSP_DELTA_C and under every lanes value, beside a host Dijkstra and the unit-weight floor.
    python tools/sssp_time.py [--rmat 22] [--skew 18] [--grid 2048] [--ef 16] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised.

Graphs: the R-MAT (0.30, 0.25, 0.25), seed 7, of scale --rmat, symmetrized on the device; the Graph500-skew R-MAT (0.57, 0.19,
0.19), seed 1, of scale --skew as generated (directed); both with edge factor --ef; and the --grid x --grid 4-neighbour grid,
the high-diameter case where the rounds dominate.  The lengths are bspgemm_weights_hashed(seed 0, [1, 255]), symmetric on
the two undirected graphs.  The source is the vertex with the longest row (the grid: a corner).  Per graph:
    whole     Context.sssp(A, W, source) with the default delta, with the counts of its info: 8 n bytes cross the link
    parts     the same call on a second context created under BSPGEMM_SSSP_TIMING, which synchronises behind every launch
              and prints its own host-clock sums: relax, hub, settle and advance launches, read-backs, the parent pass and
              the longest round.  The extra synchronisations make its total larger than `whole`.
    delta     the whole call under delta = max(1, c * (sum / nnz) / max(1, nnz / n)) for c = 1, 4, 16, 32, 64, 256, and under
              delta = 2^64 - 1 (Bellman-Ford in one bucket)
    lanes     the whole call under lanes 4, 16 and 64 (0, the automatic choice, is `whole`)
    parents   the whole call with the parent pass
    baseline  A.download() + W.download() + scipy.sparse.csgraph.dijkstra on the host   up to --dijkstra-max stored entries
              bspgemm_bfs_tree under PUSH from the same source: the unit-weight floor for one search
At the end: the total over the graphs per c, and the c with the smallest.  --check compares the distances of every variant
with each other and with the host Dijkstra where it ran.  No threshold: the numbers are the result."""
import argparse
import sys
import time

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import show, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm
import sssp_ref

SWEEP_C = (1, 4, 16, 32, 64, 256)
INF = sssp_ref.INF


def grid(side):
    """the side x side 4-neighbour grid, both directions stored, rows ascending"""
    v = np.arange(side * side, dtype=np.int64).reshape(side, side)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    rows, cols = np.concatenate([a, b]), np.concatenate([b, a])
    o = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=side * side))])
    return rp.astype(np.int32), cols[o].astype(np.int32), side * side


def host_dijkstra(A, W, source):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    rp, ci = A.download()
    w = W.download()
    M = sp.csr_matrix((w.astype(np.float64), ci, rp), shape=(A.rows, A.rows))     # (lengths >= 1; the graphs have no repeats)
    d = dijkstra(M, directed=True, indices=source)
    return np.where(np.isinf(d), float(INF), d)


def measure(ctx, ctx_timed, name, A, At, symmetric, source, args, totals):
    n = A.rows
    W = ctx.weights_hashed(A, 0, 1, 255, symmetric=symmetric)
    Wt = ctx_timed.weights_hashed(At, 0, 1, 255, symmetric=symmetric)
    print("%s: n = %d, nnz = %d, source %d, weight sum %d" % (name, n, A.nnz, source, W.sum), flush=True)
    show("    weights_hashed", wall_ms(ctx, lambda: [ctx.weights_hashed(A, 0, 1, 255, symmetric=symmetric)], args.reps))
    res = {}

    def run(delta=0, lanes=0, parents=False):
        def fn():
            res["dist"], _, res["info"] = ctx.sssp(A, W, source, delta=delta, lanes=lanes, parents=parents)
        return fn

    def counts():
        return ("  delta %(delta)d: %(rounds)d rounds, %(buckets)d buckets, %(entries_walked)d walked, %(improved)d improved, "
                "%(hub_chunks)d hub chunks, %(lanes)d lanes, reached %(reached)d, dist_max %(dist_max)d" % res["info"])

    whole = show("    sssp, default delta (whole call)", wall_ms(ctx, run(), args.reps))
    print("    " + counts(), flush=True)
    base = res["dist"].copy()
    ok = True
    stderr_of(lambda: ctx_timed.sssp(At, Wt, source))                    # warm-up: the workspace
    for ln in stderr_of(lambda: ctx_timed.sssp(At, Wt, source)).splitlines():
        print("      parts: " + ln.strip(), flush=True)
    for c in SWEEP_C + (None,):
        delta = INF if c is None else sssp_ref.default_delta(W.sum, A.nnz, n, c)
        ms = show("    delta c = %-4s" % ("inf" if c is None else c), wall_ms(ctx, run(delta), args.reps))
        print("    " + counts(), flush=True)
        totals.setdefault(c, 0.0)
        totals[c] += ms
        if args.check:
            ok &= np.array_equal(res["dist"], base)
    for lanes in (4, 16, 64):
        show("    lanes %2d, default delta" % lanes, wall_ms(ctx, run(0, lanes), args.reps))
        if args.check:
            ok &= np.array_equal(res["dist"], base)
    show("    with the parent pass, default delta", wall_ms(ctx, run(0, 0, True), args.reps))
    if args.check:
        print("      check of every delta and lanes against the default: %s" % ("equal" if ok else "DIFFERENT"), flush=True)

    def bfs():
        r, res["bfs"] = ctx.bfs_tree(A, None, source, "push")
        return [r]

    ms = show("    baseline: bfs_tree PUSH from the same source", wall_ms(ctx, bfs, args.reps))
    print("      depth %d, reached %d: sssp is %.1f x the unit-weight search" % (res["bfs"]["depth"], res["bfs"]["reached"], whole / ms),
          flush=True)
    if A.nnz > args.dijkstra_max:
        print("      baseline: download + scipy dijkstra: not run (more than %d stored entries)" % args.dijkstra_max, flush=True)
    else:
        t = time.perf_counter()
        ref = host_dijkstra(A, W, source)
        hms = (time.perf_counter() - t) * 1e3
        print("      baseline: download + scipy dijkstra                  %10.3f ms  (once): %.1f x the whole call" % (hms, hms / whole),
              flush=True)
        if args.check:
            same = np.array_equal(np.where(base == np.uint64(INF), float(INF), base.astype(np.float64)), ref)
            ok &= same
            print("      check against scipy dijkstra: %s" % ("equal" if same else "DIFFERENT"), flush=True)
    Wt.free()
    W.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rmat", type=int, default=22, help="scale of the (0.30, 0.25, 0.25) R-MAT, symmetrized (0: none)")
    ap.add_argument("--skew", type=int, default=18, help="scale of the Graph500-skew R-MAT (0: none)")
    ap.add_argument("--grid", type=int, default=2048, help="side of the grid (0: none)")
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dijkstra-max", type=int, default=300_000_000, help="largest nnz for the host Dijkstra")
    ap.add_argument("--check", action="store_true", help="compare the distances with each other and with the host Dijkstra")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_SSSP_TIMING")
    ok, totals = True, {}

    def graph(name, rp, ci, n, symmetrize, symmetric):
        A0 = ctx.upload(rp, ci, n)
        A = ctx.symmetrize(A0) if symmetrize else A0
        rp2, ci2 = A.download()
        At = ctx_timed.upload(rp2, ci2, n)
        source = int(np.argmax(np.diff(rp2)))
        good = measure(ctx, ctx_timed, name, A, At, symmetric, source, args, totals)
        At.free()
        if symmetrize:
            A.free()
        A0.free()
        return good

    if args.rmat:
        ok &= graph("R-MAT %d symmetrized, edge factor %d, (0.30, 0.25, 0.25)" % (args.rmat, args.ef),
                    *bspgemm.gen_rmat(args.rmat, args.ef, (0.30, 0.25, 0.25), seed=7), True, True)
    if args.skew:
        ok &= graph("Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (args.skew, args.ef),
                    *bspgemm.gen_rmat(args.skew, args.ef, (0.57, 0.19, 0.19), seed=1), False, False)
    if args.grid:
        ok &= graph("grid %d x %d" % (args.grid, args.grid), *grid(args.grid), False, True)
    print("total over the graphs, ms, per c of the sweep:", flush=True)
    for c, ms in totals.items():
        print("    c = %-4s %12.3f" % ("inf" if c is None else c, ms), flush=True)
    best = min((c for c in totals if c is not None), key=lambda c: totals[c])
    print("smallest total among the finite c: c = %d (BSPGEMM_SSSP_DELTA_C is %d)" % (best, bspgemm.SSSP_DELTA_C), flush=True)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
