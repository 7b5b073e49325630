#!/usr/bin/env python3
"""What the single-source direction-optimising BFS (bspgemm_bfs_tree) costs on an MI355X, beside the only way to get one
source's levels without it, bspgemm_bfs with that one source, and beside scipy on the host.
    python tools/bfs_tree_time.py [--scales 18 22] [--ef 16] [--sources 8] [--reps 6] [--check] [--sweeps] [--log FILE]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the results is outside.

Graphs: at scale 18 the two R-MATs that the other measurements use -- the benchmark's mild skew (0.45, 0.15, 0.15) and the
Graph500 skew (0.57, 0.19, 0.19), edge factor --ef, seed 1 -- each directed as generated and symmetrised on the device
(bspgemm_matrix_symmetrize, diagonal dropped); at any larger scale the mild-skew graph symmetrised.  --sources sources are
drawn (default_rng(9)) from the largest weakly connected component, found on the device, among its vertices with out-edges.
Columns per source:
    auto / push / pull   Context.bfs_tree with AT given (the symmetrised graph is its own AT)
    auto, AT NULL        the call transposes inside where it pulls
    bfs, one source      Context.bfs(A, [source]): one complement product per level
    host                 A downloaded once (outside), scipy breadth_first_order per source (one repetition)
    GTEPS                stored entries of A with both ends reached / the auto time
--check first compares the levels with bspgemm_bfs and runs the tree check (parent one level up, over a stored edge, no
stored edge more than one level down).  --sweeps adds alpha x beta under AUTO and the lanes per frontier vertex under PUSH,
on the first two sources.  The last line says whether AUTO with AT given was no slower than bspgemm_bfs, minimum against
minimum, on every graph and source."""
import argparse
import statistics
import sys
import time

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import wall_ms
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import breadth_first_order
import bspgemm

LOG = None


def log(line):
    print(line, flush=True)
    if LOG:
        LOG.write(line + "\n")
        LOG.flush()


def dense(R, n):
    """(level, parent) as arrays of n, -1 where unreached"""
    rp, parent = R.download()
    level = R.download_values()
    reached = np.flatnonzero(np.diff(rp))
    lv, pa = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    lv[reached], pa[reached] = level, parent
    return lv, pa


def check(ctx, A, AT, G, rows, n, source):
    R, info = ctx.bfs_tree(A, AT, source)
    level, parent = dense(R, n)
    R.free()
    L, depth, complete = ctx.bfs(A, [source])
    l_rp, l_ci = L.download()
    l_v = L.download_values()
    L.free()
    ok = np.array_equal(np.flatnonzero(level >= 0), l_ci) and np.array_equal(level[l_ci], l_v) and depth == info["depth"]
    others = np.flatnonzero((level >= 0) & (np.arange(n) != source))
    ok = ok and level[source] == 0 and parent[source] == source
    ok = ok and bool((level[parent[others]] == level[others] - 1).all())
    ok = ok and bool((np.asarray(G[parent[others], others]).ravel() != 0).all())
    walked = level[rows] >= 0
    ok = ok and bool((level[G.indices[walked]] >= 0).all()) and bool((level[G.indices[walked]] <= level[rows[walked]] + 1).all())
    log("    check source %d: %s (%d reached, depth %d, pull_mask %s)" % (source, "equal to bspgemm_bfs, tree valid" if ok else "DIFFERENT",
                                                                          info["reached"], info["depth"], bin(info["pull_mask"])))
    if not ok:
        sys.exit(1)


def measure(ctx, name, A, AT, args, verdict):
    n = A.rows
    rp, ci = A.download()
    deg = np.diff(rp).astype(np.int64)
    P, ncomp, _ = ctx.connected_components(A)
    label = P.download()[1]
    P.free()
    big = np.bincount(label).argmax()
    pool = np.flatnonzero((label == big) & (deg > 0))
    sources = np.random.default_rng(9).choice(pool, size=min(args.sources, pool.size), replace=False).tolist()
    log("== %s: n = %d, nnz = %d, largest component %d vertices of %d components; sources %s"
        % (name, n, A.nnz, int((label == big).sum()), ncomp, sources))
    G = csr_matrix((np.ones(ci.size, np.int8), ci, rp), shape=(n, n))
    if args.check:
        rows = np.repeat(np.arange(n), deg)
        for s in sources[:1 if n > 1 << 20 else len(sources)]:
            check(ctx, A, AT, G, rows, n, s)
        del rows
    for s in sources:
        res = {}

        def tree(direction, at):
            def run():
                R, res["info"] = ctx.bfs_tree(A, at, s, direction)
                return [R]
            return run

        def bfs():
            R, res["depth"], _ = ctx.bfs(A, [s])
            return [R]

        col = {d: wall_ms(ctx, tree(d, AT), args.reps) for d in ("auto", "push", "pull")}
        R, info = ctx.bfs_tree(A, AT, s)
        level, _ = dense(R, n)
        R.free()
        edges = int(deg[level >= 0].sum())
        col["auto, AT NULL"] = wall_ms(ctx, tree("auto", None), args.reps)
        col["bfs, one source"] = wall_ms(ctx, bfs, args.bfs_reps)
        t = time.perf_counter()
        breadth_first_order(G, s, directed=True, return_predecessors=True)
        host = (time.perf_counter() - t) * 1e3
        a, b = min(col["auto"]), min(col["bfs, one source"])
        best = min(min(col["push"]), min(col["pull"]))
        verdict.append(a <= b)
        log("  source %8d: reached %d, depth %d, push/pull levels %d/%d, pull_mask %s, edges pushed %d of %d"
            % (s, info["reached"], info["depth"], info["push_levels"], info["pull_levels"], bin(info["pull_mask"]),
               info["edges_pushed"], edges))
        log("    " + " | ".join("%s min %.3f med %.3f" % (k, min(v), statistics.median(v)) for k, v in col.items())
            + " | host scipy %.1f ms" % host)
        log("    auto %.3f GTEPS; auto against bfs: %s (%.1fx); auto against the better of push and pull (%.3f ms): %s"
            % (edges / a * 1e-6, "no slower" if a <= b else "SLOWER", b / a, best, "no slower" if a <= best else "SLOWER (finding)"))
    if args.sweeps:
        for s in sources[:2]:
            for alpha in (4, 8, 15, 30, 60):
                cells = []
                for beta in (6, 18, 54):
                    ctx.set_option("bfs_alpha", alpha)
                    ctx.set_option("bfs_beta", beta)

                    def run():
                        return [ctx.bfs_tree(A, AT, s)[0]]
                    cells.append("beta %2d: %8.3f" % (beta, min(wall_ms(ctx, run, 3))))
                log("    sweep source %d alpha %2d: %s ms" % (s, alpha, "  ".join(cells)))
            ctx.set_option("bfs_alpha", 15)
            ctx.set_option("bfs_beta", 18)
            cells = []
            for lanes in (4, 16, 64, 0):
                ctx.set_option("bfs_push_lanes", lanes)

                def run():
                    return [ctx.bfs_tree(A, None, s, "push")[0]]
                cells.append("W %2d: %8.3f" % (lanes, min(wall_ms(ctx, run, 3))))
            ctx.set_option("bfs_push_lanes", 0)
            log("    sweep source %d push lanes (0 = per level): %s ms" % (s, "  ".join(cells)))


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[18, 22])
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--bfs-reps", type=int, default=None, help="repetitions of bspgemm_bfs (default: --reps)")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--sweeps", action="store_true")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.bfs_reps is None:
        args.bfs_reps = args.reps
    if args.log:
        LOG = open(args.log, "a")
    ctx = bspgemm.Context(0)
    verdict = []
    for scale in args.scales:
        skews = (("mild", (0.45, 0.15, 0.15)), ("Graph500-skew", (0.57, 0.19, 0.19))) if scale <= 18 else (("mild", (0.45, 0.15, 0.15)),)
        for what, abc in skews:
            A = ctx.upload(*bspgemm.gen_rmat(scale, args.ef, abc, seed=1))
            S = ctx.symmetrize(A, drop_diagonal=True)
            measure(ctx, "%s R-MAT %d, edge factor %d, symmetrised" % (what, scale, args.ef), S, S, args, verdict)
            S.free()
            if scale <= 18:
                AT = ctx.transpose(A)
                measure(ctx, "%s R-MAT %d, edge factor %d, directed" % (what, scale, args.ef), A, AT, args, verdict)
                AT.free()
            A.free()
    log("AUTO with AT given against bspgemm_bfs with one source, minimum against minimum: %s on %d of %d (graph, source) pairs"
        % ("no slower everywhere" if all(verdict) else "SLOWER somewhere", sum(verdict), len(verdict)))
    ctx.close()
    sys.exit(0 if all(verdict) else 1)


if __name__ == "__main__":
    main()
