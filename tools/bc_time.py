#!/usr/bin/env python3
"""What the device-resident betweenness centrality (bspgemm_betweenness) costs on an MI355X, in whole, per source and in
parts, beside a push search from the same sources (bspgemm_bfs_tree under PUSH: the forward sweep does its work plus one
64-bit atomic per DAG edge) and beside the only way to get the values without it: download the operand and run the numpy model
of the definition on the host.
    python tools/bc_time.py [--graphs rmat22 mild18] [--sources 8] [--seed 1] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls, which end synchronised and with the values on the host (16 n bytes cross the link).

Graphs: rmatS = the benchmark's R-MAT (0.30, 0.25, 0.25), seed 1, scale S, edge factor 16; mildS = the directed mild-skew
R-MAT of tools/scc_time.py (0.45, 0.15, 0.15); skewS = the Graph500-skew R-MAT (0.57, 0.19, 0.19).  The sources: seeded
vertices whose push search reaches at least half of what the best of 64 candidates reaches (the largest component).  Per graph:
    whole     all sources in one call, under BSPGEMM_OPT_BC_LANES 0, 4, 16, 64; ms per source
    single    every source in a call of its own (BC_LANES 0), and with zero sources (checks, init, read-out)
    search    bspgemm_bfs_tree under PUSH from the same sources, one call each, and their sum
    parts     all sources on a second context created under BSPGEMM_BC_TIMING, which synchronises behind every launch
              group and prints its own host-clock sums by stage, the hub launches' share among them
    baseline  A.download() + the numpy model for ONE source on the host, once
--check compares the values under every BC_LANES with each other and (graphs of up to --numpy-max entries) with the numpy
model of the definition.  No threshold: the numbers are the result."""
import argparse
import sys
import time

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import show, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm
import bc_ref as B

LANES = (0, 4, 16, 64)


def generate(name):
    kind, scale = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    abcd = {"rmat": (0.30, 0.25, 0.25), "mild": (0.45, 0.15, 0.15), "skew": (0.57, 0.19, 0.19)}[kind]
    return "R-MAT scale %d, edge factor 16, %r, seed 1" % (scale, abcd), bspgemm.gen_rmat(scale, 16, abcd, seed=1)


def search(ctx, A, s):
    tree, info = ctx.bfs_tree(A, None, int(s), "push")
    tree.free()
    return info


def pick_sources(ctx, A, n, k, seed):
    cand = np.random.default_rng(seed).integers(0, n, 64)
    reach = [search(ctx, A, s)["reached"] for s in cand]
    good = [int(s) for s, r in zip(cand, reach) if 2 * r >= max(reach)]
    return np.array(good[:k], np.int32), max(reach)


def measure(ctx, ctx_timed, title, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    At = ctx_timed.upload(rp, ci, n)
    nnz = A.nnz
    sources, reach = pick_sources(ctx, A, n, args.sources, args.seed)
    k = len(sources)
    print("%s: n = %d, nnz = %d, %d sources %s (the best candidate reaches %d vertices)" % (title, n, nnz, k, sources.tolist(), reach),
          flush=True)
    ok, values, whole = True, {}, {}
    for lanes in LANES:
        ctx.set_option("bc_lanes", lanes)
        whole[lanes] = show("    BC_LANES %d, %d sources (whole call)" % (lanes, k), wall_ms(ctx, lambda: (ctx.betweenness(A, sources), None)[1], args.reps))
        values[lanes] = ctx.betweenness(A, sources)
        print("      per source %.3f ms; info %s" % (whole[lanes] / max(k, 1), values[lanes][2]), flush=True)
    ctx.set_option("bc_lanes", 0)
    ms0 = show("    0 sources (checks, init, read-out)", wall_ms(ctx, lambda: (ctx.betweenness(A, []), None)[1], args.reps))
    singles, searches = [], []
    for s in sources:
        singles.append(show("    source %d alone" % s, wall_ms(ctx, lambda: (ctx.betweenness(A, [s]), None)[1], args.reps)))
        searches.append(show("    source %d, bspgemm_bfs_tree PUSH" % s, wall_ms(ctx, lambda: (search(ctx, A, s), None)[1], args.reps)))
        info = search(ctx, A, s)
        print("      the search: reached %d, depth %d, %d entries pushed" % (info["reached"], info["depth"], info["edges_pushed"]),
              flush=True)
    print("    sum over the sources: betweenness alone %.3f ms (less %d x the empty call: %.3f ms), push searches %.3f ms; "
          "one call for all %.3f ms" % (sum(singles), k, sum(singles) - k * ms0, sum(searches), whole[0]), flush=True)
    for lanes in LANES:
        ctx_timed.set_option("bc_lanes", lanes)
        stderr_of(lambda: ctx_timed.betweenness(At, sources))   # warm-up: workspaces
        for ln in stderr_of(lambda: ctx_timed.betweenness(At, sources)).splitlines():
            print("      parts, BC_LANES %d: %s" % (lanes, ln.strip()), flush=True)
    ctx_timed.set_option("bc_lanes", 0)
    t = time.perf_counter()
    h_rp, h_ci = A.download()
    t_down = (time.perf_counter() - t) * 1e3
    exp1 = B.model(h_rp, h_ci, n, sources[:1]) if nnz <= args.numpy_max else None
    ms = (time.perf_counter() - t) * 1e3
    if exp1 is not None:
        print("    baseline: download %.3f ms + the numpy model for one source on the host = %.3f ms (once); the device's call for "
              "that source %.3f ms" % (t_down, ms, singles[0] if singles else 0.0), flush=True)
    if args.check:
        same = all(np.array_equal(v[0], values[0][0]) and v[2] == values[0][2] for v in values.values())
        ok &= same
        print("      check of every BC_LANES against each other: %s" % ("equal" if same else "DIFFERENT"), flush=True)
        if exp1 is not None and k:
            got = ctx.betweenness(A, sources[:1])
            same = np.array_equal(got[0], exp1["fixed"]) and all(got[2][f] == exp1[f] for f in got[2])
            ok &= same
            print("      check of one source against the numpy model of the definition: %s" % ("equal" if same else "DIFFERENT"),
                  flush=True)
    At.free()
    A.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="*", default=["rmat22", "mild18"])
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=100_000_000, help="largest nnz for the numpy model of the definition")
    ap.add_argument("--check", action="store_true", help="compare the values with the numpy model and between the lane widths")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_BC_TIMING")
    ok = True
    for name in args.graphs:
        title, (rp, ci, n) = generate(name)
        ok &= measure(ctx, ctx_timed, title, rp, ci, n, args)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
