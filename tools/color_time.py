#!/usr/bin/env python3
"""What the device-resident greedy colouring (bspgemm_graph_coloring) costs on an MI355X, in whole and in parts, under each
of its three orders, beside the only way to get a colouring without it: download the operand and colour it on the host.
    python tools/color_time.py [--scales 16 20 22] [--ef 16] [--powerlaw 1048576] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the result is outside.

Graphs: the Graph500-skew R-MAT (0.57, 0.19, 0.19), seed 1, of every --scales value with edge factor --ef, and the power-law
generator with --powerlaw vertices, mean degree --ef, alpha 2.1.  Per graph and order (natural, random, largest; seed 0):
    whole     Context.graph_coloring(A, order) on the operand as generated (the call symmetrizes it), with the number of
              colours and of frontier launches (rounds): 4 n bytes would cross the link
    parts     the same call on a second context created under BSPGEMM_COLOR_TIMING, which synchronises behind every launch
              and prints its own host-clock sums: symmetrize, the count (init, count and seed), the frontier launches, the
              read-backs, and the longest single launch (what a hub row in the frontier costs: one wave walks it, 64 entries
              per step) with its frontier size; and from them the time per launch.  The extra synchronisations make its
              total a little larger than `whole`.
    baseline  A.download()                                      the whole operand over the link
              the numpy level-synchronous model (tests/color_ref.py)  graphs of up to --numpy-max stored entries
              networkx.greedy_color in the same vertex order    graphs of up to --nx-max stored entries
and once per graph `symmetrize alone`, for comparison with the part above.
--check compares the device's colours with each host baseline that ran.  No threshold: the numbers are the result."""
import argparse
import re
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import host_baseline, show, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm
import color_ref

ORDERS = ("natural", "random", "largest")
SEED = 0


def host_model(A, order):
    """colours by what the library offered before: the operand downloaded, symmetrized and coloured round by round"""
    rp, ci = A.download()
    return color_ref.coloring(rp, ci, A.rows, order, SEED)[0]


def host_networkx(A, order):
    import networkx as nx
    rp, ci = A.download()
    n = A.rows
    G = nx.Graph()
    G.add_nodes_from(range(n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = rows != ci
    G.add_edges_from(zip(rows[keep].tolist(), ci[keep].tolist()))
    deg = np.fromiter((G.degree(v) for v in range(n)), np.int64, n)
    visit = color_ref.visit_order(color_ref.keys(n, order, SEED, deg)).tolist()
    by_vertex = nx.greedy_color(G, strategy=lambda g, c: visit)
    return np.fromiter((by_vertex[v] for v in range(n)), np.int32, n)


def measure(ctx, ctx_timed, name, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    At = ctx_timed.upload(rp, ci, n)
    print("%s: n = %d, nnz = %d" % (name, n, A.nnz), flush=True)
    show("    symmetrize alone", wall_ms(ctx, lambda: [ctx.symmetrize(A, drop_diagonal=True)], args.reps))
    show("    baseline: download of the operand", wall_ms(ctx, lambda: (A.download(), [])[1], args.reps))
    ok = True
    for order in ORDERS:
        res = {}

        def run():
            P, res["colors"], res["rounds"] = ctx.graph_coloring(A, order, SEED)
            return [P]

        whole = show("    graph_coloring %-8s (whole call)" % order, wall_ms(ctx, run, args.reps))
        print("      %d colours, %d launches (rounds)" % (res["colors"], res["rounds"]), flush=True)
        stderr_of(lambda: ctx_timed.graph_coloring(At, order, SEED)[0].free())  # warm-up: workspaces
        lines = stderr_of(lambda: ctx_timed.graph_coloring(At, order, SEED)[0].free())
        for ln in lines.splitlines():
            print("      parts: " + ln.strip(), flush=True)
            m = re.search(r"\+ (\d+) launches ([0-9.]+) \+ read-backs ([0-9.]+)", ln)
            if m and int(m.group(1)):
                k = int(m.group(1))
                print("      per launch: %.1f us in the kernel, %.1f us in its read-back" %
                      (1e3 * float(m.group(2)) / k, 1e3 * float(m.group(3)) / (k + 1)), flush=True)
        got = None
        if args.check:
            P = ctx.graph_coloring(A, order, SEED)[0]
            got = P.download()[1]
            P.free()
        for label, fn, limit in (("numpy level-synchronous model", host_model, args.numpy_max),
                                 ("networkx.greedy_color", host_networkx, args.nx_max)):
            ok &= host_baseline(label, lambda: fn(A, order), limit, A.nnz, whole, got)
    At.free()
    A.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--powerlaw", type=int, default=1 << 20, help="vertices of the power-law graph (0: none)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=20_000_000, help="largest nnz for the numpy host baseline")
    ap.add_argument("--nx-max", type=int, default=1_500_000, help="largest nnz for the networkx host baseline")
    ap.add_argument("--check", action="store_true", help="compare the colours with the host baselines that run")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_COLOR_TIMING")
    ok = True
    for scale in args.scales:
        ok &= measure(ctx, ctx_timed, "Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (scale, args.ef),
                      *bspgemm.gen_rmat(scale, args.ef, (0.57, 0.19, 0.19), seed=1), args)
    if args.powerlaw:
        ok &= measure(ctx, ctx_timed, "power-law, mean degree %d, alpha 2.1" % args.ef,
                      *bspgemm.gen_powerlaw(args.powerlaw, args.ef, seed=1), args)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
