#!/usr/bin/env python3
"""What the device-resident k-core decomposition (bspgemm_core_numbers) costs on an MI355X, in whole and in parts, beside the
only way to get core numbers without it: download the operand and peel it on the host.
    python tools/kcore_time.py [--scales 16 20 22] [--ef 16] [--powerlaw 1048576] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the result is outside.

Graphs: the Graph500-skew R-MAT (0.57, 0.19, 0.19), seed 1, of every --scales value with edge factor --ef, and the power-law
generator with --powerlaw vertices, mean degree --ef, alpha 2.1.  Per graph:
    whole     Context.core_numbers(A) on the operand as generated (the call symmetrizes it): 4 n bytes would cross the link
    parts     the same call on a second context created under BSPGEMM_KCORE_TIMING, which synchronises behind every kernel
              and prints its own host-clock sums: symmetrize, the scans, the peel launches, the read-backs, the number of
              scans and of peel launches, and the longest single peel launch (what a hub row in the frontier costs: one
              wave walks it, 64 entries per step) with its level and frontier size.  The extra synchronisations make its
              total a little larger than `whole`.
    symmetrize alone, for comparison with the part above
    baseline  A.download()                                    the whole operand over the link
              numpy level-synchronous peeling on the host      graphs of up to --numpy-max stored entries
              networkx.core_number (pure Python)               graphs of up to --nx-max stored entries
--check compares the device's core numbers with each host baseline that ran.  No threshold: the numbers are the result."""
import argparse
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import host_baseline, show, stderr_of, timed_context, wall_ms
import numpy as np
from scipy.sparse import csr_matrix
import bspgemm


def host_simple(rp, ci, n):
    """A | A^T without the diagonal, sorted rows (scipy)"""
    A = csr_matrix((np.ones(ci.size, np.int8), ci, rp), shape=(n, n)).tocoo()
    keep = A.row != A.col
    r, c = np.concatenate([A.row[keep], A.col[keep]]), np.concatenate([A.col[keep], A.row[keep]])
    S = csr_matrix((np.ones(r.size, np.int8), (r, c)), shape=(n, n))
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices


def host_numpy(A):
    """core numbers by what the library offered before: the operand downloaded, symmetrized and peeled level by level"""
    rp, ci = A.download()
    n = A.rows
    srp, sci = host_simple(rp, ci, n)
    deg = np.diff(srp)
    core = np.zeros(n, np.int32)
    alive = np.ones(n, bool)
    k = 0
    left = n
    while left:
        k = max(k, int(deg[alive].min()))
        f = np.flatnonzero(alive & (deg <= k))
        while f.size:
            core[f] = k
            alive[f] = False
            left -= f.size
            lens = srp[f + 1] - srp[f]
            total = int(lens.sum())
            if not total:
                break
            at = np.repeat(srp[f] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(total)
            nb = sci[at]
            nb = nb[alive[nb]]
            np.subtract.at(deg, nb, 1)
            f = np.unique(nb[deg[nb] <= k])
        k += 1
    return core


def host_networkx(A):
    import networkx as nx
    rp, ci = A.download()
    n = A.rows
    G = nx.Graph()
    G.add_nodes_from(range(n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = rows != ci
    G.add_edges_from(zip(rows[keep].tolist(), ci[keep].tolist()))
    by_vertex = nx.core_number(G)
    return np.fromiter((by_vertex[v] for v in range(n)), np.int32, n)


def measure(ctx, ctx_timed, name, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    print("%s: n = %d, nnz = %d" % (name, n, A.nnz), flush=True)
    res = {}

    def run():
        R, res["top"], res["rounds"] = ctx.core_numbers(A)
        return [R]

    whole = show("    core_numbers (whole call)", wall_ms(ctx, run, args.reps))
    print("    degeneracy %d, %d peel launches" % (res["top"], res["rounds"]), flush=True)
    show("    symmetrize alone", wall_ms(ctx, lambda: [ctx.symmetrize(A, drop_diagonal=True)], args.reps))
    At = ctx_timed.upload(rp, ci, n)
    stderr_of(lambda: ctx_timed.core_numbers(At)[0].free())  # warm-up: workspaces, result cache
    lines = stderr_of(lambda: ctx_timed.core_numbers(At)[0].free())
    At.free()
    for ln in lines.splitlines():
        print("    parts: " + ln.strip(), flush=True)
    show("    baseline: download of the operand", wall_ms(ctx, lambda: (A.download(), [])[1], args.reps))
    got = None
    if args.check:
        R = ctx.core_numbers(A)[0]
        got = R.download_values()
        R.free()
    ok = True
    for label, fn, limit in (("numpy level-synchronous peeling", host_numpy, args.numpy_max),
                             ("networkx.core_number", host_networkx, args.nx_max)):
        ok &= host_baseline(label, lambda: fn(A), limit, A.nnz, whole, got, indent="    ")
    A.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--powerlaw", type=int, default=1 << 20, help="vertices of the power-law graph (0: none)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=100_000_000, help="largest nnz for the numpy host baseline")
    ap.add_argument("--nx-max", type=int, default=1_500_000, help="largest nnz for the networkx host baseline")
    ap.add_argument("--check", action="store_true", help="compare the core numbers with the host baselines that run")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_KCORE_TIMING")
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
