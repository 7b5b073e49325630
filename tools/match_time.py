#!/usr/bin/env python3
"""What the device-resident maximal matching (bspgemm_maximal_matching) costs on an MI355X, in whole and in parts, under each
of its three orders and under every BSPGEMM_OPT_MATCH_LANES, beside the only way to get a matching without it: download the
operand and match it on the host.
    python tools/match_time.py [--rmat 22] [--skew 18] [--ef 16] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the result is outside.

Graphs: the R-MAT (0.30, 0.25, 0.25), seed 7, of scale --rmat (the benchmark's family) and the Graph500-skew R-MAT (0.57, 0.19,
0.19), seed 1, of scale --skew, both with edge factor --ef.  Per graph and order (natural, random, light; seed 0):
    whole     Context.maximal_matching(A, order) on the operand as generated (the call symmetrizes it), with the pairs, the
              rounds, the entries walked over all rounds and the hub chunks: 4 n bytes would cross the link
    parts     the same call on a second context created under BSPGEMM_MATCH_TIMING, which synchronises behind every launch
              and prints its own host-clock sums: symmetrize, the seed, the point, hub and pair launches, the read-backs and
              the longest round; and from them the time per round.  The extra synchronisations make its total a little
              larger than `whole`.
    lanes     the whole call under BSPGEMM_OPT_MATCH_LANES 4, 16 and 64 (0, the automatic choice, is `whole`)
    baseline  A.download()                                          the whole operand over the link
              sequential greedy over the sorted edges (tests/match_ref.py greedy)   up to --greedy-max stored entries
              the numpy round model (tests/match_ref.py matching)                   up to --numpy-max stored entries
and once per graph `symmetrize alone`, for comparison with the part above.
--check compares the device's mates under every lanes value with each other and with each host baseline that ran.  No
threshold: the numbers are the result."""
import argparse
import re
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import host_baseline, show, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm
import match_ref

SEED = 0


def host_greedy(A, order):
    rp, ci = A.download()
    srp, sci = match_ref.simple(rp, ci, A.rows)
    return match_ref.greedy(srp, sci, A.rows, order, SEED)


def host_model(A, order):
    rp, ci = A.download()
    return match_ref.matching(rp, ci, A.rows, order, SEED).mate


def measure(ctx, ctx_timed, name, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    At = ctx_timed.upload(rp, ci, n)
    print("%s: n = %d, nnz = %d" % (name, n, A.nnz), flush=True)
    show("    symmetrize alone", wall_ms(ctx, lambda: [ctx.symmetrize(A, drop_diagonal=True)], args.reps))
    show("    baseline: download of the operand", wall_ms(ctx, lambda: (A.download(), [])[1], args.reps))
    ok = True
    for order in match_ref.ORDERS:
        res = {}

        def run():
            P, _, res["info"] = ctx.maximal_matching(A, order, SEED)
            return [P]

        whole = show("    maximal_matching %-8s (whole call)" % order, wall_ms(ctx, run, args.reps))
        print("      %(pairs)d pairs, %(rounds)d rounds, %(entries_walked)d entries walked, %(hub_chunks)d hub chunks, %(lanes)d lanes"
              % res["info"], flush=True)
        stderr_of(lambda: ctx_timed.maximal_matching(At, order, SEED)[0].free())  # warm-up: workspaces
        lines = stderr_of(lambda: ctx_timed.maximal_matching(At, order, SEED)[0].free())
        for ln in lines.splitlines():
            print("      parts: " + ln.strip(), flush=True)
            m = re.search(r"\+ (\d+) point launches ([0-9.]+) \+ hub launches ([0-9.]+) \+ pair launches ([0-9.]+) \+ read-backs ([0-9.]+)", ln)
            if m and int(m.group(1)):
                k = int(m.group(1))
                print("      per round: %.1f us point, %.1f us hub, %.1f us pair, %.1f us read-back" %
                      tuple(1e3 * float(m.group(i)) / k for i in (2, 3, 4, 5)), flush=True)
        mates = {}
        for lanes in (4, 16, 64):
            ctx.set_option("match_lanes", lanes)
            show("    MATCH_LANES %2d, %-8s" % (lanes, order), wall_ms(ctx, run, args.reps))
            if args.check:
                P, mates[lanes], _ = ctx.maximal_matching(A, order, SEED, mate=True)
                P.free()
        ctx.set_option("match_lanes", 0)
        got = None
        if args.check:
            P, got, _ = ctx.maximal_matching(A, order, SEED, mate=True)
            P.free()
            same = all(np.array_equal(got, m) for m in mates.values())
            ok &= same
            print("      check of every MATCH_LANES against each other: %s" % ("equal" if same else "DIFFERENT"), flush=True)
        for label, fn, limit in (("sequential greedy over the sorted edges", host_greedy, args.greedy_max),
                                 ("the numpy round model", host_model, args.numpy_max)):
            ok &= host_baseline(label, lambda: fn(A, order), limit, A.nnz, whole, got)
    At.free()
    A.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rmat", type=int, default=22, help="scale of the (0.30, 0.25, 0.25) R-MAT (0: none)")
    ap.add_argument("--skew", type=int, default=18, help="scale of the Graph500-skew R-MAT (0: none)")
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--greedy-max", type=int, default=5_000_000, help="largest nnz for the sequential host greedy")
    ap.add_argument("--numpy-max", type=int, default=5_000_000, help="largest nnz for the numpy round model")
    ap.add_argument("--check", action="store_true", help="compare the mates with each other and with the host baselines that run")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_MATCH_TIMING")
    ok = True
    if args.rmat:
        ok &= measure(ctx, ctx_timed, "R-MAT %d, edge factor %d, (0.30, 0.25, 0.25)" % (args.rmat, args.ef),
                      *bspgemm.gen_rmat(args.rmat, args.ef, (0.30, 0.25, 0.25), seed=7), args)
    if args.skew:
        ok &= measure(ctx, ctx_timed, "Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (args.skew, args.ef),
                      *bspgemm.gen_rmat(args.skew, args.ef, (0.57, 0.19, 0.19), seed=1), args)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
