#!/usr/bin/env python3
"""What the device-resident connected components (bspgemm_connected_components) cost on an MI355X, beside the only way to
get min-vertex labels without them: download the operand and label it on the host.
    python tools/cc_time.py [--scale 18] [--ef 16] [--reps 6] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the result is outside.

Two graphs that the other measurements use, symmetrized on the device (bspgemm_matrix_symmetrize) before the timer starts:
the benchmark's mild-skew R-MAT --scale, edge factor --ef, (0.45, 0.15, 0.15), seed 1, and the Graph500-skew R-MAT of the
same size, (0.57, 0.19, 0.19), seed 1.
    cc        Context.connected_components(A): everything stays on the device, 4 n bytes of labels would cross the link
    baseline  A.download()                                       the whole operand over the link
              scipy connected_components(directed, weak)         on the host
              np.minimum.at over the labels, then index          the min-id canonicalisation
--check compares the two label arrays first.  Also printed: the rounds, the time per round, and the bytes per round of the
model 4 nnz + 4 (n + 1) + 8 n (col_idx and row_ptr read by the hook, parent[] read and written by the jump; the gathers of
parent[] come on top) against a copy rate of 6.0-6.3 TB/s."""
import argparse
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import show, wall_ms
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components
import bspgemm


def baseline(A):
    """(labels int32[n], ncomponents) by what the parent commit offers: the operand downloaded and labelled on the host"""
    rp, ci = A.download()
    n = A.rows
    ncomp, comp = connected_components(csr_matrix((np.ones(ci.size, np.int8), ci, rp), shape=(n, n)), directed=True,
                                       connection="weak")
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.int32), int(ncomp)


def measure(ctx, name, rp, ci, n, args):
    D = ctx.upload(rp, ci, n)
    A = ctx.symmetrize(D)
    D.free()
    print("%s, symmetrized: n = %d, nnz = %d" % (name, n, A.nnz), flush=True)
    if args.check:
        P, count, rounds = ctx.connected_components(A)
        got = P.download()[1]
        P.free()
        exp, e_count = baseline(A)
        same = np.array_equal(got, exp) and count == e_count
        print("    check %s (%d components, largest %d)" % ("equal" if same else "DIFFERENT", count, int(np.bincount(got).max())),
              flush=True)
        if not same:
            sys.exit(1)
    res = {}

    def run_cc():
        P, res["count"], res["rounds"] = ctx.connected_components(A)
        return [P]

    def run_baseline():
        baseline(A)
        return []

    new = show("connected_components (whole call)", wall_ms(ctx, run_cc, args.reps))
    per_round = new / max(res["rounds"], 1)
    model = 4 * A.nnz + 4 * (n + 1) + 8 * n
    print("    %d components, %d rounds, %.3f ms per round; model %.2f MB per round: %.1f us at 6.0 TB/s, %.2f TB/s achieved" %
          (res["count"], res["rounds"], per_round, model / 1e6, model / 6.0e12 * 1e6, model / (per_round * 1e-3) / 1e12), flush=True)
    old = show("baseline (download + scipy + min-id)", wall_ms(ctx, run_baseline, args.reps))
    print("    cc %.3f ms against %.3f ms: %s" % (new, old, "no slower" if new <= old else "SLOWER"), flush=True)
    A.free()
    return new <= old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--check", action="store_true", help="compare the two label arrays first")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ok = measure(ctx, "R-MAT %d, edge factor %d, (0.45, 0.15, 0.15)" % (args.scale, args.ef),
                 *bspgemm.gen_rmat(args.scale, args.ef, (0.45, 0.15, 0.15), seed=1), args)
    ok &= measure(ctx, "Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (args.scale, args.ef),
                  *bspgemm.gen_rmat(args.scale, args.ef, (0.57, 0.19, 0.19), seed=1), args)
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
