#!/usr/bin/env python3
"""What the device-resident strongly connected components (bspgemm_strongly_connected_components) cost on an MI355X, beside
the only way to get min-vertex labels without them: download the operand and label it on the host.
    python tools/scc_time.py [--scale 18] [--ef 16] [--reps 6] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the result is outside.

Two graphs that the other measurements use, as the generator emits them -- directed, not symmetrized: the benchmark's
mild-skew R-MAT --scale, edge factor --ef, (0.45, 0.15, 0.15), seed 1, and the Graph500-skew R-MAT of the same size,
(0.57, 0.19, 0.19), seed 1.
    scc       Context.strongly_connected_components(A): everything stays on the device, 4 n bytes of labels would cross the
              link
    baseline  A.download()                                       the whole operand over the link
              sum_duplicates, sort_indices                       (scipy's strong components want a canonical CSR)
              scipy connected_components(directed, strong)       on the host
              np.minimum.at over the labels, then index          the min-id canonicalisation
--check compares the two label arrays first.  Also printed: the rounds and the sweeps, the time per sweep, the bytes per
sweep of the model 4 nnz + 4 (n + 1) (col_idx and row_ptr; the gathers of the per-vertex arrays come on top) against a copy
rate of 6.0 TB/s, and the trim / forward / backward split of the same call on a second context created under
BSPGEMM_SCC_TIMING."""
import argparse
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import show, stderr_of, timed_context, wall_ms
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components
import bspgemm


def baseline(A):
    """(labels int32[n], ncomponents) by what the parent commit offers: the operand downloaded and labelled on the host"""
    rp, ci = A.download()
    n = A.rows
    G = csr_matrix((np.ones(ci.size, np.int8), ci, rp), shape=(n, n))
    G.sum_duplicates()
    G.sort_indices()
    ncomp, comp = connected_components(G, directed=True, connection="strong")
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.int32), int(ncomp)


def measure(ctx, ctx_timed, name, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    print("%s, directed: n = %d, nnz = %d" % (name, n, A.nnz), flush=True)
    if args.check:
        P, count, rounds, sweeps = ctx.strongly_connected_components(A)
        got = P.download()[1]
        P.free()
        exp, e_count = baseline(A)
        same = np.array_equal(got, exp) and count == e_count
        print("    check %s (%d components, largest %d)" % ("equal" if same else "DIFFERENT", count, int(np.bincount(got).max())),
              flush=True)
        if not same:
            sys.exit(1)
    res = {}

    def run_scc():
        P, res["count"], res["rounds"], res["sweeps"] = ctx.strongly_connected_components(A)
        return [P]

    def run_baseline():
        baseline(A)
        return []

    new = show("strongly_connected_components (whole call)", wall_ms(ctx, run_scc, args.reps))
    per_sweep = new / max(res["sweeps"], 1)
    model = 4 * A.nnz + 4 * (n + 1)
    print("    %d components, %d rounds, %d sweeps, %.3f ms per sweep; model %.2f MB per sweep: %.1f us at 6.0 TB/s, %.2f TB/s achieved" %
          (res["count"], res["rounds"], res["sweeps"], per_sweep, model / 1e6, model / 6.0e12 * 1e6,
           model / (per_sweep * 1e-3) / 1e12), flush=True)
    At = ctx_timed.upload(rp, ci, n)
    stderr_of(lambda: ctx_timed.strongly_connected_components(At)[0].free())     # warm-up: the workspace
    for ln in stderr_of(lambda: ctx_timed.strongly_connected_components(At)[0].free()).splitlines():
        print("    parts: " + ln.strip(), flush=True)
    At.free()
    old = show("baseline (download + scipy + min-id)", wall_ms(ctx, run_baseline, args.reps))
    print("    scc %.3f ms against %.3f ms: %s" % (new, old, "no slower" if new <= old else "SLOWER"), flush=True)
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
    ctx_timed = timed_context("BSPGEMM_SCC_TIMING")
    ok = measure(ctx, ctx_timed, "R-MAT %d, edge factor %d, (0.45, 0.15, 0.15)" % (args.scale, args.ef),
                 *bspgemm.gen_rmat(args.scale, args.ef, (0.45, 0.15, 0.15), seed=1), args)
    ok &= measure(ctx, ctx_timed, "Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (args.scale, args.ef),
                  *bspgemm.gen_rmat(args.scale, args.ef, (0.57, 0.19, 0.19), seed=1), args)
    ctx_timed.close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
