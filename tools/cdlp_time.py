#!/usr/bin/env python3
"""What the device-resident label propagation (bspgemm_label_propagation) costs on an MI355X, in whole and in parts, beside
the only way to get the communities without it: download the operand and propagate on the host.
    python tools/cdlp_time.py [--scales 18 20 22] [--ef 16] [--powerlaw 1048576] [--iterations 10] [--reps 3] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised; freeing the result is outside.

Graphs: the Graph500-skew R-MAT (0.57, 0.19, 0.19), seed 1, of every --scales value with edge factor --ef, and the power-law
generator with --powerlaw vertices, mean degree --ef, alpha 2.1.  Per graph, --iterations iterations from label(v) = v:
    whole     Context.label_propagation(A, iterations) on the operand as generated (the call symmetrizes it), with the
              iterations run, converged, the communities and the vertices per degree class: 4 n bytes would cross the link
    parts     the same call on a second context created under BSPGEMM_LP_TIMING, which synchronises behind every class's
              launch and prints its own host-clock sums: symmetrize, the class lists, the iterations by class (lane, wave,
              workgroup, hub: the table's memset, the walk and the reduce), the read-backs and the longest iteration; and
              from them the time per iteration.  The extra synchronisations make its total a little larger than `whole`.
    classes   the whole call under BSPGEMM_OPT_LP_MIN_CLASS 1, 2 and 3: every row in the wave kernel at least, in the
              workgroup kernel at least, in the hub tables -- what the caps between the classes buy (same labels)
    baseline  A.download()                                      the whole operand over the link
              the numpy model (tests/cdlp_ref.py)               graphs of up to --numpy-max stored entries
and once per graph `symmetrize alone`, for comparison with the part above.
--check compares the device's labels and counters with the host model where it ran, and the labels under every
LP_MIN_CLASS with each other.  No threshold: the numbers are the result."""
import argparse
import re
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import host_baseline, show, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm
import cdlp_ref


def measure(ctx, ctx_timed, name, rp, ci, n, args):
    A = ctx.upload(rp, ci, n)
    At = ctx_timed.upload(rp, ci, n)
    K = args.iterations
    print("%s: n = %d, nnz = %d, %d iterations" % (name, n, A.nnz, K), flush=True)
    show("    symmetrize alone", wall_ms(ctx, lambda: [ctx.symmetrize(A, drop_diagonal=True)], args.reps))
    show("    baseline: download of the operand", wall_ms(ctx, lambda: (A.download(), [])[1], args.reps))
    ok, labels, res = True, {}, {}

    def run():
        P, res["info"] = ctx.label_propagation(A, K)
        return [P]

    for min_class in (0, 1, 2, 3):
        ctx.set_option("lp_min_class", min_class)
        ms = show("    label_propagation, LP_MIN_CLASS %d (whole call)" % min_class, wall_ms(ctx, run, args.reps))
        info = res["info"]
        print("      %d iterations, converged %d, %d communities, classes %s" %
              (info["iterations"], info["converged"], info["communities"], info["class_vertices"]), flush=True)
        if min_class == 0:
            whole = ms
        if args.check:
            P = ctx.label_propagation(A, K)[0]
            labels[min_class] = P.download()[1]
            P.free()
            same = np.array_equal(labels[min_class], labels[0])
            ok &= same
            print("      check against LP_MIN_CLASS 0: %s" % ("equal" if same else "DIFFERENT"), flush=True)
    ctx.set_option("lp_min_class", 0)
    stderr_of(lambda: ctx_timed.label_propagation(At, K)[0].free())      # warm-up: workspaces
    for ln in stderr_of(lambda: ctx_timed.label_propagation(At, K)[0].free()).splitlines():
        print("      parts: " + ln.strip(), flush=True)
        m = re.search(r"\+ (\d+) iterations ([0-9.]+) .*\+ read-backs ([0-9.]+)", ln)
        if m and int(m.group(1)):
            k = int(m.group(1))
            print("      per iteration: %.1f us in the kernels, %.1f us in its read-back" %
                  (1e3 * float(m.group(2)) / k, 1e3 * float(m.group(3)) / k), flush=True)

    def same(exp):
        info = res["info"]
        return np.array_equal(labels[0], exp[0]) and exp[1:] == (info["iterations"], info["converged"], info["changed"],
                                                                  info["communities"])

    ok &= host_baseline("numpy model", lambda: cdlp_ref.label_propagation(*A.download(), n, K), args.numpy_max, A.nnz, whole,
                        same if args.check else None, check_label="the numpy model")
    At.free()
    A.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20, 22])
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--powerlaw", type=int, default=1 << 20, help="vertices of the power-law graph (0: none)")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=40_000_000, help="largest nnz for the numpy host baseline")
    ap.add_argument("--check", action="store_true", help="compare the labels with the host model and between the classes")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    ctx_timed = timed_context("BSPGEMM_LP_TIMING")
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
