#!/usr/bin/env python3
"""What the on-device set operations cost on an MI355X, beside the select and beside the only way to get a union, an
intersection or a difference without them: a product through an identity operand.
    python tools/setop_time.py [--scale 20] [--skew-scale 18] [--ef 16] [--reps 6] [--check]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).  Times are wall
times around whole calls that end synchronised, the new operand's allocation included; freeing it is outside.

Two matrices that the other measurements use: G = R-MAT --scale, edge factor 16, (0.30, 0.25, 0.25), seed 1 (bench.py's
generator), and the Graph500-skew R-MAT --skew-scale, (0.57, 0.19, 0.19), seed 1.  On each, with GT = transpose(G) and I the
identity:
    setop(G, GT, op) for the four ops, matrix_equal(G, G), symmetrize(G), matrix_select(G, tril)
    the baselines:  G | GT  = matrix_from_result(multiply_accumulate(I, GT, D = G))
                    G & GT  = matrix_from_result(multiply_masked(I, GT, F = G))
                    GT \\ G  = matrix_from_result(multiply_masked(I, GT, F = G, complement))   against setop(GT, G, andnot)
Entries touched, for the rate per entry: a setop reads nnz(A) + nnz(B) entries, the select nnz(G).  --check compares every
baseline's operand with the setop's, entry for entry, before anything is timed."""
import argparse
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import wall_ms
import numpy as np
import bspgemm


def show(name, ms, entries=None):
    return timing_common.show(name, ms, "  %7.2f G entries/s" % (entries / min(ms) / 1e6) if entries else "")


def measure(ctx, name, rp, ci, n, args):
    G = ctx.upload(rp, ci, n)
    GT = ctx.transpose(G)
    eye = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    both = G.nnz + GT.nnz
    print("%s: n = %d, nnz(G) = %d, nnz(GT) = %d, longest row %d" % (name, n, G.nnz, GT.nnz, int(np.diff(rp).max())), flush=True)

    def via_product(product):
        P = product()
        M = ctx.matrix_from_result(P, n)
        P.free()
        return M

    baselines = {
        "or": ("multiply_accumulate(I, GT, D = G) + matrix_from_result", G, GT,
               lambda: via_product(lambda: ctx.multiply_accumulate(eye, GT, G))),
        "and": ("multiply_masked(I, GT, F = G) + matrix_from_result", G, GT,
                lambda: via_product(lambda: ctx.multiply_masked(eye, GT, G))),
        "andnot": ("multiply_masked(I, GT, !G) + matrix_from_result", GT, G,
                   lambda: via_product(lambda: ctx.multiply_masked(eye, GT, G, complement=True))),
    }
    if args.check:
        for op, (_, x, y, base) in baselines.items():
            S, M = ctx.setop(x, y, op), base()
            same = S.nnz == M.nnz and all(np.array_equal(a, b) for a, b in zip(S.download(), M.download()))
            print("    check %-6s %s (%d entries)" % (op, "equal" if same else "DIFFERENT", S.nnz), flush=True)
            S.free()
            M.free()
            if not same:
                sys.exit(1)
    best = {}
    for op in ("or", "and", "andnot", "xor"):
        x, y = (GT, G) if op == "andnot" else (G, GT)
        label = "setop(GT, G, andnot)" if op == "andnot" else "setop(G, GT, %s)" % op
        best[op] = show(label, wall_ms(ctx, lambda: [ctx.setop(x, y, op)], args.reps), both)
    res = {}

    def equal():
        res["eq"] = ctx.matrix_equal(G, G)
        return []
    show("matrix_equal(G, G)", wall_ms(ctx, equal, args.reps), 2 * G.nnz)
    assert res["eq"]
    show("symmetrize(G)  (transpose + setop or)", wall_ms(ctx, lambda: [ctx.symmetrize(G)], args.reps))
    show("matrix_select(G, tril)", wall_ms(ctx, lambda: [ctx.select(G, "tril")], args.reps), G.nnz)
    for op, (label, _, _, base) in baselines.items():
        b = show("baseline %-6s %s" % (op, label), wall_ms(ctx, lambda: [base()], args.reps))
        print("    %-6s setop %.3f ms against %.3f ms: %s" % (op, best[op], b, "no slower" if best[op] <= b else "SLOWER"), flush=True)
    for h in (G, GT, eye):
        h.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--skew-scale", type=int, default=18)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--check", action="store_true", help="compare the baselines' operands with the setops' first")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    measure(ctx, "R-MAT %d, edge factor %d, (0.30, 0.25, 0.25)" % (args.scale, args.ef),
            *bspgemm.gen_rmat(args.scale, args.ef, (0.30, 0.25, 0.25), seed=1), args)
    measure(ctx, "Graph500-skew R-MAT %d, edge factor %d, (0.57, 0.19, 0.19)" % (args.skew_scale, args.ef),
            *bspgemm.gen_rmat(args.skew_scale, args.ef, (0.57, 0.19, 0.19), seed=1), args)
    ctx.close()


if __name__ == "__main__":
    main()
