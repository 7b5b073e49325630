#!/usr/bin/env python3
"""Cost of the OR-accumulating product C = D | (A*B) against the plain product, on the benchmark's matrix, and of the
transitive closure A+ on a Graph500-skew graph.
    python tools/accumulate_time.py [--scale 22] [--steps 20] [--cases plain,a,b,c,closure]
R-MAT scale 22, edge factor 16, (0.30, 0.25, 0.25), seed 1 (bench.py's default workload), A*A; one process, 20 timed
steps per case after one warm-up.  Cases: the plain product; the accumulating product with (a) an empty D, (b) D = A
(about 5 % more inserts than products), (c) D = pattern(A*A) (the closure step: twice the inserts).  GNZ/s counts nnz of
the plain product in every row, so that the rows compare.  Then the transitive closure (bspgemm_closure_ex,
BSPGEMM_CLOSURE_TRANSITIVE) of one Graph500-skew R-MAT graph of scale 16 and edge factor 1 (--closure-ef: the closure of
denser graphs of this skew is nearly dense in their giant component), timed once after one warm-up."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-spgemm_amd"))
import torch  # noqa: E402,F401  (first: one HIP runtime in the process)
import bspgemm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cases", default="plain,a,b,c,closure", help="comma-separated subset of plain,a,b,c,closure")
    ap.add_argument("--closure-scale", type=int, default=16)
    ap.add_argument("--closure-ef", type=int, default=1)
    args = ap.parse_args()
    keep = set(args.cases.split(","))
    ctx = bspgemm.Context(0)
    rp, ci, n = bspgemm.gen_rmat(args.scale, 16, (0.30, 0.25, 0.25), seed=1)
    A = ctx.upload(rp, ci, n)
    C = ctx.multiply(A, A)
    nnz_c = C.nnz
    products = ctx.stats()["products"]
    P = ctx.matrix_from_result(C, n)
    C.free()
    empty = ctx.upload([0] * (n + 1), [], n)
    print("R-MAT scale %d: nnz(A) %d, products %d, nnz(A*A) %d" % (args.scale, A.nnz, products, nnz_c))
    cases = [("plain A*A", "plain", lambda: ctx.multiply(A, A)),
             ("(a) empty D", "a", lambda: ctx.multiply_accumulate(A, A, empty)),
             ("(b) D = A", "b", lambda: ctx.multiply_accumulate(A, A, A)),
             ("(c) D = pattern(A*A)", "c", lambda: ctx.multiply_accumulate(A, A, P))]
    base = None
    print("%-24s %9s %8s %8s %12s %10s %10s" % ("case", "ms", "GNZ/s", "vs plain", "nnz(C)", "numeric", "stitch"))
    for name, key, fn in cases:
        if key not in keep:
            continue
        fn().free()
        t = time.perf_counter()
        for _ in range(args.steps):
            R = fn()
            nnz = R.nnz
            R.free()
        ms = (time.perf_counter() - t) / args.steps * 1e3
        st = ctx.stats()
        base = base or ms
        print("%-24s %9.3f %8.2f %7.1f%% %12d %10.3f %10.3f" % (name, ms, nnz_c / ms / 1e6, 100.0 * (ms / base - 1.0), nnz,
                                                              st["ms_numeric"], st["ms_stitch"]))
    for h in (A, P, empty):
        h.free()
    if "closure" in keep:
        grp, gci, gn = bspgemm.gen_rmat(args.closure_scale, args.closure_ef, (0.57, 0.19, 0.19), seed=1)
        G = ctx.upload(grp, gci, gn)
        for warm in (True, False):
            t = time.perf_counter()
            T, it = ctx.closure(G, transitive=True)
            ms = (time.perf_counter() - t) * 1e3
            nnz_t = T.nnz
            T.free()
        print("transitive closure, Graph500-skew scale %d, edge factor %d (nnz %d): %d products, nnz(A+) %d, %.1f ms"
              % (args.closure_scale, args.closure_ef, G.nnz, it, nnz_t, ms))
        G.free()
    ctx.close()


if __name__ == "__main__":
    main()
