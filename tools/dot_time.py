#!/usr/bin/env python3
"""The masked dot product beside the counting product on an MI355X: triangle count, one k-truss step and the whole
k-truss under both methods, and the sweep of BSPGEMM_OPT_DOT_LIGHT.
    python tools/dot_time.py [--graphs g500-18,rmat-18,rmat-20] [--k 4] [--reps 6] [--light 4,8,16,32,64] [--log PATH]
One process; every timed call is warmed up once and repeated --reps times (minimum / median of the wall time around calls
that end synchronised).  The log goes to profiles/dot_time.log (and to stdout).

Graphs, all symmetrised (A | A^T without the diagonal, on the host):
    g500-18   Graph500-skew R-MAT scale 18, edge factor 16, (0.57, 0.19, 0.19), seed 1: the graph of DESIGN.md 4.10
    rmat-18   R-MAT scale 18, edge factor 16, (0.30, 0.25, 0.25), seed 1 (bench.py's generator)
    rmat-20   the same at scale 20
Per graph:
    triangle_count            method "product" (L .* (L*L), the counting product) and "dot" (masked_dot(L, L, L))
    one k-truss step          C = S .* (S*S) by multiply_masked_count / by multiply_masked_dot(S, S, S), each followed by
                              matrix_from_result_where(C, >= k - 2); of the dot step also the product call alone
    the whole k-truss         ktruss(k) under both methods
    T sweep                   the dot step's call alone and the dot triangle count under each --light value, with
                              info.entries / info.heavy_entries of the step
    check                     both methods give the same triangle count, the same step result (row_ptr, col_idx, values
                              compared on the host) and the same truss (nnz, iterations, converged)"""
import argparse
import os
import statistics
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import ROOT, wall_ms
import numpy as np
import bspgemm

GRAPHS = {"g500-18": (18, 16, (0.57, 0.19, 0.19)), "rmat-18": (18, 16, (0.30, 0.25, 0.25)), "rmat-20": (20, 16, (0.30, 0.25, 0.25))}


def symmetrise(rp, ci, n):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    ci = ci.astype(np.int64)
    r, c = np.concatenate([rows, ci]), np.concatenate([ci, rows])
    key = np.unique((r[r != c] << 32) | c[r != c])
    counts = np.bincount(key >> 32, minlength=n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)


class Log:
    def __init__(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self.f = open(path, "w")

    def __call__(self, text=""):
        print(text, flush=True)
        self.f.write(text + "\n")
        self.f.flush()


def show(log, name, ms, extra=""):
    log(timing_common.line(name, ms, "  " + extra))
    return min(ms)


def one_graph(ctx, log, name, args):
    scale, ef, abc = GRAPHS[name]
    rp, ci, n = bspgemm.gen_rmat(scale, ef, abc, seed=1)
    s_rp, s_ci = symmetrise(rp, ci, n)
    A = ctx.upload(s_rp, s_ci, n)
    k, reps = args.k, args.reps
    default = ctx.get_option("dot_light")
    log("== %s: symmetrised R-MAT scale %d, edge factor %d, %r: n = %d, nnz = %d, longest row %d; k = %d, dot_light = %d"
        % (name, scale, ef, abc, n, A.nnz, int(np.diff(s_rp).max()), k, default))
    res = {}

    def tri(method):
        def fn():
            res["tri-" + method] = ctx.triangle_count(A, method=method)
        return fn

    def step_product():
        Cc = ctx.multiply_masked_count(A, A, A)
        ctx.matrix_from_result_where(Cc, n, ">=", k - 2).free()
        Cc.free()

    def step_dot():
        Cc, info = ctx.multiply_masked_dot(A, A, A)
        res["info"] = info
        ctx.matrix_from_result_where(Cc, n, ">=", k - 2).free()
        Cc.free()

    def call_dot():
        Cc, info = ctx.multiply_masked_dot(A, A, A)
        res["info"] = info
        Cc.free()

    def truss(method):
        def fn():
            T, it, conv = ctx.ktruss(A, k, method=method)
            res["truss-" + method] = (T.nnz, it, conv)
            T.free()
        return fn

    tp = show(log, "triangle_count, product", wall_ms(ctx, tri("product"), reps))
    td = show(log, "triangle_count, dot", wall_ms(ctx, tri("dot"), reps))
    log("    triangles %d / %d; dot takes %.2f x the product's time" % (res["tri-product"], res["tri-dot"], td / tp))
    sp = show(log, "one step, product (counted product + select)", wall_ms(ctx, step_product, reps))
    sd = show(log, "one step, dot (masked dot + select)", wall_ms(ctx, step_dot, reps))
    show(log, "    of which the masked dot call", wall_ms(ctx, call_dot, reps))
    log("    mask entries %d, of them heavy %d, kept %d; dot takes %.2f x the product's time"
        % (res["info"]["entries"], res["info"]["heavy_entries"], res["info"]["kept"], sd / sp))
    kreps = max(2, reps // 3)
    kp = show(log, "ktruss(k = %d), product" % k, wall_ms(ctx, truss("product"), kreps))
    kd = show(log, "ktruss(k = %d), dot" % k, wall_ms(ctx, truss("dot"), kreps))
    log("    truss nnz %d, %d steps, converged %s / nnz %d, %d steps, converged %s; dot takes %.2f x the product's time"
        % (res["truss-product"] + res["truss-dot"] + (kd / kp,)))
    # the sweep of the light / heavy threshold
    try:
        for T in args.light:
            ctx.set_option("dot_light", T)
            ms = wall_ms(ctx, call_dot, reps)
            tms = wall_ms(ctx, tri("dot"), reps)
            log("dot_light %3d: masked dot call min %9.3f ms  median %9.3f ms  heavy %9d of %d | triangle_count, dot min %8.3f ms  median %8.3f ms"
                % (T, min(ms), statistics.median(ms), res["info"]["heavy_entries"], res["info"]["entries"], min(tms),
                   statistics.median(tms)))
    finally:
        ctx.set_option("dot_light", default)
    # both methods agree
    Cp = ctx.multiply_masked_count(A, A, A)
    Cd, _ = ctx.multiply_masked_dot(A, A, A)
    p, d = Cp.download() + (Cp.download_values(),), Cd.download() + (Cd.download_values(),)
    same_step = all(np.array_equal(x, y) for x, y in zip(p, d))
    Cp.free()
    Cd.free()
    ok = same_step and res["tri-product"] == res["tri-dot"] and res["truss-product"] == res["truss-dot"]
    log("check: step results equal %s, triangle counts equal %s, trusses equal %s -> %s"
        % (same_step, res["tri-product"] == res["tri-dot"], res["truss-product"] == res["truss-dot"], "OK" if ok else "MISMATCH"))
    A.free()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="g500-18,rmat-18,rmat-20")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--light", default="4,8,16,32,64")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "dot_time.log"))
    args = ap.parse_args()
    args.light = [int(x) for x in args.light.split(",") if x]
    log = Log(args.log)
    log("tools/dot_time.py --graphs %s --k %d --reps %d --light %s" % (args.graphs, args.k, args.reps, ",".join(map(str, args.light))))
    ctx = bspgemm.Context(0)
    ok = True
    for name in args.graphs.split(","):
        ok = one_graph(ctx, log, name, args) and ok
        log()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
