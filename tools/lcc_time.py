#!/usr/bin/env python3
"""bspgemm_local_clustering on an MI355X beside the only route there was before it, the stage split, and the two halves.
    python tools/lcc_time.py [--graphs g500-18,rmat-18,rmat-20] [--reps 6] [--log PATH]
One process; every timed call is warmed up once and repeated --reps times (minimum / median of the wall time around calls
that end synchronised).  The log goes to profiles/lcc_time.log (and to stdout).

Graphs (tools/dot_time.py's three, here as generated: directed, so that both modes have something to tell apart):
    g500-18   Graph500-skew R-MAT scale 18, edge factor 16, (0.57, 0.19, 0.19), seed 1
    rmat-18   R-MAT scale 18, edge factor 16, (0.30, 0.25, 0.25), seed 1 (bench.py's generator)
    rmat-20   the same at scale 20
Per graph:
    the whole call            local_clustering undirected and directed: counts on the device, degrees and coefficients on the host
    the route before          symmetrize, then S .* (S * S) by multiply_masked_count / by multiply_masked_dot(S, S, S), the
                              download of row_ptr and values, numpy add.reduceat
    the stage split           a context created under BSPGEMM_LCC_TIMING=1: the library's own line (symmetrize and select,
                              weights, count, heavy, finish), the run with the smallest total of --reps
    TRIL against TRIU         the same under BSPGEMM_LCC_TIMING=2, which walks the half the library does not keep
    check                     the counts of the call, of both routes before and of both halves are equal"""
import argparse
import os
import re
import sys

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import ROOT, stderr_of, timed_context, wall_ms
import numpy as np
import bspgemm

GRAPHS = {"g500-18": (18, 16, (0.57, 0.19, 0.19)), "rmat-18": (18, 16, (0.30, 0.25, 0.25)), "rmat-20": (20, 16, (0.30, 0.25, 0.25))}


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


def stage_split(log, mode, rp, ci, n, reps):
    """the library's own stage lines under BSPGEMM_LCC_TIMING=mode, the best of reps per direction; returns the counts"""
    ctx = timed_context("BSPGEMM_LCC_TIMING", str(mode))
    A = ctx.upload(rp, ci, n)
    out = {}
    for directed in (False, True):
        def run():
            R, _, _, _ = ctx.local_clustering(A, directed)
            out[directed] = R.download_values()
            R.free()
        lines = [x for x in stderr_of(lambda: [run() for _ in range(reps + 1)]).split("\n") if "bspgemm_local_clustering" in x][1:]
        best = min(lines, key=lambda x: float(re.search(r"total ([0-9.]+) ms", x).group(1)))
        log("    " + best.strip())
    A.free()
    ctx.close()
    return out


def one_graph(ctx, log, name, args):
    scale, ef, abc = GRAPHS[name]
    rp, ci, n = bspgemm.gen_rmat(scale, ef, abc, seed=1)
    A = ctx.upload(rp, ci, n)
    reps = args.reps
    res = {}

    def call(directed):
        def fn():
            R, d, lcc, info = ctx.local_clustering(A, directed)
            res["info", directed], res["d"], res["lcc", directed] = info, d, lcc
            R.free()
        return fn

    def route(product):
        def fn():
            S = ctx.symmetrize(A, drop_diagonal=True)
            C = ctx.multiply_masked_count(S, S, S) if product else ctx.multiply_masked_dot(S, S, S)[0]
            c_rp, _ = C.download(col_idx=False)
            vals = C.download_values().astype(np.int64)
            num = np.zeros(n, np.int64)
            rows = np.flatnonzero(np.diff(c_rp))
            if vals.size:
                num[rows] = np.add.reduceat(vals, c_rp[rows])
            res["route", product] = num
            C.free()
            S.free()
        return fn

    log("== %s: R-MAT scale %d, edge factor %d, %r, as generated (directed): n = %d, nnz = %d; dot_light = %d"
        % (name, scale, ef, abc, n, A.nnz, ctx.get_option("dot_light")))
    tu = show(log, "local_clustering, undirected (the whole call)", wall_ms(ctx, call(False), reps))
    td = show(log, "local_clustering, directed (the whole call)", wall_ms(ctx, call(True), reps))
    iu, idr = res["info", False], res["info", True]
    log("    triangles %d, entries of T %d, heavy %d, reciprocal %d; max degree %d, mean lcc %.6f undirected, %.6f directed"
        % (iu["triangles"], iu["entries"], iu["heavy_entries"], idr["reciprocal"], int(res["d"].max()), res["lcc", False].mean(),
           res["lcc", True].mean()))
    tp = show(log, "before: symmetrize + masked_count(S, S, S) + download + reduceat", wall_ms(ctx, route(True), reps))
    tdot = show(log, "before: symmetrize + masked_dot(S, S, S) + download + reduceat", wall_ms(ctx, route(False), reps))
    log("    the undirected call takes %.2f x the counted product's route, %.2f x the masked dot's; directed / undirected %.2f"
        % (tu / tp, tu / tdot, td / tu))
    R, _, _, _ = ctx.local_clustering(A)
    num = R.download_values().astype(np.int64)
    R.free()
    A.free()
    log("stage split, TRIL (BSPGEMM_LCC_TIMING=1; every stage synchronised):")
    lower = stage_split(log, 1, rp, ci, n, reps)
    log("stage split, TRIU (BSPGEMM_LCC_TIMING=2):")
    upper = stage_split(log, 2, rp, ci, n, reps)
    same_routes = np.array_equal(num, res["route", True]) and np.array_equal(num, res["route", False])
    same_halves = np.array_equal(lower[False], upper[False]) and np.array_equal(lower[True], upper[True]) and np.array_equal(lower[False], num)
    ok = same_routes and same_halves and int(num.sum()) == 6 * iu["triangles"]
    log("check: counts equal those of both routes before %s, both halves give equal counts %s, sum = 6 triangles %s -> %s"
        % (same_routes, same_halves, int(num.sum()) == 6 * iu["triangles"], "OK" if ok else "MISMATCH"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="g500-18,rmat-18,rmat-20")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "lcc_time.log"))
    args = ap.parse_args()
    log = Log(args.log)
    log("tools/lcc_time.py --graphs %s --reps %d" % (args.graphs, args.reps))
    ctx = bspgemm.Context(0)
    ok = True
    for name in args.graphs.split(","):
        ok = one_graph(ctx, log, name, args) and ok
        log()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
