#!/usr/bin/env python3
"""Cost of the counting masked product C = F .* (A*B) with path counts against the masked and the plain product.
    python tools/masked_count_time.py [--scale 22] [--skew-scale 18] [--steps 20]
One process, 20 timed steps per case after one warm-up.  Cases:
  on the benchmark's matrix (R-MAT scale 22, edge factor 16, (0.30, 0.25, 0.25), seed 1 -- bench.py's workload):
    the plain product A*A, the masked product A .* (A*A), the counting product with F = A;
  the triangle count sum(L .* (L*L)) of the symmetrised graph, L its strictly lower triangle (built on the device);
  Graph500-skew (0.57, 0.19, 0.19, 0.05) scale 18: the masked and the counting product with F = A.
The last column is the counting product's time over the masked product's on the same matrix and mask."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-spgemm_amd"))
import torch  # noqa: E402  (first: one HIP runtime in the process)
import bspgemm  # noqa: E402


def lower_triangle(ctx, rp, ci, n):
    """L = strict lower triangle of A | A^T, sorted and duplicate-free, as a device operand"""
    rp_t = torch.from_numpy(rp.astype('int64')).cuda()
    ci_t = torch.from_numpy(ci.astype('int64')).cuda()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), rp_t.diff())
    hi, lo = torch.maximum(rows, ci_t), torch.minimum(rows, ci_t)
    keys = torch.unique(hi[hi != lo] * n + lo[hi != lo])
    del rows, hi, lo, ci_t
    r, c = keys // n, (keys % n).to(torch.int32)
    lrp = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    lrp[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    lrp32 = lrp.to(torch.int32)
    torch.cuda.synchronize()                     # (the library's stream does not wait for torch's)
    return ctx.wrap_device(n, n, int(keys.numel()), lrp32.data_ptr(), c.data_ptr(), keep=(lrp32, c))


def timed(ctx, fn, steps):
    fn().free()
    t = time.perf_counter()
    for _ in range(steps):
        R = fn()
        nnz = R.nnz
        R.free()
    ms = (time.perf_counter() - t) / steps * 1e3
    return ms, nnz, ctx.stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--skew-scale", type=int, default=18)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    print("%-44s %9s %12s %10s %10s %9s" % ("case", "ms", "nnz(C)", "numeric", "stitch", "vs masked"))

    def report(name, res, masked_ms=None):
        ms, nnz, st = res
        rel = "%8.2fx" % (ms / masked_ms) if masked_ms else ""
        print("%-44s %9.3f %12d %10.3f %10.3f %9s" % (name, ms, nnz, st["ms_numeric"], st["ms_stitch"], rel), flush=True)
        return ms

    rp, ci, n = bspgemm.gen_rmat(args.scale, 16, (0.30, 0.25, 0.25), seed=1)
    A = ctx.upload(rp, ci, n)
    tag = "R-MAT %d" % args.scale
    report("%s plain A*A" % tag, timed(ctx, lambda: ctx.multiply(A, A), args.steps))
    m = report("%s masked A .* (A*A)" % tag, timed(ctx, lambda: ctx.multiply_masked(A, A, A), args.steps))
    report("%s counting, F = A" % tag, timed(ctx, lambda: ctx.multiply_masked_count(A, A, A), args.steps), m)
    L = lower_triangle(ctx, rp, ci, n)
    m = report("%s masked L .* (L*L)" % tag, timed(ctx, lambda: ctx.multiply_masked(L, L, L), args.steps))
    report("%s triangles: counting L .* (L*L)" % tag, timed(ctx, lambda: ctx.multiply_masked_count(L, L, L), args.steps), m)
    R = ctx.multiply_masked_count(L, L, L)
    print("  triangles: %d (L: %d entries)" % (int(torch.from_numpy(R.download_values()).sum()), L.nnz))
    R.free()
    L.free()
    A.free()

    rp, ci, n = bspgemm.gen_rmat(args.skew_scale, 16, (0.57, 0.19, 0.19), seed=1)
    A = ctx.upload(rp, ci, n)
    tag = "G500-skew %d" % args.skew_scale
    m = report("%s masked A .* (A*A)" % tag, timed(ctx, lambda: ctx.multiply_masked(A, A, A), args.steps))
    res = timed(ctx, lambda: ctx.multiply_masked_count(A, A, A), args.steps)
    report("%s counting, F = A" % tag, res, m)
    st = res[2]
    print("  classes (rows per bin): %s" % st["rows_per_bin"])
    A.free()
    ctx.close()


if __name__ == "__main__":
    main()
