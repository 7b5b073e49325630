"""Times the prepass when A has long runs of empty rows, B being the bench matrix itself (R-MAT scale 22, edge factor 16,
(0.30,0.25,0.25,0.20), seed 1: the blocked extents table): A = the bench matrix with its second half of rows emptied (a
2.1 M-row empty tail), with its middle half emptied, and the bench matrix unchanged.  Median of 10 products after 2.
usage: python3 tools/empty_rows_time.py   (from the repository root)"""
import sys
sys.path.insert(0, "binary-spgemm_amd")
import numpy as np
import torch, bspgemm  # noqa: F401  (torch first: one HIP runtime)

ctx = bspgemm.Context(0)
rp, ci, n = bspgemm.gen_rmat(22, 16, (0.30, 0.25, 0.25), seed=1)
B = ctx.upload(rp, ci, n)


def emptied(lo, hi):
    """the bench matrix with rows [lo, hi) emptied"""
    lengths = np.diff(rp.astype(np.int64))
    keep = np.ones(n, dtype=bool)
    keep[lo:hi] = False
    lengths[~keep] = 0
    arp = np.zeros(n + 1, dtype=np.int64)
    arp[1:] = np.cumsum(lengths)
    aci = ci[np.repeat(keep, np.diff(rp.astype(np.int64)))]
    return arp.astype(np.int32), aci


cases = [("empty tail (rows n/2..n)", emptied(n // 2, n)), ("empty middle (rows n/4..3n/4)", emptied(n // 4, 3 * n // 4)),
         ("bench matrix", (rp, ci))]
for name, (arp, aci) in cases:
    A = ctx.upload(arp, aci, n)
    ts = []
    for r in range(12):
        C = ctx.multiply(A, B); st = ctx.stats(); nnz = C.nnz; C.free()
        if r >= 2: ts.append((st["ms_total"], st["ms_prepass"]))
    t = np.median(np.array(ts), axis=0)
    print("%-32s prepass_kernel %d  total %.3f ms  prepass %.3f ms  nnz(A) %d nnz(C) %d" % (name, st["prepass_kernel"], t[0], t[1],
          int(arp[-1]), nnz), flush=True)
    A.free()
B.free()
ctx.close()
