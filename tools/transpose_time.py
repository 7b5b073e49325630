#!/usr/bin/env python3
"""Time of the operand transpose AT = pattern(A)^T (bspgemm_matrix_transpose) on two workloads.
    python tools/transpose_time.py [--steps 20] [--warmup 3] [--workloads mild22,g500s20] [--no-check]
  mild22   R-MAT scale 22, edge factor 16, (0.30, 0.25, 0.25), seed 1: bench.py's matrix
  g500s20  R-MAT scale 20, edge factor 16, Graph500 skew (0.57, 0.19, 0.19), seed 1: hub columns
Each call is timed by the host clock around the whole call, which ends in a device synchronise (the call's own read-back
of nnz(AT)); it includes AT's allocation.  The result is freed outside the timed region.  Rate by algorithmic bytes: read A
(4(rows+1) + 4 nnz(A)) plus write AT (4(cols+1) + 4 nnz(AT)); "of HBM peak" is that rate over 8.0 TB/s (spec; about
6.3 TB/s is reachable by a plain copy).  The last output of each workload is compared in full with a numpy transpose.
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -d DIR -o transpose --` with a few steps."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-spgemm_amd"))
import torch  # noqa: E402,F401  (first: one HIP runtime in the process)
import bspgemm  # noqa: E402

HBM_PEAK = 8.0e12
WORKLOADS = {"mild22": (22, (0.30, 0.25, 0.25)), "g500s20": (20, (0.57, 0.19, 0.19))}


def ref_transpose(rp, ci, cols):
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp.astype(np.int64)))
    key = np.unique((ci.astype(np.int64) << 32) | rows)
    k = key >> 32
    out = np.zeros(cols + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(k, minlength=cols))
    return out.astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="mild22,g500s20")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with numpy (e.g. under a profiler)")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    for name in args.workloads.split(","):
        scale, abc = WORKLOADS[name]
        rp, ci, n = bspgemm.gen_rmat(scale, 16, abc, seed=1)
        A = ctx.upload(rp, ci, n)
        for _ in range(args.warmup):
            ctx.transpose(A).free()
        ms = []
        AT = None
        for _ in range(args.steps):
            if AT is not None:
                AT.free()
            t0 = time.perf_counter()
            AT = ctx.transpose(A)
            ms.append((time.perf_counter() - t0) * 1e3)
        nbytes = 4 * (A.rows + 1) + 4 * A.nnz + 4 * (AT.rows + 1) + 4 * AT.nnz
        med = statistics.median(ms)
        row = {"workload": name, "scale": scale, "abc": abc, "nnz_a": int(A.nnz), "nnz_at": int(AT.nnz),
               "steps": args.steps, "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
               "bytes_alg": int(nbytes), "GBps_alg": round(nbytes / med / 1e6, 1),
               "frac_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
        if not args.no_check:
            grp, gci = AT.download()
            erp, eci = ref_transpose(rp, ci, n)
            row["matches_numpy"] = bool(np.array_equal(grp, erp) and np.array_equal(gci, eci))
        print(json.dumps(row), flush=True)
        AT.free()
        A.free()
        if row.get("matches_numpy") is False:
            sys.exit(1)
    ctx.close()


if __name__ == "__main__":
    main()
