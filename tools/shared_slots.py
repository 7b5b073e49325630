#!/usr/bin/env python3
"""How many products of a bench.py workload sit in rows of few shared slots (CPU only, sampled rows).
    tools/shared_slots.py [--workload rmat|rmat-g500|uniform|powerlaw] [--scale S] [--rows 30000] [--seed 1]
A row of the product A*A has F products; its columns fall into 32-column level-0 slots.  e = F - (slots used) is what the
one-wave kernel compares with shared_max (csrc/wave_rows.inc, BSPGEMM_OPT_SHARED_SLOTS): e = 0 is a sparse row, a row with
0 < e <= shared_max is emitted from its columns alone, every other row builds its masks.  The tables are weighted by
products, over the sampled rows of the one-wave classes with 2 or more levels' worth of columns, and per class."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-spgemm_amd"))
import bspgemm  # noqa: E402

CHUNKS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32)      # csrc/kernels.hpp kWaveChunks

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="rmat", choices=("rmat", "rmat-g500", "uniform", "powerlaw"))
ap.add_argument("--scale", type=int, default=0)
ap.add_argument("--rows", type=int, default=30000)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
if args.workload == "rmat":
    rp, ci, n = bspgemm.gen_rmat(args.scale or 22, 16, (0.30, 0.25, 0.25), seed=1)
elif args.workload == "rmat-g500":
    rp, ci, n = bspgemm.gen_rmat(args.scale or 18, 16, (0.57, 0.19, 0.19), seed=1)
elif args.workload == "uniform":
    rp, ci, n = bspgemm.gen_uniform(1 << (args.scale or 18), 16, seed=1)
else:
    rp, ci, n = bspgemm.gen_powerlaw(1 << (args.scale or 20), 64, seed=1)
rp = np.asarray(rp, np.int64)
deg = np.diff(rp)
rng = np.random.default_rng(args.seed)
rows = rng.choice(n, size=min(args.rows, n), replace=False)
F, e, dup = [], [], []
for i in rows:
    src = ci[rp[i]:rp[i + 1]]
    f = int(deg[src].sum())
    if f == 0 or f > 64 * CHUNKS[-1]:
        continue                                                        # empty, or a heavy row: not this kernel
    c = np.concatenate([ci[rp[j]:rp[j + 1]] for j in src])
    F.append(f)
    e.append(f - np.unique(c >> 5).size)
    dup.append(f - np.unique(c).size)
F, e, dup = np.asarray(F, np.int64), np.asarray(e), np.asarray(dup)
tot = F.sum()
cls = np.searchsorted(64 * np.asarray(CHUNKS), F, side="left")
print("%s: n = %d, %d sampled one-wave rows, %d products" % (args.workload, n, F.size, tot))
print("products in duplicate-free rows        %5.1f %%" % (100.0 * F[dup == 0].sum() / tot))
print("products in sparse rows (e = 0)        %5.1f %%" % (100.0 * F[e == 0].sum() / tot))
for k in (1, 2, 4, 8, 16):
    print("products in rows with e <= %-2d          %5.1f %%" % (k, 100.0 * F[e <= k].sum() / tot))
print("mean e per row                         %5.2f" % e.mean())
print("\nchunks  rows   products %   sparse %   e<=4 %  e<=8 %  (of the class's rows)")
for b, ch in enumerate(CHUNKS):
    m = cls == b
    if m.any():
        print("%5d %6d %9.1f %9.1f %8.1f %7.1f" % (ch, m.sum(), 100.0 * F[m].sum() / tot, 100.0 * (e[m] == 0).mean(),
                                                   100.0 * (e[m] <= 4).mean(), 100.0 * (e[m] <= 8).mean()))
