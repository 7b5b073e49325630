#!/usr/bin/env python3
"""Per-class yardstick of the one-wave numeric kernel (csrc/wave_rows.inc): every capacity class alone on ONE stream.
    tools/class_time.py [--workload rmat|rmat-g500|uniform|powerlaw] [--scale S] [--reps 8] [--streams 1]
                        [--shared-slots K] [--kres FILE | --no-kres] [--save-kres FILE]
The class launches run back to back on one stream (option class_streams = 1) with an event pair around each
(bspgemm_set_class_timing), so a class's time is its own and not what it shares with its neighbour; the figure is the
MEDIAN over --reps multiplies, with min and max beside it (the class's own run-to-run spread).  Products per class come
from the host (row_work_prefix and the class bounds of bspgemm_stats), ps / product = ms / products.
The last columns are the resources of the instance that ran, from tools/kres.py (hipcc's kernel-resource-usage remarks
for the LEVELS and top-bitmap size this matrix takes): VGPRs, scratch bytes per lane, LDS bytes per workgroup, occ = the
resident waves per SIMD (the compiler's figure: registers and LDS together), byVGPR = what the registers alone allow
(512 per SIMD, granules of 8, at most 8 waves) and WG/CU = the workgroups that fit a CU's 160 KB of LDS.
--kres FILE reads a saved tools/kres.py table instead of compiling (the compile takes minutes); --save-kres writes one."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "binary-spgemm_amd")
sys.path.insert(0, PKG)

LDS_PER_CU = 160 * 1024


def levels_and_twp(n):
    """csrc/kernels.hpp wave_levels_for_cols and wave_rows.inc launch_one: LEVELS and top-bitmap words per lane"""
    levels = next((L for L in range(1, 5) if n <= (256 << (5 * L))), 5)
    if levels == 4 and n <= (512 << 15):
        levels = 3
    topw = -(-n // (1 << (5 * levels)))
    return levels, (2 if topw <= 128 else (4 if topw <= 256 else 8))


def kres_table(levels):
    """tools/kres.py on the MODE None object of `levels` (a one-line source that includes wave_rows.inc)"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "wave_rows_kres.hip")
        with open(src, "w") as f:
            f.write('#include "wave_rows.inc"\n')
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), src, "-I" + os.path.join(PKG, "csrc"),
                               "-DBSP_WAVE_LEVELS=%d" % levels, "-DBSP_WAVE_MODE=None"], cwd=PKG, capture_output=True,
                              text=True, check=True).stdout


def parse_kres(text, levels, twp):
    """{chunks: (vgpr, scratch, lds, occ)} of the emitting (COUNT = false) instances of (levels, twp)"""
    out = {}
    for line in text.splitlines():
        m = re.search(r"k_wave_rows<(\d+), (\d+), (\d+), \(bsp::MaskMode\)(\d+), (false|true)>\s+(.*)", line)
        if not m or (int(m.group(1)), int(m.group(3)), m.group(5)) != (levels, twp, "false"):
            continue
        f = m.group(6).split()                                     # SGPR VGPR AGPR occ LDS scratch
        out[int(m.group(2))] = (int(f[1]) + int(f[2]), int(f[5]), int(f[4]), int(f[3]))     # (AGPRs: spilled VGPRs, one file)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="rmat", choices=("rmat", "rmat-g500", "uniform", "powerlaw"))
    ap.add_argument("--scale", type=int, default=0)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--shared-slots", type=int, default=None, help="BSPGEMM_OPT_SHARED_SLOTS for the run (default: the library's)")
    ap.add_argument("--kres", help="a saved tools/kres.py table of wave_rows.inc")
    ap.add_argument("--save-kres", help="write the tools/kres.py table here")
    ap.add_argument("--no-kres", action="store_true")
    args = ap.parse_args()

    import bspgemm
    if args.workload == "rmat":
        rp, ci, n = bspgemm.gen_rmat(args.scale or 22, 16, (0.30, 0.25, 0.25), seed=1)
    elif args.workload == "rmat-g500":
        rp, ci, n = bspgemm.gen_rmat(args.scale or 18, 16, (0.57, 0.19, 0.19), seed=1)
    elif args.workload == "uniform":
        rp, ci, n = bspgemm.gen_uniform(1 << (args.scale or 18), 16, seed=1)
    else:
        rp, ci, n = bspgemm.gen_powerlaw(1 << (args.scale or 20), 64, seed=1)
    levels, twp = levels_and_twp(n)

    res = {}
    if not args.no_kres:
        if args.kres:
            with open(args.kres) as f:
                text = f.read()
        else:
            text = kres_table(levels)
        if args.save_kres:
            with open(args.save_kres, "w") as f:
                f.write(text)
        res = parse_kres(text, levels, twp)

    ctx = bspgemm.Context(0)
    ctx.set_option("class_streams", args.streams)
    if args.shared_slots is not None:
        ctx.set_option("shared_slots", args.shared_slots)
    ctx.set_class_timing(True)
    A = ctx.upload(rp, ci, n)
    F_row = np.diff(np.asarray(ctx.row_work_prefix(A, A), np.int64))
    ms, numeric = [], []
    for i in range(args.reps + 2):                                 # two warm-up multiplies
        C = ctx.multiply(A, A)
        C.free()
        st = ctx.stats()
        if i >= 2:
            ms.append(st["ms_bin"])
            numeric.append(st["ms_numeric"])
    ms = np.asarray(ms, np.float64)
    caps = st["bin_cap"]
    cls = np.zeros(F_row.shape, np.int64)
    cls[F_row > 0] = 1
    for k in range(1, len(caps) - 1):
        cls[F_row > caps[k]] = k + 1

    print("%s scale %s: n = %d, LEVELS = %d, top words per lane = %d, class_streams = %d, shared_slots = %d, %d multiplies"
          % (args.workload, args.scale or "default", n, levels, twp, st["class_streams"], ctx.get_option("shared_slots"), args.reps))
    print("numeric phase %.3f ms (median; min %.3f, max %.3f)" % (np.median(numeric), min(numeric), max(numeric)))
    print("%6s %9s %12s %8s %8s %8s %8s | %5s %7s %7s %4s %7s %7s" % ("chunks", "rows", "products", "ms", "min", "max", "ps/prod",
                                                                  "VGPR", "scratch", "LDS", "occ", "byVGPR", "WG/CU"))
    tot_ms = tot_p = 0.0
    for b in range(1, len(caps)):
        if caps[b] > 2048 or not (cls == b).any():
            continue
        ch = caps[b] // 64
        p = int(F_row[cls == b].sum())
        t = float(np.median(ms[:, b]))
        tot_ms += t
        tot_p += p
        line = "%6d %9d %12d %8.4f %8.4f %8.4f %8.2f |" % (ch, int((cls == b).sum()), p, t, ms[:, b].min(), ms[:, b].max(), t * 1e9 / p)
        if ch in res:
            vgpr, scratch, lds, occ = res[ch]
            line += " %5d %7d %7d %4d %7d %7d" % (vgpr, scratch, lds, occ, min(8, 512 // ((vgpr + 7) & ~7)), LDS_PER_CU // lds)
        print(line)
    print("%6s %9s %12d %8.4f %26.2f |" % ("sum", "", tot_p, tot_ms, tot_ms * 1e9 / tot_p))
    ctx.close()


if __name__ == "__main__":
    main()
