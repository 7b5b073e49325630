#!/usr/bin/env python3
"""What the on-device select, the value sum, the triangle count and the k-truss loop cost on an MI355X.
    python tools/ktruss_time.py [--stream-scale 20] [--scale 20] [--ef 16] [--k 4] [--reps 10] [--kernels] [--skip-stream]
One process; every timed call is warmed up once and repeated --reps times (minimum and median printed).

(i)  The streaming primitives at size, beside the compaction in the same run.  G = R-MAT --stream-scale, edge factor 16,
     (0.30, 0.25, 0.25), seed 1 (bench.py's generator).  P = G*G is a plain multiply: its stitch phase (count scan +
     k_compact) moves 8 bytes per entry of P.  Fm = pattern(P) as an operand, C = Fm .* (G*G) with counts: a counted result
     of nnz(P) entries.  Timed with device events on the context's stream: bspgemm_matrix_from_result_where(C, >= 2),
     bspgemm_matrix_select(Fm, tril), bspgemm_result_values_sum(C).  Bytes of a select over E entries that keeps K, in
     W = E / 64 words and R rows:  pass 1 reads 4 E and writes 12 W;  the scan reads 4 W and writes 8 W;  pass 2 reads
     16 W and the 16-byte groups that keep an entry (at most min(4 E, 16 K)) and writes 4 K;  the row pass reads
     R row_ptr entries (4 or 8 bytes each) and writes 4 R.  The event bracket also holds the call's one synchronisation and
     the allocation of the new operand, so these are CALL rates; --kernels runs the same calls a few times without any
     timing, for a kernel trace taken in a run of its own.
(ii) One k-truss step on the symmetrised Graph500-skew R-MAT --scale, edge factor --ef: the counted product and the filter
     on the device, against the same step through the host (download the result and its values, filter in numpy, upload
     the new operand) -- the only way before the select existed.
(iii) bspgemm_ktruss(k) and bspgemm_triangle_count on that graph, wall time around calls that end synchronised."""
import argparse

import timing_common  # noqa: F401  (first: the paths, and torch before bspgemm)
from timing_common import wall_ms
import torch
import numpy as np
import bspgemm


def symmetrise(rp, ci, n):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    ci = ci.astype(np.int64)
    r, c = np.concatenate([rows, ci]), np.concatenate([ci, rows])
    key = np.unique((r[r != c] << 32) | c[r != c])
    counts = np.bincount(key >> 32, minlength=n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32)


def select_bytes(entries, kept, rows, row_ptr_bytes):
    words = -(-entries // 4096) * 64
    return (4 * entries + 12 * words + 12 * words + 16 * words + min(4 * entries, 16 * kept) + 4 * kept
            + (row_ptr_bytes + 4) * (rows + 1))


def event_ms(stream, fn, reps):
    """device-event time of fn() on `stream`, per repetition; fn returns a handle that is freed outside the bracket"""
    out = []
    fn().free()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h = fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
        if h is not None:
            h.free()
    return out


def show(name, ms, nbytes=None, extra=""):
    rate = "  %8.1f GB/s" % (nbytes / min(ms) / 1e6) if nbytes else ""
    timing_common.show(name, ms, rate + "  " + extra)


class _Freed:
    def free(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream-scale", type=int, default=20)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernels", action="store_true", help="only run the streaming calls, untimed (for a kernel trace)")
    ap.add_argument("--skip-stream", action="store_true", help="parts (ii) and (iii) only")
    args = ap.parse_args()
    ctx = bspgemm.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)

    if not args.skip_stream:
        streaming(ctx, stream, args)
    if not args.kernels:
        loops(ctx, args)
    ctx.close()


def streaming(ctx, stream, args):
    """(i) the streaming primitives at size"""
    rp, ci, n = bspgemm.gen_rmat(args.stream_scale, 16, (0.30, 0.25, 0.25), seed=1)
    G = ctx.upload(rp, ci, n)
    ctx.multiply(G, G).free()
    stitch = []
    for _ in range(3 if args.kernels else args.reps):
        P = ctx.multiply(G, G)
        st = ctx.stats()
        stitch.append(st["ms_stitch"])
        nnz_p = P.nnz
        P.free()
    P = ctx.multiply(G, G)
    Fm = ctx.matrix_from_result(P, n)
    P.free()
    Cc = ctx.multiply_masked_count(G, G, Fm)
    E = Cc.nnz
    if args.kernels:
        for _ in range(3):
            ctx.matrix_from_result_where(Cc, n, ">=", 2).free()
            ctx.select(Fm, "tril").free()
            Cc.values_sum()
        ctx.synchronize()
        print("kernels run: %d entries" % E)
        return
    print("(i) R-MAT %d, edge factor 16: nnz(G) = %d, nnz(G*G) = %d entries (%d tiles of 4096)" % (args.stream_scale, G.nnz, E, E // 4096))
    show("plain multiply, stitch phase (count scan + k_compact)", stitch, 8 * nnz_p, "8 B/entry")
    W = ctx.matrix_from_result_where(Cc, n, ">=", 2)
    kept_w = W.nnz
    W.free()
    show("matrix_from_result_where(C, >= 2)  kept %d" % kept_w,
         event_ms(stream, lambda: ctx.matrix_from_result_where(Cc, n, ">=", 2), args.reps), select_bytes(E, kept_w, n, 8))
    show("matrix_from_result_where(C, >= 1)  kept all",
         event_ms(stream, lambda: ctx.matrix_from_result_where(Cc, n, ">=", 1), args.reps), select_bytes(E, E, n, 8))
    S = ctx.select(Fm, "tril")
    kept_s = S.nnz
    S.free()
    show("matrix_select(pattern(G*G), tril)  kept %d" % kept_s,
         event_ms(stream, lambda: ctx.select(Fm, "tril"), args.reps), select_bytes(E, kept_s, n, 4))
    show("matrix_from_result(C)  (plain copy, for scale)",
         event_ms(stream, lambda: ctx.matrix_from_result(Cc, n), args.reps), 8 * E + 12 * (n + 1))

    def vsum():
        Cc.values_sum()
        return _Freed()
    show("result_values_sum(C)", event_ms(stream, vsum, args.reps), 4 * E)
    for h in (Cc, Fm, G):
        h.free()


def loops(ctx, args):
    """(ii) one k-truss step, (iii) the loops"""
    rp, ci, n = bspgemm.gen_rmat(args.scale, args.ef, (0.57, 0.19, 0.19), seed=1)
    s_rp, s_ci = symmetrise(rp, ci, n)
    A = ctx.upload(s_rp, s_ci, n)
    k = args.k
    print("(ii) symmetrised Graph500-skew R-MAT %d, edge factor %d: n = %d, nnz = %d, longest row %d; k = %d"
          % (args.scale, args.ef, n, A.nnz, int(np.diff(s_rp).max()), k))
    product_ms = []

    def step_device():
        Cc = ctx.multiply_masked_count(A, A, A)
        product_ms.append(ctx.stats()["ms_total"])
        ctx.matrix_from_result_where(Cc, n, ">=", k - 2).free()
        Cc.free()

    def step_host():
        Cc = ctx.multiply_masked_count(A, A, A)
        crp, cci = Cc.download()
        v = Cc.download_values()
        Cc.free()
        keep = v >= k - 2
        rows = np.repeat(np.arange(n), np.diff(crp))
        nrp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
        ctx.upload(nrp, cci[keep], n).free()

    dev = wall_ms(ctx, step_device, args.reps)
    show("one step, device-resident (counted product + select)", dev)
    show("    of which the counted product (stats ms_total)", product_ms[1:])
    show("one step through the host (download, numpy, upload)", wall_ms(ctx, step_host, max(2, args.reps // 3)))
    print("(iii)")
    res = {}

    def truss():
        T, it, conv = ctx.ktruss(A, k)
        res["truss"] = (T.nnz, it, conv)
        T.free()

    def triangles():
        res["tri"] = ctx.triangle_count(A)
    show("ktruss(k = %d)" % k, wall_ms(ctx, truss, max(2, args.reps // 3)))
    print("    truss nnz %d, %d counted products, converged %s" % res["truss"])
    show("triangle_count", wall_ms(ctx, triangles, args.reps))
    print("    triangles %d" % res["tri"])
    A.free()


if __name__ == "__main__":
    main()
