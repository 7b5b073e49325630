"""Every branch of bspgemm_local_clustering that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of one DIRECTED call fails, k = 1, 2, ... until the
hook no longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *counts == NULL, a zeroed info and a message; the same
call, unarmed, on the same context returns the exact counts, degrees and coefficients; after freeing every handle and
destroying the context the gate's live count and live bytes are back where they were.

The graph is K_70 with every edge stored one way, the other or both: the directed call builds A', its transpose, S, R and
T, writes the weight bytes and runs both intersection kernels (666 heavy entries at the default split).

Four requests cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp, grown once before
anything else to the most that any stage of the call takes) and the three buffers of the counted result (result_alloc: its
row_ptr, col_idx and values, the call's last three requests), which after an out-of-memory answer drop the cache of freed
results and ask again -- "a new request, which may succeed", as include/bspgemm.h says of the hook.  The test accepts
BSPGEMM_OK from an armed call only with the exact counts and with exactly one request more than a cold call makes (the
failed one, repeated), and from at most those four k; every other k must end in BSPGEMM_ERR_ALLOC: the operands A', A'^T, S,
R and T (three arrays each), the tile rows.  A cold call makes 32 requests (measured on an MI355X: the retries were k = 1, 30,
31 and 32).  The sweep prints the count (ALLOCSWEEP), and a cold call that makes more than CAP fails the test before it
(tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import lcc_ref
from alloc_sweep import OK, SENTINEL, VP, Case, L, Out, fields, filled, sweep

pytestmark = pytest.mark.gpu

CAP = 60
GRAPH = "k70_oriented"
INFO = ("triangles", "entries", "heavy_entries", "reciprocal")


def lcc_case():
    rp, ci, n = lcc_ref.GRAPHS[GRAPH]()
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)

    def call(env, inp):
        R, info = VP(SENTINEL), filled(bspgemm.LccInfo)
        d, lcc = np.zeros(n, np.int32), np.zeros(n, np.float64)
        st = L().bspgemm_local_clustering(env.ctx, inp["A"], bspgemm.LCC_DIRECTED, C.byref(R), d.ctypes.data, lcc.ctypes.data,
                                          C.byref(info))
        if st == OK and R.value not in (None, SENTINEL):
            env.res(R)
        return Out(st, {"counts": ("r", R)}, structs={"info": info}, arrays={"degree": d, "lcc": lcc})

    def expect():
        e_num, e_d, e_lcc, e_triangles, e_reciprocal = lcc_ref.local_clustering(rp, ci, n, True)
        e_heavy = lcc_ref.heavy_entries(rp, ci, n, lcc_ref.LIGHT_DEFAULT)
        assert e_reciprocal > 0 and 0 < e_heavy < lcc_ref.half_entries(rp, ci, n) and e_num.min() > 0
        return e_num, e_d, e_lcc.view(np.uint64), e_triangles, lcc_ref.half_entries(rp, ci, n), e_heavy, e_reciprocal

    def read(env, inp, out):
        counts = env.result(out.handles["counts"][1], values=True)[2]
        return (counts, out.arrays["degree"], out.arrays["lcc"].view(np.uint64)) + fields(out.structs["info"], INFO)

    return Case("local_clustering", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect, zeroed=("info",),
                cap=CAP, min_failed=15, max_retried=4, strict_requests=True)   # five operands of three arrays each cannot be retried


def test_every_allocation_failure_of_the_call():
    sweep(lcc_case())
