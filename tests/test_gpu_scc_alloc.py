"""Every branch of bspgemm_strongly_connected_components that follows a failed device allocation, taken one at a time
through bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the
hook no longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *P == NULL and a message; the same call, unarmed, on
the same context returns the exact labels; after freeing every handle and destroying the context the gate's live count
and live bytes are back where they were.

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp), which after an
out-of-memory answer drops the cache of freed results and asks again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  On an MI355X that is k = 2: the armed call returns BSPGEMM_OK.  The test accepts
BSPGEMM_OK from an armed call only with the exact labels and with exactly one request more than a cold call makes (the
failed one, repeated), and from at most one k; every other k must end in BSPGEMM_ERR_ALLOC.

A cold call makes five device allocations (the tile rows and the workspace of the context, P.row_ptr, P.col_idx and the
row-length bytes of P); a cold call that makes more than twice that fails the test before the sweep (tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import gen
import scc_ref
from alloc_sweep import OK, SENTINEL, VP, Case, L, Out, sweep

pytestmark = pytest.mark.gpu

COLD = 5


def scc_case():
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 5403)
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)

    def call(env, inp):
        P, count, rounds, sweeps = VP(SENTINEL), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        st = L().bspgemm_strongly_connected_components(env.ctx, inp["A"], C.byref(P), C.byref(count), C.byref(rounds),
                                                       C.byref(sweeps))
        if st == OK and P.value not in (None, SENTINEL):
            env.mat(P)
        return Out(st, {"P": ("m", P)}, {"ncomponents": count, "rounds": rounds, "sweeps": sweeps})

    def expect():
        e_label, e_count = scc_ref.labels(rp, ci, n)
        assert 1 < e_count < n
        return np.arange(n + 1), e_label, e_count, 1

    def read(env, inp, out):
        assert out.scalars["sweeps"].value >= 3
        return env.matrix(out.handles["P"][1]) + (out.scalars["ncomponents"].value, out.scalars["rounds"].value)

    return Case("strongly_connected_components", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect,
                failed={"ncomponents": 0, "rounds": 0, "sweeps": 0},
                cap=2 * COLD, min_failed=lambda cold: cold - 1, max_retried=1, strict_requests=True)


def test_every_allocation_failure_of_the_call():
    sweep(scc_case())
