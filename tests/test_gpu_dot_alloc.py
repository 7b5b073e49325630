"""Every branch of bspgemm_multiply_masked_dot that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  The three operands are NOT canonical (A holds repeats, B's rows are unsorted, F both), so the call also
runs its canonicalising branch: three pairs of transposes, each with its operands and workspace, then the passes again.

An armed call returns BSPGEMM_ERR_ALLOC with *C == NULL, a zeroed info and a message; or, where the request that failed
belongs to the context's workspace (ensure_tmp) or to the result's buffers (result_alloc), which after an out-of-memory
answer drop the cache of freed results and ask again -- "a new request, which may succeed", as include/bspgemm.h says of
the hook -- BSPGEMM_OK with the exact result and exactly one request more than a cold call makes (the failed one,
repeated).  The same call, unarmed, on the same context returns the exact result; after freeing every handle and
destroying the context the gate's live count and live bytes are back where they were.

The sweep prints the cold call's allocation count (ALLOCSWEEP), and a cold call that makes more than CAP fails the test
before it (tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import dot_ref
from alloc_sweep import OK, SENTINEL, VP, Case, L, Out, fields, sweep

pytestmark = pytest.mark.gpu

CAP = 96
N, M, COLS = 400, 300, 150


def _inputs():
    rng = np.random.default_rng(8801)

    def rows(n, ncols, lo, hi, repeats, shuffle):
        out = []
        for k in rng.integers(lo, hi, n):
            r = np.sort(rng.choice(ncols, size=int(k), replace=False)).tolist()
            if repeats:
                r = sorted(r + [r[int(q)] for q in rng.integers(0, len(r), 2)])
            if shuffle:
                r = [r[int(q)] for q in rng.permutation(len(r))]
            out.append(r)
        return dot_ref.csr(out)

    return rows(N, COLS, 2, 80, True, False), rows(M, COLS, 2, 80, False, True), rows(N, M, 8, 20, True, True)


def dot_case():
    a, b, f = _inputs()

    def call(env, inp):
        r, info = VP(SENTINEL), bspgemm.DotInfo(7, 7, 7, 7)
        st = L().bspgemm_multiply_masked_dot(env.ctx, inp["A"], inp["B"], inp["F"], 0, C.byref(r), C.byref(info))
        if st == OK and r.value not in (None, SENTINEL):
            env.res(r)
        return Out(st, {"C": ("r", r)}, structs={"info": info})

    def expect():
        exp = dot_ref.dot_ref(a, b, f, N, M, COLS, M)
        entries = dot_ref.heavy_at_zero(a, b, f, N, M, COLS, M)[1]
        assert exp[1].size > 1000 and f[1].size > entries > 4096
        return tuple(exp) + (7, entries, exp[1].size)

    def read(env, inp, out):
        return env.result(out.handles["C"][1], values=True) + fields(out.structs["info"], ("canonicalised", "entries", "kept"))

    # zeroed: entries, heavy_entries, kept and canonicalised are all of bspgemm_dot_info
    return Case("multiply_masked_dot", lambda env: dict(A=env.upload(*a, COLS), B=env.upload(*b, COLS), F=env.upload(*f, M)),
                call, read, expect, zeroed=("info",),
                cap=CAP, min_failed=18, strict_requests=True)   # the six transposes' operands (three arrays each) cannot be retried


def test_every_allocation_failure_of_the_call():
    sweep(dot_case())
