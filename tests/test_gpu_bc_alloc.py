"""Every branch of bspgemm_betweenness that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of one call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with a zeroed info, untouched outputs and a message; the same call,
unarmed, on the same context returns the model's bits; after freeing every handle and destroying the context the gate's live
count and live bytes are back where they were.

The variants: rmat11 and hub_chunks (canonical operands: the workspace and the tile rows alone) and untidy (the call
canonicalises A: two transposes, whose operands it owns and frees).

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp, grown once before
anything else), which after an out-of-memory answer drops the cache of freed results and asks again -- "a new request, which
may succeed", as include/bspgemm.h says of the hook.  The test accepts BSPGEMM_OK from an armed call only with the exact
sums and with exactly one request more than a cold call makes, and from at most that one k.  The sweep ends within the
request count of a first unarmed run (plus the one k at which the hook no longer fires): a condition, not a loop until
something breaks (tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import bc_ref as B
from alloc_sweep import Case, L, Out, fields, filled, sweep

pytestmark = pytest.mark.gpu

INFO = ("sigma_max", "reached", "edges_forward", "hub_chunks", "sources", "depth_max", "levels", "canonicalised")
VARIANTS = {
    # name: the fewest k that must end in ERR_ALLOC
    "rmat11": 1,
    "hub_chunks": 1,
    "untidy": 4,               # the tile rows and an operand of three arrays
}


def bc_case(variant):
    rp, ci, n = B.graph(variant)
    sources = np.ascontiguousarray(B.sources_of(variant)[:9], np.int32)

    def call(env, inp):
        info = filled(bspgemm.BcInfo)
        fixed, bc = np.full(n, 77, np.uint64), np.full(n, -7.25)
        st = L().bspgemm_betweenness(env.ctx, inp["A"], sources.size, sources.ctypes.data, fixed.ctypes.data, bc.ctypes.data,
                                     C.byref(info))
        return Out(st, structs={"info": info}, arrays={"fixed": fixed, "bc": bc})

    def expect():
        exp = B.model(rp, ci, n, sources)
        return (exp["fixed"], exp["bc"].view(np.uint64)) + tuple(exp[k] for k in INFO)

    def read(env, inp, out):
        return (out.arrays["fixed"], out.arrays["bc"].view(np.uint64)) + fields(out.structs["info"], INFO)

    return Case(variant, lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect, zeroed=("info",),
                untouched={"fixed": 77, "bc": -7.25}, cap=40, min_failed=VARIANTS[variant], max_retried=1, strict_requests=True)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_allocation_failure_of_the_call(variant):
    sweep(bc_case(variant))
