"""Every branch of bspgemm_pagerank that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of one call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with a zeroed info and a message; the same call, unarmed, on the same
context returns the model's bits; after freeing every handle and destroying the context the gate's live count and live bytes
are back where they were.

The variants: PULL with AT NULL on a non-canonical A (the call transposes twice: its transpose and the canonical A), PULL
with AT given, and PUSH (both on a canonical A: the workspace and the tile rows alone, two requests).

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp, grown once before
anything else), which after an out-of-memory answer drops the cache of freed results and asks again -- "a new request, which
may succeed", as include/bspgemm.h says of the hook.  The test accepts BSPGEMM_OK from an armed call only with the exact
ranks and with exactly one request more than a cold call makes, and from at most that one k.  The sweep ends within the
request count of a first unarmed run (plus the one k at which the hook no longer fires): a condition, not a loop until
something breaks (tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import pagerank_ref as P
from alloc_sweep import Case, L, Out, fields, filled, sweep

pytestmark = pytest.mark.gpu

VARIANTS = {
    # name: (graph, method, AT given, the fewest k that must end in ERR_ALLOC)
    "pull_at_null_untidy": ("untidy", P.PR_PULL, False, 7),    # the tile rows and two operands of three arrays each
    "pull_at_given": ("symmetric_rmat9", P.PR_PULL, True, 1),
    "push": ("symmetric_rmat9", P.PR_PUSH, False, 1),
}


def pagerank_case(variant):
    name, method, with_at, least = VARIANTS[variant]
    rp, ci, n = P.graph(name)

    def setup(env):
        return dict(A=env.upload(rp, ci, n), AT=env.upload(*P.transposed(rp, ci, n)[:2], n) if with_at else None)

    def call(env, inp):
        info = filled(bspgemm.PrInfo)
        fixed, rank = np.zeros(n, np.uint64), np.zeros(n, np.float64)
        st = L().bspgemm_pagerank(env.ctx, inp["A"], inp["AT"], method, 0.85, 20, 0.0, fixed.ctypes.data, rank.ctypes.data,
                                  C.byref(info))
        return Out(st, structs={"info": info}, arrays={"fixed": fixed, "rank": rank})

    def expect():
        exp = P.pagerank(rp, ci, n, 0.85, 20)
        return exp["fixed"], exp["rank"].view(np.uint64), exp["mass"], exp["delta"], exp["dangling"], 20

    def read(env, inp, out):
        return (out.arrays["fixed"], out.arrays["rank"].view(np.uint64)) + fields(
            out.structs["info"], ("mass", "delta", "dangling", "iterations"))

    return Case(variant, setup, call, read, expect, zeroed=("info",), cap=40, min_failed=least, max_retried=1, strict_requests=True)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_allocation_failure_of_the_call(variant):
    sweep(pagerank_case(variant))
