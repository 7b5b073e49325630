"""Every branch of bspgemm_matrix_extract that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of one call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *out = NULL, a zeroed info and a message; the same call,
unarmed, on the same context returns the model's bits; after freeing every handle and destroying the context the gate's live
count and live bytes are back where they were.

The variants: canonical (the workspace, the tile rows, the operand's three arrays), hub (the values workspace for the chunk
records too), untidy (the call canonicalises A: two transposes, whose operands it owns and frees) and fallback (an out row
beyond the workgroup sort: out goes through two transposes, and the first out is freed).

The requests for a context workspace cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook (ensure_tmp and ensure_tmpv; how
many a variant makes stands in VARIANTS): after an out-of-memory answer they drop the cache of freed results and ask again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The test accepts BSPGEMM_OK from an armed call only with the exact result and with
exactly one request more than a cold call makes.  The sweep ends within the request count of a first unarmed run (plus the
one k at which the hook no longer fires): a condition, not a loop until something breaks (tests/alloc_sweep.py).
"""
import numpy as np
import pytest

import bspgemm
import gen
import extract_ref as X
from alloc_sweep import Case, L, call_to_handle, fields, sweep

pytestmark = pytest.mark.gpu


def _canonical():
    rp, ci, n = gen.rmat(10, 8, (0.45, 0.22, 0.22, 0.11), seed=51)
    rng = np.random.default_rng(52)
    return rp, ci, n, n, rng.integers(0, n, 300).astype(np.int32), np.sort(rng.permutation(n)[:400]).astype(np.int32), 0


def _hub():
    return X.hub_case() + (0,)


def _untidy():
    rp, ci, n = gen.dups_unsorted(500, 6, seed=9)
    p = np.random.default_rng(53).permutation(n).astype(np.int32)
    return rp, ci, n, n, p, p, 1


def _fallback():
    rp, ci, rows, cols = X.sort_case(True)
    return rp, ci, rows, cols, None, np.arange(cols, dtype=np.int32)[::-1].copy(), 0


VARIANTS = {
    # name: (case, the fewest k that must end in ERR_ALLOC, the most requests for a workspace, each of which is retried:
    # the call's own (ensure_tmp, which covers the transposes of an untidy A), with hubs the values workspace for the
    # chunk records (ensure_tmpv, sized after read-back one), and in the fallback the transposes of `out`, should they need
    # more than the call's own)
    "canonical": (_canonical, 3, 1),
    "hub": (_hub, 3, 2),
    "untidy": (_untidy, 8, 1),
    "fallback": (_fallback, 8, 3),
}


def extract_case(variant):
    inputs, least, workspace_requests = VARIANTS[variant]
    rp, ci, rows, cols, I, J, canonicalised = inputs()

    def call(env, inp, out, info):
        return L().bspgemm_matrix_extract(env.ctx, inp["A"], 0 if I is None else I.size, None if I is None else I.ctypes.data,
                                          0 if J is None else J.size, None if J is None else J.ctypes.data, 0, out, info)

    def expect():
        exp = X.model(rp, ci, rows, cols, I, J)
        assert exp["canonicalised"] == canonicalised and (exp["sorted_by"] == 2) == (variant == "fallback")
        assert (exp["hub_chunks"] > 0) == (variant in ("hub", "fallback"))
        return (exp["rp"], exp["ci"]) + tuple(exp[k] for k in X.INFO)

    def read(env, inp, out):
        return env.matrix(out.handles["out"][1]) + fields(out.structs["info"], X.INFO)

    return Case(variant, lambda env: dict(A=env.upload(rp, ci, cols)),
                call_to_handle("m", "out", call, structs={"info": bspgemm.ExtractInfo}, sentinel=77), read, expect,
                zeroed=("info",), cap=40, min_failed=least, max_retried=workspace_requests, strict_requests=True)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_allocation_failure_of_the_call(variant):
    sweep(extract_case(variant))
