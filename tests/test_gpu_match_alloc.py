"""Every branch of bspgemm_maximal_matching that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *P == NULL, a zeroed info and a message; the same call,
unarmed, on the same context returns the exact mates and counts; after freeing every handle and destroying the context the
gate's live count and live bytes are back where they were.

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp), which after an
out-of-memory answer drops the cache of freed results and asks again.  The call grows the workspace once, before anything
else, to what the symmetrize inside it and its own state take at most, so that is k = 1: the armed call returns BSPGEMM_OK.
The test accepts BSPGEMM_OK from an armed call only with the exact bits and with exactly one request more than a cold call
makes, and from at most one k; every other k must end in BSPGEMM_ERR_ALLOC.

A cold call makes 14 device allocations (what the sweep prints on an MI355X, ALLOCSWEEP): the workspace, the ten of
bspgemm_matrix_symmetrize, then P.row_ptr, P.col_idx and the row-length bytes of P -- the same as the colouring, whose state
the matching's replaces.  A cold call that makes more than twice that fails the test before the sweep
(tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
import match_ref
from alloc_sweep import OK, SENTINEL, VP, Case, L, Out, fields, filled, sweep

pytestmark = pytest.mark.gpu

COLD = 14
ORDER, SEED = 3, 11             # BSPGEMM_MATCH_LIGHT_FIRST
INFO = ("pairs", "entries_walked", "hub_chunks", "rounds", "lanes")


def match_case():
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 5403)
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)

    def call(env, inp):
        P, info, mate = VP(SENTINEL), filled(bspgemm.MatchInfo), np.full(n, -7, np.int32)
        st = L().bspgemm_maximal_matching(env.ctx, inp["A"], ORDER, SEED, C.byref(P), mate.ctypes.data, C.byref(info))
        if st == OK and P.value not in (None, SENTINEL):
            env.mat(P)
        return Out(st, {"P": ("m", P)}, structs={"info": info}, arrays={"mate": mate})

    def expect():
        r = match_ref.matching(rp, ci, n, "light", SEED)
        assert 2 < r.pairs < n // 2 and r.rounds > 1
        return np.arange(n + 1), r.labels, r.mate, (r.pairs, r.entries_walked, r.hub_chunks, r.rounds, r.lanes)

    def read(env, inp, out):
        return env.matrix(out.handles["P"][1]) + (out.arrays["mate"], fields(out.structs["info"], INFO))

    return Case("maximal_matching", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect, zeroed=("info",),
                cap=2 * COLD, min_failed=lambda cold: cold - 1, max_retried=1, strict_requests=True)


def test_every_allocation_failure_of_the_call():
    sweep(match_case())
