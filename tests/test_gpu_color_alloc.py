"""Every branch of bspgemm_graph_coloring that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *P == NULL and a message; the same call, unarmed, on the same
context returns the exact colours; after freeing every handle and destroying the context the gate's live count and live
bytes are back where they were.

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp), which after an
out-of-memory answer drops the cache of freed results and asks again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The call grows the workspace once, before anything else, to what the symmetrize inside
it and its own state take at most, so that is k = 1 on an MI355X: the armed call returns BSPGEMM_OK.  The test accepts
BSPGEMM_OK from an armed call only with the exact colours and with exactly one request more than a cold call makes (the
failed one, repeated), and from at most one k; every other k must end in BSPGEMM_ERR_ALLOC.

A cold call makes 14 device allocations (measured on an MI355X; the sweep prints it, ALLOCSWEEP): the workspace, the ten
of bspgemm_matrix_symmetrize (the tile rows of the context and three arrays each for the select's, the transpose's and the
union's operand), then P.row_ptr, P.col_idx and the row-length bytes of P.  A cold call that makes more than twice that
fails the test before the sweep (tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import color_ref
import gen
from alloc_sweep import OK, SENTINEL, VP, Case, L, Out, sweep

pytestmark = pytest.mark.gpu

COLD = 14
ORDER, SEED = 3, 11             # BSPGEMM_COLOR_LARGEST_FIRST


def color_case():
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 5403)
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)

    def call(env, inp):
        P, colors, rounds = VP(SENTINEL), C.c_int(-1), C.c_int(-1)
        st = L().bspgemm_graph_coloring(env.ctx, inp["A"], ORDER, SEED, C.byref(P), C.byref(colors), C.byref(rounds))
        if st == OK and P.value not in (None, SENTINEL):
            env.mat(P)
        return Out(st, {"P": ("m", P)}, {"ncolors": colors, "rounds": rounds})

    def expect():
        e_colour, e_colors, e_rounds = color_ref.coloring(rp, ci, n, "largest", SEED)
        assert 2 < e_colors < n and e_rounds > 1
        return np.arange(n + 1), e_colour, e_colors, e_rounds

    def read(env, inp, out):
        return env.matrix(out.handles["P"][1]) + (out.scalars["ncolors"].value, out.scalars["rounds"].value)

    return Case("graph_coloring", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect,
                failed={"ncolors": 0, "rounds": 0},
                cap=2 * COLD, min_failed=lambda cold: cold - 1, max_retried=1, strict_requests=True)


def test_every_allocation_failure_of_the_call():
    sweep(color_case())
