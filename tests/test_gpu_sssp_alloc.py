"""Every branch of bspgemm_weights_hashed and of bspgemm_sssp that follows a failed device allocation, taken one at a time
through bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the
hook no longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *W == NULL (the weights) or a zeroed info and untouched
host arrays (the search) and a message; the same call, unarmed, on the same context returns the exact bits; after freeing
every handle and destroying the context the gate's live count and live bytes are back where they were.

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp), which after an
out-of-memory answer drops the cache of freed results and asks again.  Both calls grow the workspace first, so that is
k = 1: the armed call returns BSPGEMM_OK.  The test accepts BSPGEMM_OK from an armed call only with the exact bits and with
exactly one request more than a cold call makes, and from at most one k; every other k must end in BSPGEMM_ERR_ALLOC.

A cold bspgemm_weights_hashed makes 3 device allocations (what the sweep prints on an MI355X, ALLOCSWEEP): the workspace
(the sum's word), the tile rows of the entry-parallel launch and the weights themselves.  A cold bspgemm_sssp makes 2: the
workspace, which holds all of its state, and the tile rows of the column check and the parent pass.  A cold call that makes
more than twice that fails the test before the sweep (tests/alloc_sweep.py).
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import sssp_ref
from alloc_sweep import OK, VP, Case, L, Out, fields, filled, sweep

pytestmark = pytest.mark.gpu

COLD_HASHED, COLD_SSSP = 3, 2
SEED, WMIN, WMAX = 7, 1, 255


def _graph():
    g = sssp_ref.rmat(10, True)
    return g, np.ascontiguousarray(g.rp, np.int32), np.ascontiguousarray(g.ci, np.int32)


class _WeightsEnv:
    """the weights handles of a case's environment: freed before the context goes (Env.close knows operands and results)"""

    def __init__(self, env):
        self.env, self.made = env, []
        close = env.close

        def close_all():
            for w in self.made:
                L().bspgemm_weights_free(w)
            self.made = []
            close()
        env.close = close_all


def hashed_case():
    g, rp, ci = _graph()

    def setup(env):
        return dict(A=env.upload(rp, ci, g.n), weights=_WeightsEnv(env))

    def call(env, inp):
        W = VP(0x5A5A5A5A)
        st = L().bspgemm_weights_hashed(env.ctx, inp["A"], SEED, WMIN, WMAX, bspgemm.WEIGHTS_SYMMETRIC, C.byref(W))
        if st == OK and W.value:
            inp["weights"].made.append(W)
        return Out(st, scalars={"W": W})

    def read(env, inp, out):
        W = out.scalars["W"]
        w = np.zeros(g.ci.size, np.uint32)
        assert W.value and L().bspgemm_weights_download(env.ctx, W, w.ctypes.data) == OK
        return w, int(L().bspgemm_weights_sum(W)), int(L().bspgemm_weights_nnz(W))

    def expect():
        return g.w, int(g.w.sum(dtype=np.uint64)), int(g.ci.size)

    return Case("weights_hashed", setup, call, read, expect, failed={"W": None}, cap=2 * COLD_HASHED,
                min_failed=lambda cold: cold - 1, max_retried=1, strict_requests=True)


def sssp_case():
    g, rp, ci = _graph()
    names = sssp_ref.INFO

    def setup(env):
        A, keep = env.upload(rp, ci, g.n), _WeightsEnv(env)
        W = VP()
        assert L().bspgemm_weights_upload(env.ctx, A, g.w.ctypes.data, C.byref(W)) == OK
        keep.made.append(W)
        return dict(A=A, W=W, weights=keep)

    def call(env, inp):
        info = filled(bspgemm.SsspInfo)
        dist, parent = np.full(g.n, 9, np.uint64), np.full(g.n, 9, np.int32)
        st = L().bspgemm_sssp(env.ctx, inp["A"], inp["W"], g.source, None, dist.ctypes.data, parent.ctypes.data, C.byref(info))
        return Out(st, structs={"info": info}, arrays={"dist": dist, "parent": parent})

    def read(env, inp, out):
        return out.arrays["dist"], out.arrays["parent"], fields(out.structs["info"], names)

    def expect():
        m = sssp_ref.model_of(g)
        dist, parent = sssp_ref.reference_of(g)
        assert np.array_equal(m.dist, dist) and m.rounds > 3 and m.reached > g.n // 2
        return dist, parent, tuple(getattr(m, k) for k in names)

    return Case("sssp", setup, call, read, expect, zeroed=("info",), untouched={"dist": 9, "parent": 9}, cap=2 * COLD_SSSP,
                min_failed=lambda cold: cold - 1, max_retried=1, strict_requests=True)


@pytest.mark.parametrize("case", [hashed_case, sssp_case], ids=["weights_hashed", "sssp"])
def test_every_allocation_failure_of_the_call(case):
    sweep(case())
