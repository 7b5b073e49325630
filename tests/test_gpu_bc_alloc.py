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
something breaks.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import bc_ref as B

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
NAME = "bspgemm_betweenness"
INFO = ("sigma_max", "reached", "edges_forward", "hub_chunks", "sources", "depth_max", "levels", "canonicalised")
VARIANTS = {
    # name: the fewest k that must end in ERR_ALLOC
    "rmat11": 1,
    "hub_chunks": 1,
    "untidy": 4,               # the tile rows and an operand of three arrays
}


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


class _Env:
    """one context with the graph uploaded"""

    def __init__(self, rp, ci, n, sources):
        L = bspgemm.lib()
        self.n, self.sources = n, np.ascontiguousarray(sources, np.int32)
        self.ctx, self.A = VP(), VP()
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        assert L.bspgemm_matrix_upload(self.ctx, n, n, rp.ctypes.data, ci.ctypes.data, C.byref(self.A)) == OK, _last_error()

    def call(self):
        """(status, fixed, bc, info)"""
        info = bspgemm.BcInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        fixed, bc = np.full(self.n, 77, np.uint64), np.full(self.n, -7.25)
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.A, self.sources.size, self.sources.ctypes.data, fixed.ctypes.data,
                                          bc.ctypes.data, C.byref(info))
        return st, fixed, bc, info

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_allocation_failure_of_the_call(variant):
    L = bspgemm.lib()
    least = VARIANTS[variant]
    rp, ci, n = B.graph(variant)
    sources = B.sources_of(variant)[:9]
    exp = B.model(rp, ci, n, sources)

    def exact(fixed, bc, info, what):
        assert np.array_equal(fixed, exp["fixed"]) and bc.tobytes() == exp["bc"].tobytes(), what
        assert all(getattr(info, k) == exp[k] for k in INFO), (what, info.as_dict())

    def good(env, what):
        st, fixed, bc, info = env.call()
        assert st == OK, "%s: status %d (%s)" % (what, st, _last_error())
        exact(fixed, bc, info, what)

    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L.bspgemm_debug_fail_alloc(0)
    base = bspgemm.debug_alloc_state()
    # a first unarmed run: its request count bounds the sweep
    env = _Env(rp, ci, n, sources)
    try:
        before = bspgemm.debug_alloc_state()
        good(env, "unarmed")
        cold = bspgemm.debug_alloc_state()[0] - before[0]
    finally:
        env.close()
    assert bspgemm.debug_alloc_state()[1:3] == base[1:3]
    assert 1 <= cold <= 40, cold
    failed, retried, fired = [], [], True
    for k in range(1, cold + 2):
        what = "%s k=%d" % (variant, k)
        env = _Env(rp, ci, n, sources)
        try:
            before = bspgemm.debug_alloc_state()
            L.bspgemm_debug_fail_alloc(k)
            st, fixed, bc, info = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert k == cold + 1, "%s: the hook is not reached, a cold call makes %d requests" % (what, cold)
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                exact(fixed, bc, info, what)
            else:
                assert fired == 1
                if st == OK:                         # (the documented retry: proven by its request count)
                    exact(fixed, bc, info, what + " armed")
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert bytes(info) == bytes(C.sizeof(info)) and _last_error(), what
                    assert (fixed == 77).all() and (bc == -7.25).all(), what + ": the outputs were written"
                    failed.append(k)
                good(env, what + " repeated")
        finally:
            L.bspgemm_debug_fail_alloc(0)
            env.close()
        now = bspgemm.debug_alloc_state()
        assert now[1:3] == base[1:3], "%s: leak: live (count, bytes) %r, before the context %r" % (what, now[1:3], base[1:3])
    assert not fired, "the hook still fires at k = %d, one past the %d requests of a cold call" % (cold + 1, cold)
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % (variant, cold, failed, retried))
    assert len(failed) + len(retried) == cold, (cold, failed, retried)                # every request of the call was failed once
    assert len(retried) <= 1 and len(failed) >= least, (failed, retried)
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
