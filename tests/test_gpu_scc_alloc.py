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
row-length bytes of P); the sweep stops with a failure at twice that, so a hook that never stops firing cannot loop.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import gen
import scc_ref

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
SENTINEL = 0x5A5A5A5A
COLD = 5
NAME = "bspgemm_strongly_connected_components"


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


class _Env:
    """one context with rmat10 uploaded"""

    def __init__(self, rp, ci, n):
        L = bspgemm.lib()
        self.ctx, self.A = VP(), VP()
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        assert L.bspgemm_matrix_upload(self.ctx, n, n, rp.ctypes.data, ci.ctypes.data, C.byref(self.A)) == OK, _last_error()

    def call(self):
        """(status, P, ncomponents, rounds, sweeps)"""
        P, count, rounds, sweeps = VP(SENTINEL), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.A, C.byref(P), C.byref(count), C.byref(rounds), C.byref(sweeps))
        return st, P, count.value, rounds.value, sweeps.value

    def labels(self, P, n):
        """P downloaded and freed"""
        L = bspgemm.lib()
        rp, label = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        assert L.bspgemm_matrix_nnz(P) == n
        assert L.bspgemm_matrix_download(self.ctx, P, rp.ctypes.data, label.ctypes.data) == OK, _last_error()
        L.bspgemm_matrix_free(P)
        return rp, label

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


def test_every_allocation_failure_of_the_call():
    L = bspgemm.lib()
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 5403)
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    e_label, e_count = scc_ref.labels(rp, ci, n)
    assert 1 < e_count < n

    def good(env, what):
        st, P, count, rounds, sweeps = env.call()
        assert st == OK and P.value not in (None, SENTINEL), "%s: status %d (%s)" % (what, st, _last_error())
        g_rp, g_label = env.labels(P, n)
        assert np.array_equal(g_rp, np.arange(n + 1)) and np.array_equal(g_label, e_label), what
        assert (count, rounds) == (e_count, 1) and sweeps >= 3, (what, count, rounds, sweeps)

    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L.bspgemm_debug_fail_alloc(0)
    base = bspgemm.debug_alloc_state()
    failed, retried, cold = [], [], None
    for k in range(1, 2 * COLD + 1):
        what = "k=%d" % k
        env = _Env(rp, ci, n)
        try:
            before = bspgemm.debug_alloc_state()
            L.bspgemm_debug_fail_alloc(k)
            st, P, count, rounds, sweeps = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                g_rp, g_label = env.labels(P, n)
                assert np.array_equal(g_label, e_label) and count == e_count
                cold = after[0] - before[0]
            else:
                assert fired == 1
                if st == OK:                         # (the workspace's documented retry: proven below by its request count)
                    g_rp, g_label = env.labels(P, n)
                    assert np.array_equal(g_rp, np.arange(n + 1)) and np.array_equal(g_label, e_label), what + " armed"
                    assert (count, rounds) == (e_count, 1), (what, count, rounds)
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert P.value is None, "%s armed: *P is %r after a failure, not NULL" % (what, P.value)
                    assert (count, rounds, sweeps) == (0, 0, 0) and _last_error(), what
                    failed.append(k)
                good(env, what + " repeated")
        finally:
            L.bspgemm_debug_fail_alloc(0)
            env.close()
        now = bspgemm.debug_alloc_state()
        assert now[1:3] == base[1:3], "%s: leak: live (count, bytes) %r, before the context %r" % (what, now[1:3], base[1:3])
        if not fired:
            break
    else:
        pytest.fail("the hook still fires at k = %d (twice the cold count)" % (2 * COLD))
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % ("strongly_connected_components", cold, failed, retried))
    assert failed, "no k ended in BSPGEMM_ERR_ALLOC"
    assert len(failed) >= cold - 1 and len(retried) <= 1, (failed, retried)
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
