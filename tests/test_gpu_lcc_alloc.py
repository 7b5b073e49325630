"""Every branch of bspgemm_local_clustering that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of one DIRECTED call fails, k = 1, 2, ... until the
hook no longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *counts == NULL, a zeroed info and a message; the same
call, unarmed, on the same context returns the exact counts, degrees and coefficients; after freeing every handle and
destroying the context the gate's live count and live bytes are back where they were.

The graph is K_70 with every edge stored one way, the other or both: the directed call builds A', its transpose, S, R and
T, writes the weight bytes and runs both intersection kernels (666 heavy entries at the default split).

Four requests cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp, grown once before
anything else to the most that any stage of the call takes) and the three buffers of the counted result (result_alloc: its
row_ptr, col_idx and values, the call's last three requests), which after an out-of-memory answer drop the cache of freed
results and ask again -- "a new request, which may succeed", as include/bspgemm.h says of the hook.  The test accepts
BSPGEMM_OK from an armed call only with the exact counts and with exactly one request more than a cold call makes (the
failed one, repeated), and from at most those four k; every other k must end in BSPGEMM_ERR_ALLOC: the operands A', A'^T, S,
R and T (three arrays each), the tile rows.  A cold call makes 32 requests (measured on an MI355X: the retries were k = 1, 30,
31 and 32).  The sweep prints the count (ALLOCSWEEP) and stops with a failure at CAP, so a hook that never stops firing
cannot loop.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import lcc_ref

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
SENTINEL = 0x5A5A5A5A
CAP = 60
NAME = "bspgemm_local_clustering"
GRAPH = "k70_oriented"


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


class _Env:
    """one context with the graph uploaded"""

    def __init__(self, rp, ci, n):
        L = bspgemm.lib()
        self.n = n
        self.ctx, self.A = VP(), VP()
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        assert L.bspgemm_matrix_upload(self.ctx, n, n, rp.ctypes.data, ci.ctypes.data, C.byref(self.A)) == OK, _last_error()

    def call(self):
        """(status, counts, degree, lcc, info)"""
        R, info = VP(SENTINEL), bspgemm.LccInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        d, lcc = np.zeros(self.n, np.int32), np.zeros(self.n, np.float64)
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.A, bspgemm.LCC_DIRECTED, C.byref(R), d.ctypes.data, lcc.ctypes.data,
                                          C.byref(info))
        return st, R, d, lcc, info

    def values(self, R):
        """the counts downloaded, the result freed"""
        L = bspgemm.lib()
        num = np.zeros(self.n, np.int32)
        assert L.bspgemm_result_nnz(R) == self.n
        assert L.bspgemm_result_download_values(self.ctx, R, num.ctypes.data) == OK, _last_error()
        L.bspgemm_result_free(R)
        return num

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


def test_every_allocation_failure_of_the_call():
    L = bspgemm.lib()
    rp, ci, n = lcc_ref.GRAPHS[GRAPH]()
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    e_num, e_d, e_lcc, e_triangles, e_reciprocal = lcc_ref.local_clustering(rp, ci, n, True)
    e_heavy = lcc_ref.heavy_entries(rp, ci, n, lcc_ref.LIGHT_DEFAULT)
    assert e_reciprocal > 0 and 0 < e_heavy < lcc_ref.half_entries(rp, ci, n) and e_num.min() > 0

    def exact(env, R, d, lcc, info, what):
        assert np.array_equal(env.values(R), e_num), what
        assert np.array_equal(d, e_d) and lcc.tobytes() == e_lcc.tobytes(), what
        got = info.as_dict()
        assert got == {"triangles": e_triangles, "entries": lcc_ref.half_entries(rp, ci, n), "heavy_entries": e_heavy,
                       "reciprocal": e_reciprocal}, (what, got)

    def good(env, what):
        st, R, d, lcc, info = env.call()
        assert st == OK and R.value not in (None, SENTINEL), "%s: status %d (%s)" % (what, st, _last_error())
        exact(env, R, d, lcc, info, what)

    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L.bspgemm_debug_fail_alloc(0)
    base = bspgemm.debug_alloc_state()
    failed, retried, cold = [], [], None
    for k in range(1, CAP + 1):
        what = "k=%d" % k
        env = _Env(rp, ci, n)
        try:
            before = bspgemm.debug_alloc_state()
            L.bspgemm_debug_fail_alloc(k)
            st, R, d, lcc, info = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                exact(env, R, d, lcc, info, what)
                cold = after[0] - before[0]
            else:
                assert fired == 1
                if st == OK:                         # (a documented retry: proven below by its request count)
                    exact(env, R, d, lcc, info, what + " armed")
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert R.value is None, "%s armed: *counts is %r after a failure, not NULL" % (what, R.value)
                    assert bytes(info) == bytes(C.sizeof(info)) and _last_error(), what
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
        pytest.fail("the hook still fires at k = %d" % CAP)
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % ("local_clustering", cold, failed, retried))
    assert failed, "no k ended in BSPGEMM_ERR_ALLOC"
    assert len(failed) + len(retried) == cold, (cold, failed, retried)                # every request of the call was failed once
    assert len(retried) <= 4 and len(failed) >= 15, (failed, retried)                 # five operands of three arrays each cannot be retried
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
