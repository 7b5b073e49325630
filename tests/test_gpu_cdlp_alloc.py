"""Every branch of bspgemm_label_propagation that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *P == NULL, a zeroed info and a message; the same call, unarmed,
on the same context returns the exact labels; after freeing every handle and destroying the context the gate's live count
and live bytes are back where they were.

The graph is a star of 5000 leaves: its hub is longer than a workgroup's row (cdlp_ref.GROUP_CAP), so the call needs a hub
table, and in a fresh context the growth of the values workspace that holds it is one of the requests.

Two requests cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's two workspaces (ensure_tmp: the call's
state and the symmetrize's scratch, grown once before anything else; ensure_tmpv: the hub tables), which after an
out-of-memory answer drop the cache of freed results and ask again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The test accepts BSPGEMM_OK from an armed call only with the exact labels and with
exactly one request more than a cold call makes (the failed one, repeated), and from at most two k; every other k must end
in BSPGEMM_ERR_ALLOC.

A cold call makes 15 device allocations (measured on an MI355X: the retries were k = 1 and k = 14): the workspace's request,
the ten of bspgemm_matrix_symmetrize (the tile rows of the context and three arrays each for the select's, the transpose's
and the union's operand), P.row_ptr and P.col_idx, the hub tables and the row-length bytes of P; the sweep prints the count
(ALLOCSWEEP) and stops with a failure at CAP, so a hook that never stops firing cannot loop.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import cdlp_ref

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
SENTINEL = 0x5A5A5A5A
CAP = 40
MAX_ITER = 3
NAME = "bspgemm_label_propagation"


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


class _Env:
    """one context with the graph uploaded"""

    def __init__(self, rp, ci, n):
        L = bspgemm.lib()
        self.ctx, self.A = VP(), VP()
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        assert L.bspgemm_matrix_upload(self.ctx, n, n, rp.ctypes.data, ci.ctypes.data, C.byref(self.A)) == OK, _last_error()

    def call(self):
        """(status, P, info)"""
        P, info = VP(SENTINEL), bspgemm.LpInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.A, None, MAX_ITER, C.byref(P), C.byref(info))
        return st, P, info

    def labels(self, P, n):
        """P downloaded and freed"""
        L = bspgemm.lib()
        rp, labels = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        assert L.bspgemm_matrix_nnz(P) == n
        assert L.bspgemm_matrix_download(self.ctx, P, rp.ctypes.data, labels.ctypes.data) == OK, _last_error()
        L.bspgemm_matrix_free(P)
        return rp, labels

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


def test_every_allocation_failure_of_the_call():
    L = bspgemm.lib()
    rp, ci, n = cdlp_ref.GRAPHS["star_hub_last"]()
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    e_labels, e_iterations, e_converged, e_changed, e_communities = cdlp_ref.label_propagation(rp, ci, n, MAX_ITER)
    e_classes = cdlp_ref.class_vertices(rp, ci, n)
    assert e_classes == [n - 1, 0, 0, 1] and (e_iterations, e_converged, e_changed) == (MAX_ITER, 0, n)

    def exact(env, P, info, what):
        g_rp, g_labels = env.labels(P, n)
        assert np.array_equal(g_rp, np.arange(n + 1)) and np.array_equal(g_labels, e_labels), what
        d = info.as_dict()
        assert (d["iterations"], d["converged"], d["changed"], d["communities"]) == (e_iterations, e_converged, e_changed, e_communities), (what, d)
        assert d["class_vertices"] == e_classes, (what, d)                    # a hub: the call needed a table

    def good(env, what):
        st, P, info = env.call()
        assert st == OK and P.value not in (None, SENTINEL), "%s: status %d (%s)" % (what, st, _last_error())
        exact(env, P, info, what)

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
            st, P, info = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                exact(env, P, info, what)
                cold = after[0] - before[0]
            else:
                assert fired == 1
                if st == OK:                         # (a workspace's documented retry: proven below by its request count)
                    exact(env, P, info, what + " armed")
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert P.value is None, "%s armed: *P is %r after a failure, not NULL" % (what, P.value)
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
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % ("label_propagation", cold, failed, retried))
    assert failed, "no k ended in BSPGEMM_ERR_ALLOC"
    assert len(failed) >= cold - 2 and len(retried) <= 2, (failed, retried)
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
