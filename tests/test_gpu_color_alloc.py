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
union's operand), then P.row_ptr, P.col_idx and the row-length bytes of P.  The sweep stops with a failure at twice that,
so a hook that never stops firing cannot loop.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import color_ref
import gen

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
SENTINEL = 0x5A5A5A5A
COLD = 14
CAP = 2 * COLD
ORDER, SEED = 3, 11             # BSPGEMM_COLOR_LARGEST_FIRST
NAME = "bspgemm_graph_coloring"


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
        """(status, P, ncolors, rounds)"""
        P, colors, rounds = VP(SENTINEL), C.c_int(-1), C.c_int(-1)
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.A, ORDER, SEED, C.byref(P), C.byref(colors), C.byref(rounds))
        return st, P, colors.value, rounds.value

    def colours(self, P, n):
        """P downloaded and freed"""
        L = bspgemm.lib()
        rp, colour = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        assert L.bspgemm_matrix_nnz(P) == n
        assert L.bspgemm_matrix_download(self.ctx, P, rp.ctypes.data, colour.ctypes.data) == OK, _last_error()
        L.bspgemm_matrix_free(P)
        return rp, colour

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


def test_every_allocation_failure_of_the_call():
    L = bspgemm.lib()
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 5403)
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    e_colour, e_colors, e_rounds = color_ref.coloring(rp, ci, n, "largest", SEED)
    assert 2 < e_colors < n and e_rounds > 1

    def good(env, what):
        st, P, colors, rounds = env.call()
        assert st == OK and P.value not in (None, SENTINEL), "%s: status %d (%s)" % (what, st, _last_error())
        g_rp, g_colour = env.colours(P, n)
        assert np.array_equal(g_rp, np.arange(n + 1)) and np.array_equal(g_colour, e_colour), what
        assert (colors, rounds) == (e_colors, e_rounds), (what, colors, rounds)

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
            st, P, colors, rounds = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                g_rp, g_colour = env.colours(P, n)
                assert np.array_equal(g_colour, e_colour) and (colors, rounds) == (e_colors, e_rounds)
                cold = after[0] - before[0]
            else:
                assert fired == 1
                if st == OK:                         # (the workspace's documented retry: proven below by its request count)
                    g_rp, g_colour = env.colours(P, n)
                    assert np.array_equal(g_rp, np.arange(n + 1)) and np.array_equal(g_colour, e_colour), what + " armed"
                    assert (colors, rounds) == (e_colors, e_rounds), (what, colors, rounds)
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert P.value is None, "%s armed: *P is %r after a failure, not NULL" % (what, P.value)
                    assert (colors, rounds) == (0, 0) and _last_error(), what
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
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % ("graph_coloring", cold, failed, retried))
    assert failed, "no k ended in BSPGEMM_ERR_ALLOC"
    assert len(failed) >= cold - 1 and len(retried) <= 1, (failed, retried)
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
