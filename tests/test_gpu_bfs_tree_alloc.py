"""Every branch of bspgemm_bfs_tree that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *tree == NULL, a zeroed info block and a message; the same
call, unarmed, on the same context returns the exact tree; after freeing every handle and destroying the context the gate's
live count and live bytes are back where they were.  The sweep runs twice: with AT == NULL under PULL, so that the
transpose's allocations are inside the call, and with AT given under AUTO.

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp), which after an
out-of-memory answer drops the cache of freed results and asks again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The call grows the workspace once, before anything else, so that is k = 1: the armed
call returns BSPGEMM_OK.  The test accepts BSPGEMM_OK from an armed call only at k = 1, only with the exact tree and with
exactly one request more than a cold call makes (the failed one, repeated); every other k must end in BSPGEMM_ERR_ALLOC.
The result's three buffers are asked for once each (csrc/bfs_tree.hip: tree_buffer), so they end in BSPGEMM_ERR_ALLOC too.

A cold call with AT == NULL makes 8 device allocations (measured on an MI355X; the sweep prints it, ALLOCSWEEP): the
workspace, the tile rows of the operand check, the transpose's row_ptr, col_idx and row-length bytes, and the result's
row_ptr, col_idx and values: ERR_ALLOC at k = 2 .. 8, retried at k = 1.  With AT given it makes 4: the transpose that the
test ran beforehand has left a workspace that is large enough, so no k is retried and k = 1 .. 4 end in ERR_ALLOC.  The sweep
stops with a failure at twice the count, so a hook that never stops firing cannot loop.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bfs_tree_ref as ref
import bspgemm

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
SENTINEL = 0x5A5A5A5A
NAME = "rmat12_directed"
AUTO, PULL = 0, 2


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


class _Env:
    """one context with the graph uploaded and, with_at, its transpose"""

    def __init__(self, rp, ci, n, with_at):
        L = bspgemm.lib()
        self.ctx, self.A, self.AT = VP(), VP(), VP()
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        assert L.bspgemm_matrix_upload(self.ctx, n, n, rp.ctypes.data, ci.ctypes.data, C.byref(self.A)) == OK, _last_error()
        if with_at:
            assert L.bspgemm_matrix_transpose(self.ctx, self.A, C.byref(self.AT)) == OK, _last_error()

    def call(self, source, direction):
        """(status, tree, info)"""
        T, info = VP(SENTINEL), bspgemm.BfsTreeInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = bspgemm.lib().bspgemm_bfs_tree(self.ctx, self.A, self.AT if self.AT.value else None, source, direction, 0,
                                            C.byref(T), C.byref(info))
        return st, T, info

    def tree(self, T, n):
        """the result downloaded and freed"""
        L = bspgemm.lib()
        nnz = L.bspgemm_result_nnz(T)
        rp, parent, level = np.zeros(n + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.int32)
        assert L.bspgemm_result_download(self.ctx, T, rp.ctypes.data, parent.ctypes.data) == OK, _last_error()
        assert L.bspgemm_result_download_values(self.ctx, T, level.ctypes.data) == OK, _last_error()
        L.bspgemm_result_free(T)
        return rp, parent, level

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.AT)
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


@pytest.mark.parametrize("with_at,direction,cold_expected", [(False, PULL, 8), (True, AUTO, 4)])
def test_every_allocation_failure_of_the_call(with_at, direction, cold_expected):
    L = bspgemm.lib()
    rp, ci, n, source = ref.graph(NAME)
    exp = ref.expected(NAME)
    model = ref.model(rp, ci, n, source, direction="pull" if direction == PULL else "auto")
    assert model["pull_levels"] > 0 and exp[1].size > 1000
    cap = 2 * cold_expected

    def exact(env, T, info, what):
        got = env.tree(T, n)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), what
        assert {k: v for k, v in info.as_dict().items() if k in model} == model, what
        assert (info.transposed, info.canonicalised) == (int(not with_at), 0), what

    def good(env, what):
        st, T, info = env.call(source, direction)
        assert st == OK and T.value not in (None, SENTINEL), "%s: status %d (%s)" % (what, st, _last_error())
        exact(env, T, info, what)

    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L.bspgemm_debug_fail_alloc(0)
    base = bspgemm.debug_alloc_state()
    failed, retried, cold = [], [], None
    for k in range(1, cap + 1):
        what = "k=%d" % k
        env = _Env(rp, ci, n, with_at)
        try:
            before = bspgemm.debug_alloc_state()
            L.bspgemm_debug_fail_alloc(k)
            st, T, info = env.call(source, direction)
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                exact(env, T, info, what)
                cold = after[0] - before[0]
            else:
                assert fired == 1
                if st == OK:                         # (the workspace's documented retry: proven below by its request count)
                    exact(env, T, info, what + " armed")
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert T.value is None, "%s armed: *tree is %r after a failure, not NULL" % (what, T.value)
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
        pytest.fail("the hook still fires at k = %d" % cap)
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % ("bfs_tree, AT %s" % ("given" if with_at else "NULL"),
                                                                        cold, failed, retried))
    assert failed, "no k ended in BSPGEMM_ERR_ALLOC"
    assert len(failed) >= cold - 1 and len(retried) <= 1, (failed, retried)
    assert all(k == 1 and requests == cold + 1 for k, requests in retried), (retried, cold)   # the workspace request, made again
