"""Every branch of bspgemm_multiply_masked_dot that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  The three operands are NOT canonical (A holds repeats, B's rows are unsorted, F both), so the call also
runs its canonicalising branch: three pairs of transposes, each with its operands and workspace, then the passes again.

An armed call returns BSPGEMM_ERR_ALLOC with *C == NULL, a zeroed info and a message; or, where the request that failed
belongs to the context's workspace (ensure_tmp) or to the result's buffers (result_alloc), which after an out-of-memory
answer drop the cache of freed results and ask again -- "a new request, which may succeed", as include/bspgemm.h says of
the hook -- BSPGEMM_OK with the exact result and exactly one request more than a cold call makes (the failed one,
repeated).  The same call, unarmed, on the same context returns the exact result; after freeing every handle and
destroying the context the gate's live count and live bytes are back where they were.

The sweep prints the cold call's allocation count (ALLOCSWEEP) and stops with a failure at CAP, so a hook that never
stops firing cannot loop.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import dot_ref

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
SENTINEL = 0x5A5A5A5A
CAP = 96
NAME = "bspgemm_multiply_masked_dot"
N, M, COLS = 400, 300, 150


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


def _inputs():
    rng = np.random.default_rng(8801)

    def rows(n, ncols, lo, hi, repeats, shuffle):
        out = []
        for k in rng.integers(lo, hi, n):
            r = np.sort(rng.choice(ncols, size=int(k), replace=False)).tolist()
            if repeats:
                r = sorted(r + [r[int(q)] for q in rng.integers(0, len(r), 2)])
            if shuffle:
                r = [r[int(q)] for q in rng.permutation(len(r))]
            out.append(r)
        return dot_ref.csr(out)

    return rows(N, COLS, 2, 80, True, False), rows(M, COLS, 2, 80, False, True), rows(N, M, 8, 20, True, True)


class _Env:
    """one context with the three operands uploaded"""

    def __init__(self, a, b, f):
        L = bspgemm.lib()
        self.ctx, self.h = VP(), [VP(), VP(), VP()]
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        for (rp, ci), rows, cols, h in ((a, N, COLS, self.h[0]), (b, M, COLS, self.h[1]), (f, N, M, self.h[2])):
            assert L.bspgemm_matrix_upload(self.ctx, rows, cols, rp.ctypes.data, ci.ctypes.data, C.byref(h)) == OK, _last_error()

    def call(self):
        """(status, C, info)"""
        r, info = VP(SENTINEL), bspgemm.DotInfo(7, 7, 7, 7)
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.h[0], self.h[1], self.h[2], 0, C.byref(r), C.byref(info))
        return st, r, info.as_dict()

    def result(self, r):
        """C downloaded and freed"""
        L = bspgemm.lib()
        nnz = L.bspgemm_result_nnz(r)
        rp, ci, v = np.zeros(N + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.int32)
        assert L.bspgemm_result_rows(r) == N
        assert L.bspgemm_result_download(self.ctx, r, rp.ctypes.data, ci.ctypes.data) == OK, _last_error()
        assert L.bspgemm_result_download_values(self.ctx, r, v.ctypes.data) == OK, _last_error()
        L.bspgemm_result_free(r)
        return rp, ci, v

    def close(self):
        L = bspgemm.lib()
        for h in self.h:
            L.bspgemm_matrix_free(h)
        L.bspgemm_destroy(self.ctx)


def test_every_allocation_failure_of_the_call():
    L = bspgemm.lib()
    a, b, f = _inputs()
    exp = dot_ref.dot_ref(a, b, f, N, M, COLS, M)
    entries = dot_ref.heavy_at_zero(a, b, f, N, M, COLS, M)[1]
    assert exp[1].size > 1000 and f[1].size > entries > 4096

    def exact(env, r, info, what):
        got = env.result(r)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), what
        assert info["canonicalised"] == 7 and info["entries"] == entries and info["kept"] == exp[1].size, (what, info)

    def good(env, what):
        st, r, info = env.call()
        assert st == OK and r.value not in (None, SENTINEL), "%s: status %d (%s)" % (what, st, _last_error())
        exact(env, r, info, what)

    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L.bspgemm_debug_fail_alloc(0)
    base = bspgemm.debug_alloc_state()
    failed, retried, cold = [], [], None
    for k in range(1, CAP + 1):
        what = "k=%d" % k
        env = _Env(a, b, f)
        try:
            before = bspgemm.debug_alloc_state()
            L.bspgemm_debug_fail_alloc(k)
            st, r, info = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                exact(env, r, info, what)
                cold = after[0] - before[0]
            else:
                assert fired == 1
                if st == OK:                         # (the documented retry: proven below by its request count)
                    exact(env, r, info, what + " armed")
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert r.value is None, "%s armed: *C is %r after a failure, not NULL" % (what, r.value)
                    assert info == {"entries": 0, "heavy_entries": 0, "kept": 0, "canonicalised": 0} and _last_error(), what
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
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  retried at %s" % ("multiply_masked_dot", cold, failed, retried))
    assert failed, "no k ended in BSPGEMM_ERR_ALLOC"
    assert len(failed) + len(retried) == cold, (cold, failed, retried)                # every request of the call was failed once
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
    assert len(failed) >= 18, failed                 # the six transposes' operands (three arrays each) cannot be retried
