"""Every branch of bspgemm_matrix_extract that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of one call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *out = NULL, a zeroed info and a message; the same call,
unarmed, on the same context returns the model's bits; after freeing every handle and destroying the context the gate's live
count and live bytes are back where they were.

The variants: canonical (the workspace, the tile rows, the operand's three arrays), hub (the values workspace for the chunk
records too), untidy (the call canonicalises A: two transposes, whose operands it owns and frees) and fallback (an out row
beyond the workgroup sort: out goes through two transposes, and the first out is freed).

The requests for a context workspace cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook (ensure_tmp and ensure_tmpv; how
many a variant makes stands in VARIANTS): after an out-of-memory answer they drop the cache of freed results and ask again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The test accepts BSPGEMM_OK from an armed call only with the exact result and with
exactly one request more than a cold call makes.  The sweep ends within the request count of a first unarmed run (plus the
one k at which the hook no longer fires): a condition, not a loop until something breaks.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bspgemm
import gen
import extract_ref as X

pytestmark = pytest.mark.gpu

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
NAME = "bspgemm_matrix_extract"


def _canonical():
    rp, ci, n = gen.rmat(10, 8, (0.45, 0.22, 0.22, 0.11), seed=51)
    rng = np.random.default_rng(52)
    return rp, ci, n, n, rng.integers(0, n, 300).astype(np.int32), np.sort(rng.permutation(n)[:400]).astype(np.int32), 0


def _hub():
    return X.hub_case() + (0,)


def _untidy():
    rp, ci, n = gen.dups_unsorted(500, 6, seed=9)
    p = np.random.default_rng(53).permutation(n).astype(np.int32)
    return rp, ci, n, n, p, p, 1


def _fallback():
    rp, ci, rows, cols = X.sort_case(True)
    return rp, ci, rows, cols, None, np.arange(cols, dtype=np.int32)[::-1].copy(), 0


VARIANTS = {
    # name: (case, the fewest k that must end in ERR_ALLOC, the most requests for a workspace, each of which is retried:
    # the call's own (ensure_tmp, which covers the transposes of an untidy A), with hubs the values workspace for the
    # chunk records (ensure_tmpv, sized after read-back one), and in the fallback the transposes of `out`, should they need
    # more than the call's own)
    "canonical": (_canonical, 3, 1),
    "hub": (_hub, 3, 2),
    "untidy": (_untidy, 8, 1),
    "fallback": (_fallback, 8, 3),
}


def _last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


class _Env:
    """one context with the operand uploaded"""

    def __init__(self, rp, ci, rows, cols, I, J, flags):
        L = bspgemm.lib()
        self.I, self.J, self.flags = I, J, flags
        self.ctx, self.A = VP(), VP()
        assert L.bspgemm_create(0, C.byref(self.ctx)) == OK and self.ctx.value, _last_error()
        assert L.bspgemm_matrix_upload(self.ctx, rows, cols, rp.ctypes.data, ci.ctypes.data, C.byref(self.A)) == OK, _last_error()

    def call(self):
        """(status, out handle, info)"""
        info, out = bspgemm.ExtractInfo(), VP(77)
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        I, J = self.I, self.J
        st = getattr(bspgemm.lib(), NAME)(self.ctx, self.A, 0 if I is None else I.size, None if I is None else I.ctypes.data,
                                          0 if J is None else J.size, None if J is None else J.ctypes.data, self.flags,
                                          C.byref(out), C.byref(info))
        return st, out, info

    def download(self, out, kept):
        L = bspgemm.lib()
        rows = L.bspgemm_matrix_rows(out)
        rp, ci = np.zeros(rows + 1, np.int32), np.zeros(max(kept, 1), np.int32)
        assert L.bspgemm_matrix_download(self.ctx, out, rp.ctypes.data, ci.ctypes.data) == OK, _last_error()
        L.bspgemm_matrix_free(out)
        return rp, ci[:kept]

    def close(self):
        L = bspgemm.lib()
        L.bspgemm_matrix_free(self.A)
        L.bspgemm_destroy(self.ctx)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_allocation_failure_of_the_call(variant):
    L = bspgemm.lib()
    case, least, workspace_requests = VARIANTS[variant]
    rp, ci, rows, cols, I, J, canonicalised = case()
    exp = X.model(rp, ci, rows, cols, I, J)
    assert exp["canonicalised"] == canonicalised and (exp["sorted_by"] == 2) == (variant == "fallback")
    assert (exp["hub_chunks"] > 0) == (variant in ("hub", "fallback"))

    def exact(env, out, info, what):
        assert all(getattr(info, k) == exp[k] for k in X.INFO), (what, info.as_dict())
        grp, gci = env.download(out, int(info.kept))
        assert np.array_equal(grp, exp["rp"]) and np.array_equal(gci, exp["ci"]), what

    def good(env, what):
        st, out, info = env.call()
        assert st == OK, "%s: status %d (%s)" % (what, st, _last_error())
        exact(env, out, info, what)

    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L.bspgemm_debug_fail_alloc(0)
    base = bspgemm.debug_alloc_state()
    # a first unarmed run: its request count bounds the sweep
    env = _Env(rp, ci, rows, cols, I, J, 0)
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
        env = _Env(rp, ci, rows, cols, I, J, 0)
        try:
            before = bspgemm.debug_alloc_state()
            L.bspgemm_debug_fail_alloc(k)
            st, out, info = env.call()
            L.bspgemm_debug_fail_alloc(0)
            after = bspgemm.debug_alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert k == cold + 1, "%s: the hook is not reached, a cold call makes %d requests" % (what, cold)
                assert st == OK, "%s (hook not reached): status %d (%s)" % (what, st, _last_error())
                exact(env, out, info, what)
            else:
                assert fired == 1
                if st == OK:                         # (the documented retry: proven by its request count)
                    exact(env, out, info, what + " armed")
                    retried.append((k, after[0] - before[0]))
                else:
                    assert st == ERR_ALLOC, "%s armed: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, st, _last_error())
                    assert bytes(info) == bytes(C.sizeof(info)) and _last_error(), what
                    assert out.value is None, what + ": *out is not NULL"
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
    assert len(retried) <= workspace_requests and len(failed) >= least, (failed, retried)
    assert all(requests == cold + 1 for _, requests in retried), (retried, cold)    # the failed request was made again
