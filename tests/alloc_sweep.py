"""The allocation-failure sweep that every test_gpu_*alloc*.py drives through bspgemm_debug_fail_alloc (no tests in here).

A *case* builds its inputs in a fresh context (setup), runs ONE entry point (call -> Out) and reads its outputs back
(read); what it must produce is computed once on the CPU (expect).  sweep(case) runs it once undisturbed, which gives the
request count of a cold call (cold) and what the context holds afterwards, then with the k-th device allocation of the
call failing, k = 1 .. cold + 1, each in a fresh context.  The hook must fire once for every k <= cold and not at cold + 1.

An armed call either returns BSPGEMM_ERR_ALLOC (check_failure: every output handle NULL, the scalars of Case.failed, the
out-structs of Case.zeroed all zero bytes, the caller's arrays of Case.untouched as they were, a message), or BSPGEMM_OK
with the exact result: the BSPGEMM_FLOW_AUTO fallback to the exact flow, or a request that is made again after the cache
of freed results is dropped ("a new request, which may succeed", include/bspgemm.h).  Then the same call, unarmed, on the
same context must pass check_success (the exact result, the stats flags the case forces), the context must hold no fewer
device arrays than after the undisturbed call (a workspace that a failed call lost for good shows here), and after
close() the gate's live count and live bytes are back where they were (the leak check).  verdict() judges the tallies.
"""
import ctypes as C
import gc
import time

import numpy as np

import bspgemm
from abi_kit import SENTINEL, dirtied, last_error

VP = C.c_void_p
OK, ERR_ALLOC = 0, 2
FLOW_AUTO, FLOW_UB, FLOW_EXACT = 0, 1, 2


def L():
    return bspgemm.lib()


def alloc_state():
    return bspgemm.debug_alloc_state()


def _ptr(a):
    return a.ctypes.data if a.size else None


def filled(struct_type):
    """an out-struct of 0x5A bytes: a failed call must have zeroed it"""
    return dirtied(struct_type, 0x5A)


def fields(struct, names):
    """the named fields of an out-struct, as read() returns them"""
    return tuple(int(getattr(struct, k)) for k in names)


class Env:
    """one bspgemm_create'd context, the operands and results made in it, all freed by close()"""

    def __init__(self):
        self.ctx = VP()
        st = L().bspgemm_create(0, C.byref(self.ctx))
        assert st == OK and self.ctx.value, "bspgemm_create: %d %s" % (st, last_error())
        self.mats, self.ress = [], []

    def option(self, name, value):
        assert L().bspgemm_set_option(self.ctx, bspgemm.OPTIONS[name], value) == OK

    def flow(self, flow):
        assert L().bspgemm_set_flow(self.ctx, flow) == OK

    def upload(self, rp, ci, cols):
        rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        m = VP()
        st = L().bspgemm_matrix_upload(self.ctx, rp.size - 1, cols, _ptr(rp), _ptr(ci), C.byref(m))
        assert st == OK, "upload: %d %s" % (st, last_error())
        return self.mat(m)

    def mat(self, m):
        self.mats.append(m)
        return m

    def res(self, r):
        self.ress.append(r)
        return r

    def free_outputs(self, out):
        for kind, h in out.handles.values():
            if h.value and h.value != out.sentinel:
                if kind == "m":
                    self.mats = [x for x in self.mats if x is not h]
                    L().bspgemm_matrix_free(h)
                else:
                    self.ress = [x for x in self.ress if x is not h]
                    L().bspgemm_result_free(h)

    def stats(self):
        s = bspgemm.Stats()
        assert L().bspgemm_last_stats(self.ctx, C.byref(s)) == OK, last_error()
        return s.as_dict()

    def matrix(self, m):
        rows, nnz = L().bspgemm_matrix_rows(m), L().bspgemm_matrix_nnz(m)
        rp, ci = np.zeros(rows + 1, np.int32), np.zeros(nnz, np.int32)
        assert L().bspgemm_matrix_download(self.ctx, m, _ptr(rp), _ptr(ci)) == OK, last_error()
        return rp, ci

    def result(self, r, values=False):
        rows, nnz = L().bspgemm_result_rows(r), L().bspgemm_result_nnz(r)
        rp, ci = np.zeros(rows + 1, np.int64), np.zeros(nnz, np.int32)
        assert L().bspgemm_result_download(self.ctx, r, _ptr(rp), _ptr(ci)) == OK, last_error()
        if not values:
            assert not L().bspgemm_result_values_device(r), "a pattern-only product carries a values array"
            return rp, ci
        v = np.zeros(max(nnz, 1), np.int32)
        assert L().bspgemm_result_download_values(self.ctx, r, _ptr(v)) == OK, last_error()
        return rp, ci, v[:nnz]

    def close(self):
        for r in self.ress:
            L().bspgemm_result_free(r)
        for m in self.mats:
            L().bspgemm_matrix_free(m)
        L().bspgemm_destroy(self.ctx)
        self.ctx, self.mats, self.ress = VP(), [], []


class Out:
    """what one call returned: its status, its output handles {name: ("m" | "r", c_void_p)} (sentinel: what they held
    before the call), its scalar outputs {name: ctypes int}, its out-structs {name: ctypes Structure} and the arrays the
    caller owns {name: ndarray}"""

    def __init__(self, status, handles=None, scalars=None, structs=None, arrays=None, sentinel=SENTINEL):
        self.status, self.handles, self.scalars = status, handles or {}, scalars or {}
        self.structs, self.arrays, self.sentinel = structs or {}, arrays or {}, sentinel


def call_to_handle(kind, name, fn, structs=None, sentinel=SENTINEL):
    """fn(env, inp, byref(handle), *byref(fresh out-structs)) -> status, for the entry points that return one operand
    ("m") or one result ("r"); structs: {name: ctypes Structure type}, each passed pre-filled with 0x5A"""
    def call(env, inp):
        h = VP(sentinel)
        made = {key: filled(t) for key, t in (structs or {}).items()}
        st = fn(env, inp, C.byref(h), *[C.byref(s) for s in made.values()])
        if st == OK and h.value not in (None, sentinel):
            (env.mat if kind == "m" else env.res)(h)
        return Out(st, {name: (kind, h)}, structs=made, sentinel=sentinel)
    return call


class Case:
    """setup(env) -> inputs; call(env, inputs) -> Out; read(env, inputs, out) -> tuple of arrays / ints; expect() -> the same
    from the CPU (computed once); flags: bspgemm_stats fields a successful call must show; auto: the BSPGEMM_FLOW_AUTO
    fallback is what the case must show.  After a failure: failed: {scalar output: its value}; zeroed: the out-structs
    that are all zero bytes; untouched: {caller-owned array: the value every element still has}.
    The end of the sweep (verdict): cap: the most requests a cold call may make; min_failed: the fewest k that end in
    BSPGEMM_ERR_ALLOC, an int or a function of cold; max_retried: the most k at which the armed call may succeed (None: any
    number); retried_only_at: the one k at which it may (None: anywhere); strict_requests: such a call made exactly one
    request more than a cold call, the failed one again."""

    def __init__(self, name, setup, call, read, expect, flags=None, auto=False, failed=None, zeroed=(), untouched=None,
                 cap=None, min_failed=1, max_retried=None, retried_only_at=None, strict_requests=False):
        self.name, self.setup, self.call, self.read, self._expect = name, setup, call, read, expect
        self.flags, self.auto, self.failed, self.zeroed, self.untouched = flags or {}, auto, failed or {}, zeroed, untouched or {}
        self.cap, self.min_failed, self.max_retried = cap, min_failed, max_retried
        self.retried_only_at, self.strict_requests = retried_only_at, strict_requests
        self._cached = None

    def expect(self):
        if self._cached is None:
            self._cached = self._expect()
        return self._cached


def same(a, b):
    if len(a) != len(b):
        return False
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def check_success(case, env, inputs, out, what):
    assert out.status == OK, "%s: status %d (%s)" % (what, out.status, last_error())
    for name, (_, h) in out.handles.items():
        assert h.value and h.value != out.sentinel, "%s: no %s handle after BSPGEMM_OK" % (what, name)
    got = case.read(env, inputs, out)
    assert same(got, case.expect()), "%s: the result differs from the reference" % what
    if case.flags:
        st = env.stats()
        for key, want in case.flags.items():
            assert st[key] == want, "%s: stats.%s = %r, the case forces %r" % (what, key, st[key], want)


def check_failure(case, out, what):
    assert out.status == ERR_ALLOC, "%s: status %d (%s), not BSPGEMM_ERR_ALLOC" % (what, out.status, last_error())
    for name, (_, h) in out.handles.items():
        assert h.value is None, "%s: output handle %s is %r after a failure, not NULL" % (what, name, h.value)
    for name, want in case.failed.items():
        assert out.scalars[name].value == want, "%s: *%s = %r after a failure, not %r" % (what, name, out.scalars[name].value, want)
    for name in case.zeroed:
        s = out.structs[name]
        assert bytes(s) == bytes(C.sizeof(s)), "%s: *%s is not all zero bytes after a failure" % (what, name)
    for name, want in case.untouched.items():
        assert (out.arrays[name] == want).all(), "%s: %s was written by a call that failed" % (what, name)
    assert last_error(), "%s: bspgemm_last_error() is empty after a failure" % what


def verdict(case, cold, failed, fell_back, retried):
    """the end of a sweep: failed and fell_back are lists of k, retried a list of (k, requests of that armed call)"""
    name = case.name
    assert sorted(failed + fell_back + [k for k, _ in retried]) == list(range(1, cold + 1)), (
        "%s: not every one of the %d requests was failed once: %r %r %r" % (name, cold, failed, fell_back, retried))
    if case.auto:
        assert fell_back, "%s: no k showed BSPGEMM_OK with stats.flow == BSPGEMM_FLOW_EXACT" % name
        assert not failed, "%s: BSPGEMM_FLOW_AUTO returned BSPGEMM_ERR_ALLOC at k = %s" % (name, failed)
    else:
        assert failed, "%s: no k ended in BSPGEMM_ERR_ALLOC" % name
        least = case.min_failed(cold) if callable(case.min_failed) else case.min_failed
        assert len(failed) >= least, "%s: BSPGEMM_ERR_ALLOC at %d k, at least %d must: %r" % (name, len(failed), least, failed)
        if case.max_retried is not None:
            assert len(retried) <= case.max_retried, "%s: armed calls succeeded at %r, at most %d may" % (name, retried, case.max_retried)
        if case.retried_only_at is not None:
            assert all(k == case.retried_only_at for k, _ in retried), "%s: armed calls succeeded at %r, only k = %d may" % (
                name, retried, case.retried_only_at)
    if case.strict_requests:                         # the failed request was made again, and nothing else
        assert all(requests == cold + 1 for _, requests in retried), "%s: %r, a cold call makes %d requests" % (name, retried, cold)


def sweep(case):
    gc.collect()                                     # (contexts that earlier tests dropped go now, not in the middle)
    L().bspgemm_debug_fail_alloc(0)
    base = alloc_state()
    case.expect()
    t0 = time.time()

    def closed(what):
        now = alloc_state()
        assert now[1:3] == base[1:3], "%s: leak: live (count, bytes) %r, before the context %r" % (what, now[1:3], base[1:3])

    # an undisturbed call: its request count bounds the sweep, and it is the reference for what a context holds afterwards
    env = Env()
    try:
        inputs = case.setup(env)
        before = alloc_state()
        out = case.call(env, inputs)
        cold = alloc_state()[0] - before[0]
        check_success(case, env, inputs, out, "%s unarmed" % case.name)
        clean_live = alloc_state()[1] - base[1]
    finally:
        env.close()
    closed("%s unarmed" % case.name)
    assert 1 <= cold <= case.cap, "%s: a cold call makes %d requests, at most %d are expected" % (case.name, cold, case.cap)

    failed, fell_back, retried, fired = [], [], [], True
    for k in range(1, cold + 2):
        what = "%s k=%d" % (case.name, k)
        env = Env()
        try:
            inputs = case.setup(env)
            before = alloc_state()
            L().bspgemm_debug_fail_alloc(k)
            out = case.call(env, inputs)
            L().bspgemm_debug_fail_alloc(0)
            after = alloc_state()
            fired = after[3] - before[3]
            if not fired:
                assert k == cold + 1, "%s: the hook is not reached, a cold call makes %d requests" % (what, cold)
                check_success(case, env, inputs, out, what + " (hook not reached)")
            else:
                assert fired == 1
                if out.status == OK:
                    check_success(case, env, inputs, out, what + " armed")
                    flow = env.stats()["flow"] if case.flags else None
                    if case.auto and flow == FLOW_EXACT:
                        fell_back.append(k)
                    else:
                        retried.append((k, after[0] - before[0]))
                    env.free_outputs(out)
                else:
                    check_failure(case, out, what + " armed")
                    failed.append(k)
                again = case.call(env, inputs)
                check_success(case, env, inputs, again, what + " repeated")
                if case.auto:
                    assert env.stats()["flow"] == FLOW_UB, "%s repeated: flow %d" % (what, env.stats()["flow"])
                live = alloc_state()[1] - base[1]
                assert live >= clean_live, ("%s repeated: the context holds %d device arrays, %d after an undisturbed call: "
                                            "the failed call lost one for good" % (what, live, clean_live))
        finally:
            L().bspgemm_debug_fail_alloc(0)
            env.close()
        closed(what)
    assert not fired, "%s: the hook still fires at k = %d, one past the %d requests of a cold call" % (case.name, cold + 1, cold)
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  exact fallback at %s  retried at %s  %.2f s"
          % (case.name, cold, failed, fell_back, retried, time.time() - t0))
    verdict(case, cold, failed, fell_back, retried)
