"""Every branch that follows a failed device allocation, taken one at a time through bspgemm_debug_fail_alloc.

A *case* builds its inputs in a fresh context, runs ONE entry point and reads its outputs back; what it must produce is
computed once on the CPU (oracle/oracle.py for the plain products, scipy and the tests' *_ref modules for the rest).  The
sweep (tests/alloc_sweep.py) runs the case with the k-th device allocation of the entry point failing, k = 1, 2, ... until
the hook no longer fires, one past the requests of an undisturbed call.  A call whose allocation failed either returns
BSPGEMM_ERR_ALLOC with every output handle NULL and a message, or
succeeds with the exact reference result (BSPGEMM_FLOW_AUTO falls back to the exact flow; the retry after dropping the
result cache is a new request, which succeeds).  Then the same call, unarmed, on the same context must return the exact
result with the path flags the case forces, the context must hold no fewer device arrays than after an undisturbed call
(a workspace that a failed call lost for good shows here), and after freeing every handle and destroying the context the
gate's live count and live bytes are back where they were (the leak check).

Under BSPGEMM_FLOW_AUTO a one-shot failure can never end in BSPGEMM_ERR_ALLOC: whatever fails in the upper-bound flow, the
exact flow that follows meets no failure.  Those cases must show the fallback instead (BSPGEMM_OK with stats.flow ==
BSPGEMM_FLOW_EXACT for at least one k); every other case must end in BSPGEMM_ERR_ALLOC for at least one k.

Device allocations of a cold call (the k at which the hook no longer fires, minus one), measured on an MI355X; a case
whose cold call makes more than twice that fails before its sweep, and the loops of create and the drop-ins stop with a
failure there, so a hook that never stops firing cannot loop for ever (the drop-ins: a call on their warm process-wide
context, which allocates its operands only):

    case                        cold   case                        cold   case                        cold
    multiply-auto                 17   from_result                    3   bfs-check                     45
    multiply-upper-bound          17   from_result_where              3   connected_components           5
    multiply-exact                16   transpose                      4   core_numbers                  15
    multiply-auto-knobs           24   select                         5   kcore                         40
    multiply-upper-bound-knobs    24   setop-or-unsorted             17   closure                       31
    multiply-exact-knobs          23   setop-xor-unsorted            17   closure_ex-transitive         33
    multiply-small                14   setop-or-canonical             5   row_work_prefix               11
    multiply-rank                 17   setop-xor-canonical            5   partition_rows                11
    masked                        17   equal                          9   create                         5
    masked_ex-complement          17   symmetrize                    19   SpGEMM_hip                     3
    accumulate                    17   triangle_count                29   SpGEMM_hip_bigslice            3
    masked_count                  19   ktruss                        41   SpGEMM_hip_mat                 3
    upload-interior                3   bfs                           45   SpGEMM_hip_masked              6

One bspgemm_create + bspgemm_destroy takes 12 ms there (the event sets of its 16 stat slots included); the slowest case
(bfs with BSPGEMM_OPT_CHECK, 47 contexts) 0.16 s, a family's first case 0.25 s (it loads the kernels).
"""
import ctypes as C
import gc
import time

import numpy as np
import pytest
import scipy.sparse as sp

import bfs_ref
import bspgemm
import cc_ref
import gen
import kcore_ref
import ktruss_ref
import setop_ref
from alloc_sweep import (ERR_ALLOC, FLOW_AUTO, FLOW_EXACT, FLOW_UB, OK, SENTINEL, VP, Case, Env, L, Out, alloc_state,
                         call_to_handle, last_error, same, sweep)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# cold allocation counts (the table above); a case's cap is twice the entry
COLD = {
    "multiply-auto": 17, "multiply-upper-bound": 17, "multiply-exact": 16, "multiply-auto-knobs": 24,
    "multiply-upper-bound-knobs": 24, "multiply-exact-knobs": 23, "multiply-small": 14, "multiply-rank": 17,
    "masked": 17, "masked_ex-complement": 17, "accumulate": 17, "masked_count": 19, "upload-interior": 3,
    "from_result": 3, "from_result_where": 3, "transpose": 4, "select": 5, "setop-or-unsorted": 17,
    "setop-xor-unsorted": 17, "setop-or-canonical": 5, "setop-xor-canonical": 5, "equal": 9, "symmetrize": 19,
    "triangle_count": 29, "ktruss": 41, "bfs": 45, "bfs-check": 45, "connected_components": 5, "core_numbers": 15,
    "kcore": 40, "closure": 31, "closure_ex-transitive": 33, "row_work_prefix": 11, "partition_rows": 11, "create": 5,
    "SpGEMM_hip": 3, "SpGEMM_hip_bigslice": 3, "SpGEMM_hip_mat": 3, "SpGEMM_hip_masked": 6,
}


# ------------------------------------------------------------------ inputs and references ------------------------------
R0, R1, NCOLS = 10, 190, 4096
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def mixed():
    return memo("mixed", gen.mixed_class_rows)


def mask():
    """200 x 4096, 30 draws per row, entries in stored (sorted) order"""
    return memo("mask", lambda: gen.uniform_rect(200, NCOLS, 30, 77))


def _ones(rp, ci, shape):
    m = sp.csr_matrix((np.ones(np.asarray(ci).size, np.int64), np.asarray(ci), np.asarray(rp)), shape=shape)
    m.sum_duplicates()
    return m


def product_ref(a_rp, a_ci, b_rp, b_ci, cols, r0, r1, mode=None, f=None):
    """scipy: rows [r0, r1) of A1 @ B1 (counts), kept under pattern(F) ("keep", "count"), outside it ("drop") or joined
    with it ("insert"); (row_ptr int64, col_idx int32, counts int32), rows ascending"""
    nb = np.asarray(b_rp).size - 1
    A = sp.csr_matrix((np.ones(np.asarray(a_ci).size, np.int64), np.asarray(a_ci), np.asarray(a_rp)), shape=(np.asarray(a_rp).size - 1, nb))
    P = (A[r0:r1] @ _ones(b_rp, b_ci, (nb, cols))).tocsr()
    if mode:
        F = _ones(f[0], f[1], (np.asarray(f[0]).size - 1, cols))[r0:r1]
        F.data[:] = 1
        inside = P.multiply(F).tocsr()
        P = inside if mode in ("keep", "count") else (P - inside).tocsr() if mode == "drop" else (P + F).tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    return P.indptr.astype(np.int64), P.indices.astype(np.int32), P.data.astype(np.int32)


def knob_setup(knobs):
    def apply(env):
        env.option("small_path", 0)
        if knobs:
            for name, value in (("padded_rows", 1), ("blocked_extents", 1), ("check", 1), ("class_streams", 3)):
                env.option(name, value)
    return apply


def knob_flags(knobs):
    return dict(padded_rows=1, prepass_kernel=1, checked=1, class_streams=3) if knobs else dict(padded_rows=0, checked=0)


def call_product(fn_name, with_f=False, ex_flags=None):
    def call(env, inp):
        r = VP(SENTINEL)
        fn = getattr(L(), fn_name)
        args = [env.ctx, inp["A"], inp["B"]] + ([inp["F"]] if with_f else []) + ([ex_flags] if ex_flags is not None else [])
        st = fn(*args, inp["r0"], inp["r1"], C.byref(r))
        if st == OK and r.value not in (None, SENTINEL):
            env.res(r)
        return Out(st, {"C": ("r", r)})
    return call


def multiply_case(name, flow, knobs):
    a_rp, a_ci, b_rp, b_ci = mixed()

    def setup(env):
        knob_setup(knobs)(env)
        env.flow(flow)
        return dict(A=env.upload(a_rp, a_ci, 512), B=env.upload(b_rp, b_ci, NCOLS), r0=R0, r1=R1)

    def expect():
        rp, ci = O.spgemm_rows(a_rp, a_ci, b_rp, b_ci, NCOLS, R0, R1)
        bins = gen.expected_bins(gen.row_products(a_rp, a_ci, b_rp, R0, R1), NCOLS)
        # empty rows, one-wave rows in at least three capacity classes, a heavy row (more than 2048 products)
        assert bins[0] > 0 and sum(1 for b in bins[1:gen.RANK_BIN] if b > 0) >= 3 and sum(bins[gen.RANK_BIN:]) >= 1, bins
        return rp, ci, bins

    def read(env, inp, out):
        return env.result(out.handles["C"][1]) + (env.stats()["rows_per_bin"],)

    flags = knob_flags(knobs)
    if flow != FLOW_AUTO:
        flags["flow"] = flow
    return Case(name, setup, call_product("bspgemm_multiply"), read, expect, flags=flags, auto=flow == FLOW_AUTO)


def small_case():
    a = memo("small_a", lambda: gen.uniform_rect(8, 16, 2, 5))
    b = memo("small_b", lambda: gen.uniform_rect(16, 64, 3, 6))

    def setup(env):
        env.option("small_path", 1)
        return dict(A=env.upload(a[0], a[1], 16), B=env.upload(b[0], b[1], 64), r0=0, r1=8)

    return Case("multiply-small", setup, call_product("bspgemm_multiply"), lambda env, inp, out: env.result(out.handles["C"][1]),
                lambda: O.spgemm_rows(a[0], a[1], b[0], b[1], 64, 0, 8), flags=dict(small_path=1))


RANK_COLS = (1 << 18) + 4096


def rank_case():
    def shape():
        return gen.rank_rows(RANK_COLS, [3000, 5000, 2049, 100, 700, 0, 6144], seed=5, counts=(60, 40, 20))

    def setup(env):
        a_rp, a_ci, b_rp, b_ci = memo("rank", shape)
        env.option("small_path", 0)
        env.flow(FLOW_UB)
        return dict(A=env.upload(a_rp, a_ci, 120), B=env.upload(b_rp, b_ci, RANK_COLS), r0=0, r1=7)

    def expect():
        a_rp, a_ci, b_rp, b_ci = memo("rank", shape)
        bins = gen.expected_bins(gen.row_products(a_rp, a_ci, b_rp, 0, 7), RANK_COLS)
        assert bins[gen.RANK_BIN] == 4
        return O.spgemm_rows(a_rp, a_ci, b_rp, b_ci, RANK_COLS, 0, 7) + (bins,)

    def read(env, inp, out):
        return env.result(out.handles["C"][1]) + (env.stats()["rows_per_bin"],)

    return Case("multiply-rank", setup, call_product("bspgemm_multiply"), read, expect, flags=dict(flow=FLOW_UB))


def masked_case(name, fn_name, mode, ex_flags=None):
    a_rp, a_ci, b_rp, b_ci = mixed()
    counted = mode == "count"

    def setup(env):
        env.option("small_path", 0)
        f_rp, f_ci = mask()
        return dict(A=env.upload(a_rp, a_ci, 512), B=env.upload(b_rp, b_ci, NCOLS), F=env.upload(f_rp, f_ci, NCOLS), r0=R0, r1=R1)

    def expect():
        ref = product_ref(a_rp, a_ci, b_rp, b_ci, NCOLS, R0, R1, mode, mask())
        return ref if counted else ref[:2]

    def read(env, inp, out):
        return env.result(out.handles["C"][1], values=counted)

    return Case(name, setup, call_product(fn_name, with_f=True, ex_flags=ex_flags), read, expect, flags=dict(flow=FLOW_UB))


def call_to_matrix(fn):
    """fn(env, inp, byref(out)) -> status, for the entry points that return one operand"""
    return call_to_handle("m", "M", fn)


def read_matrix(env, inp, out):
    return env.matrix(out.handles["M"][1])


def unsorted(seed, n=200):
    return memo(("unsorted", seed, n), lambda: gen.dups_unsorted(n, 6, seed))


def canonical(seed, n=200):
    return memo(("canonical", seed, n), lambda: gen.uniform(n, 5, seed))


def upload_case():
    a_rp, a_ci, _, _ = mixed()

    def call(env, inp, out):
        return L().bspgemm_matrix_upload(env.ctx, R1 - R0, 512, a_rp.ctypes.data + 4 * R0, a_ci.ctypes.data, out)

    def expect():
        return (a_rp[R0:R1 + 1] - a_rp[R0]).astype(np.int32), a_ci[a_rp[R0]:a_rp[R1]]

    return Case("upload-interior", lambda env: {}, call_to_matrix(call), read_matrix, expect)


def product_setup(counted):
    """the operands of the mixed product and its result (masked and counted, or plain), made unarmed"""
    a_rp, a_ci, b_rp, b_ci = mixed()

    def setup(env):
        env.option("small_path", 0)
        inp = dict(A=env.upload(a_rp, a_ci, 512), B=env.upload(b_rp, b_ci, NCOLS), r0=R0, r1=R1)
        if counted:
            inp["F"] = env.upload(*mask(), NCOLS)
        out = call_product("bspgemm_multiply_masked_count" if counted else "bspgemm_multiply", with_f=counted)(env, inp)
        assert out.status == OK, last_error()
        inp["C"] = out.handles["C"][1]
        return inp
    return setup


def from_result_case():
    a_rp, a_ci, b_rp, b_ci = mixed()

    def expect():
        rp, ci = O.spgemm_rows(a_rp, a_ci, b_rp, b_ci, NCOLS, R0, R1)
        return rp.astype(np.int32), ci

    return Case("from_result", product_setup(False),
                call_to_matrix(lambda env, inp, out: L().bspgemm_matrix_from_result(env.ctx, inp["C"], NCOLS, out)), read_matrix, expect)


def from_result_where_case():
    a_rp, a_ci, b_rp, b_ci = mixed()

    def expect():
        rp, ci, v = product_ref(a_rp, a_ci, b_rp, b_ci, NCOLS, R0, R1, "count", mask())
        assert 0 < (v >= 2).sum() < v.size
        return ktruss_ref.where_ref(rp, ci, v, ">=", 2)

    return Case("from_result_where", product_setup(True),
                call_to_matrix(lambda env, inp, out: L().bspgemm_matrix_from_result_where(env.ctx, inp["C"], NCOLS, bspgemm.COMPARES[">="], 2, out)),
                read_matrix, expect)


def transpose_case():
    a = memo("tr", lambda: gen.uniform_rect(100, 300, 6, 31))      # 300 columns: two digit passes, both key/value pairs

    return Case("transpose", lambda env: dict(A=env.upload(a[0], a[1], 300)),
                call_to_matrix(lambda env, inp, out: L().bspgemm_matrix_transpose(env.ctx, inp["A"], out)), read_matrix,
                lambda: setop_ref.transpose_ref(a[0], a[1], 100, 300))


def select_case():
    rp, ci, n = unsorted(11)
    return Case("select", lambda env: dict(A=env.upload(rp, ci, n)),
                call_to_matrix(lambda env, inp, out: L().bspgemm_matrix_select(env.ctx, inp["A"], bspgemm.SELECT_OPS["tril"], out)),
                read_matrix, lambda: ktruss_ref.select_ref(rp, ci, "tril"))


def setop_case(op, tidy):
    (a_rp, a_ci, n), (b_rp, b_ci, _) = (canonical(21), canonical(22)) if tidy else (unsorted(21), unsorted(22))
    return Case("setop-%s-%s" % (op, "canonical" if tidy else "unsorted"),
                lambda env: dict(A=env.upload(a_rp, a_ci, n), B=env.upload(b_rp, b_ci, n)),
                call_to_matrix(lambda env, inp, out: L().bspgemm_matrix_setop(env.ctx, inp["A"], inp["B"], bspgemm.SETOPS[op], out)),
                read_matrix, lambda: setop_ref.setop_ref(a_rp, a_ci, b_rp, b_ci, n, n, op))


def equal_case():
    rp, ci, n = unsorted(23)

    def setup(env):
        c_rp, c_ci = setop_ref.canonical_ref(rp, ci, n, n)
        return dict(A=env.upload(rp, ci, n), B=env.upload(c_rp, c_ci, n))

    def call(env, inp):
        eq = C.c_int(77)
        return Out(L().bspgemm_matrix_equal(env.ctx, inp["A"], inp["B"], C.byref(eq)), scalars={"equal": eq})

    return Case("equal", setup, call, lambda env, inp, out: (out.scalars["equal"].value,), lambda: (1,), failed={"equal": 77})


def symmetrize_case():
    rp, ci, n = unsorted(24)
    return Case("symmetrize", lambda env: dict(A=env.upload(rp, ci, n)),
                call_to_matrix(lambda env, inp, out: L().bspgemm_matrix_symmetrize(env.ctx, inp["A"], bspgemm.SYMMETRIZE_DROP_DIAGONAL, out)),
                read_matrix, lambda: setop_ref.symmetrize_ref(rp, ci, n, drop_diagonal=True))


def undirected(seed, n=120, d=5):
    def make():
        rp, ci, _ = gen.uniform(n, d, seed)
        return ktruss_ref.symmetrise(rp, ci, n) + (n,)
    return memo(("undirected", seed, n, d), make)


def triangle_case():
    rp, ci, n = undirected(3)

    def call(env, inp):
        t = C.c_int64(-77)
        return Out(L().bspgemm_triangle_count(env.ctx, inp["A"], C.byref(t)), scalars={"triangles": t})

    def expect():
        t = ktruss_ref.triangles_ref(rp, ci, n)
        assert t > 0
        return (t,)

    return Case("triangle_count", lambda env: dict(A=env.upload(rp, ci, n)), call, lambda env, inp, out: (out.scalars["triangles"].value,),
                expect, failed={"triangles": -77})


def ktruss_case():
    rp, ci, n = undirected(1)

    def call(env, inp):
        m, it, conv = VP(SENTINEL), C.c_int(-1), C.c_int(-1)
        st = L().bspgemm_ktruss(env.ctx, inp["A"], 4, 0, C.byref(m), C.byref(it), C.byref(conv))
        if st == OK and m.value not in (None, SENTINEL):
            env.mat(m)
        return Out(st, {"T": ("m", m)}, {"iterations": it, "converged": conv})

    def expect():
        (t_rp, t_ci), it, conv = ktruss_ref.ktruss_ref(rp, ci, n, 4)
        assert it >= 3 and t_ci.size > 0, "the k-truss graph needs at least three steps"
        return t_rp, t_ci, it, int(conv)

    def read(env, inp, out):
        return env.matrix(out.handles["T"][1]) + (out.scalars["iterations"].value, out.scalars["converged"].value)

    return Case("ktruss", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect, failed={"converged": 0})


def bfs_case(check):
    def graph():
        rp, ci, n, ids = bfs_ref.layered([1, 4, 9, 12, 6], 5, 17)
        return rp, ci, n, np.array([ids[0][0], ids[1][0], ids[2][0]], np.int32)

    def setup(env):
        rp, ci, n, src = memo("bfs", graph)
        env.option("check", 1 if check else 0)
        return dict(A=env.upload(rp, ci, n), src=src)

    def call(env, inp):
        r, depth, complete = VP(SENTINEL), C.c_int(-1), C.c_int(-1)
        src = inp["src"]
        st = L().bspgemm_bfs(env.ctx, inp["A"], src.size, src.ctypes.data, 0, C.byref(r), C.byref(depth), C.byref(complete))
        if st == OK and r.value not in (None, SENTINEL):
            env.res(r)
        return Out(st, {"levels": ("r", r)}, {"depth": depth, "complete": complete})

    def expect():
        rp, ci, n, src = memo("bfs", graph)
        (l_rp, l_ci, l_v), depth, complete = bfs_ref.bfs_ref(rp, ci, n, src)
        assert depth >= 3
        return l_rp, l_ci, l_v, depth, complete

    def read(env, inp, out):
        return env.result(out.handles["levels"][1], values=True) + (out.scalars["depth"].value, out.scalars["complete"].value)

    return Case("bfs-check" if check else "bfs", setup, call, read, expect, failed={"depth": 0, "complete": 0})


def cc_case():
    rp, ci, n = memo("cc", lambda: cc_ref.untidy(150, 9))

    def call(env, inp):
        m, nc, rounds = VP(SENTINEL), C.c_int(-1), C.c_int(-1)
        st = L().bspgemm_connected_components(env.ctx, inp["A"], C.byref(m), C.byref(nc), C.byref(rounds))
        if st == OK and m.value not in (None, SENTINEL):
            env.mat(m)
        return Out(st, {"P": ("m", m)}, {"ncomponents": nc, "rounds": rounds})

    def expect():
        label, ncomp = cc_ref.labels(rp, ci, n)
        assert 1 < ncomp < n
        return np.arange(n + 1, dtype=np.int32), label, ncomp

    def read(env, inp, out):
        return env.matrix(out.handles["P"][1]) + (out.scalars["ncomponents"].value,)

    return Case("connected_components", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect,
                failed={"ncomponents": 0, "rounds": 0})


def core_graph():
    return memo("core", lambda: kcore_ref.cliques([2, 4, 6, 3]))         # core values 1, 3, 5, 2


def core_numbers_case():
    rp, ci, n = core_graph()

    def call(env, inp):
        r, top, rounds = VP(SENTINEL), C.c_int(-1), C.c_int(-1)
        st = L().bspgemm_core_numbers(env.ctx, inp["A"], C.byref(r), C.byref(top), C.byref(rounds))
        if st == OK and r.value not in (None, SENTINEL):
            env.res(r)
        return Out(st, {"cores": ("r", r)}, {"degeneracy": top, "rounds": rounds})

    def expect():
        core, top, rounds = kcore_ref.core_numbers(rp, ci, n)
        assert np.unique(core).size >= 3
        return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), core, top, rounds

    def read(env, inp, out):
        return env.result(out.handles["cores"][1], values=True) + (out.scalars["degeneracy"].value, out.scalars["rounds"].value)

    return Case("core_numbers", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect, failed={"degeneracy": 0, "rounds": 0})


def kcore_case():
    rp, ci, n = core_graph()

    def call(env, inp):
        m, top = VP(SENTINEL), C.c_int(-1)
        st = L().bspgemm_kcore(env.ctx, inp["A"], 3, C.byref(m), C.byref(top))
        if st == OK and m.value not in (None, SENTINEL):
            env.mat(m)
        return Out(st, {"T": ("m", m)}, {"degeneracy": top})

    def expect():
        t_rp, t_ci = kcore_ref.kcore(rp, ci, n, 3)
        assert 0 < t_ci.size < kcore_ref.simple(rp, ci, n)[1].size
        return t_rp, t_ci, kcore_ref.core_numbers(rp, ci, n)[1]

    def read(env, inp, out):
        return env.matrix(out.handles["T"][1]) + (out.scalars["degeneracy"].value,)

    return Case("kcore", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect, failed={"degeneracy": 0})


def closure_case(transitive):
    rp, ci, n = memo("closure", lambda: bfs_ref.path(12))

    def call(env, inp):
        r, it = VP(SENTINEL), C.c_int(-1)
        if transitive:
            st = L().bspgemm_closure_ex(env.ctx, inp["A"], bspgemm.CLOSURE_TRANSITIVE, 64, C.byref(r), C.byref(it))
        else:
            st = L().bspgemm_closure(env.ctx, inp["A"], 64, C.byref(r), C.byref(it))
        if st == OK and r.value not in (None, SENTINEL):
            env.res(r)
        return Out(st, {"T": ("r", r)}, {"iterations": it})

    def expect():
        T = _ones(rp, ci, (n, n))
        if not transitive:
            T = T + sp.identity(n, dtype=np.int64, format="csr")
        while True:                                       # A* (A+): reachability by paths of length >= 0 (>= 1)
            N = (T + T @ T).tocsr()
            N.data[:] = 1
            if N.nnz == T.nnz:
                break
            T = N
        T.sort_indices()
        return T.indptr.astype(np.int64), T.indices.astype(np.int32)

    def read(env, inp, out):
        assert out.scalars["iterations"].value >= 3
        return env.result(out.handles["T"][1])

    return Case("closure_ex-transitive" if transitive else "closure", lambda env: dict(A=env.upload(rp, ci, n)), call, read, expect)


def partition_ref(prefix, R, parts):
    """include/bspgemm.h: a row costs its products + 32; bounds[p] = the first row at which the cost reaches p / parts"""
    cost = prefix + 32 * np.arange(R + 1)
    total = int(cost[R])
    return [0] + [int(np.searchsorted(cost[:R], total // parts * p, side="left")) for p in range(1, parts)] + [R]


def sharding_case(partition):
    a_rp, a_ci, b_rp, b_ci = mixed()
    R = a_rp.size - 1

    def setup(env):
        return dict(A=env.upload(a_rp, a_ci, 512), B=env.upload(b_rp, b_ci, NCOLS))

    def call(env, inp):
        if partition:
            out = np.full(5, -1, np.int32)
            st = L().bspgemm_partition_rows(env.ctx, inp["A"], inp["B"], 4, out)
        else:
            out = np.full(R + 1, -1, np.int64)
            st = L().bspgemm_row_work_prefix(env.ctx, inp["A"], inp["B"], out)
        o = Out(st)
        o.array = out
        return o

    def expect():
        prefix = np.concatenate([[0], np.cumsum(gen.row_products(a_rp, a_ci, b_rp, 0, R))])
        return (partition_ref(prefix, R, 4),) if partition else (prefix,)

    return Case("partition_rows" if partition else "row_work_prefix", setup, call, lambda env, inp, out: (out.array,), expect)


CASES = {
    "multiply": [multiply_case("multiply-auto", FLOW_AUTO, False), multiply_case("multiply-upper-bound", FLOW_UB, False),
                 multiply_case("multiply-exact", FLOW_EXACT, False), multiply_case("multiply-auto-knobs", FLOW_AUTO, True),
                 multiply_case("multiply-upper-bound-knobs", FLOW_UB, True), multiply_case("multiply-exact-knobs", FLOW_EXACT, True),
                 small_case(), rank_case()],
    "masked": [masked_case("masked", "bspgemm_multiply_masked", "keep"),
               masked_case("masked_ex-complement", "bspgemm_multiply_masked_ex", "drop", ex_flags=bspgemm.MASK_COMPLEMENT),
               masked_case("accumulate", "bspgemm_multiply_accumulate", "insert"),
               masked_case("masked_count", "bspgemm_multiply_masked_count", "count")],
    "operands": [upload_case(), from_result_case(), from_result_where_case(), transpose_case(), select_case(),
                 setop_case("or", False), setop_case("xor", False), setop_case("or", True), setop_case("xor", True), equal_case(),
                 symmetrize_case()],
    "loops": [triangle_case(), ktruss_case(), bfs_case(False), bfs_case(True), cc_case(), core_numbers_case(), kcore_case(),
              closure_case(False), closure_case(True), sharding_case(False), sharding_case(True)],
}


# An armed call that succeeds made the failed request again and nothing else (cold + 1 requests, measured on an MI355X),
# but for bfs: at k = 25 and 26 its armed call makes cold + 2.
for _case in sum(CASES.values(), []):
    _case.cap = 2 * COLD[_case.name]
    _case.strict_requests = _case.name not in ("bfs", "bfs-check")


def _params(family):
    return [pytest.param(c, id=c.name) for c in CASES[family]]


@pytest.mark.parametrize("case", _params("multiply"))
def test_multiply_alloc_failures(case):
    sweep(case)


@pytest.mark.parametrize("case", _params("masked"))
def test_masked_alloc_failures(case):
    sweep(case)


@pytest.mark.parametrize("case", _params("operands"))
def test_operands_alloc_failures(case):
    sweep(case)


@pytest.mark.parametrize("case", _params("loops"))
def test_loops_alloc_failures(case):
    sweep(case)


def test_create_alloc_failures():
    """bspgemm_create itself: a status, *ctx == NULL, and nothing of the half-built context left"""
    gc.collect()
    L().bspgemm_debug_fail_alloc(0)
    base = alloc_state()
    failed, t_create = [], None
    for k in range(1, 2 * COLD["create"] + 1):
        ctx = VP(SENTINEL)
        before = alloc_state()
        L().bspgemm_debug_fail_alloc(k)
        t0 = time.time()
        st = L().bspgemm_create(0, C.byref(ctx))
        t_create = time.time() - t0
        L().bspgemm_debug_fail_alloc(0)
        fired = alloc_state()[3] - before[3]
        if fired:
            assert st == ERR_ALLOC and ctx.value is None and last_error(), "k=%d: status %d, ctx %r" % (k, st, ctx.value)
            failed.append(k)
        else:
            assert st == OK and ctx.value not in (None, SENTINEL), last_error()
            cold = alloc_state()[0] - before[0]
            L().bspgemm_destroy(ctx)
        assert alloc_state()[1:3] == base[1:3], "k=%d: live (count, bytes) %r, before %r" % (k, alloc_state()[1:3], base[1:3])
        if not fired:
            break
    else:
        pytest.fail("the hook still fires at k = %d" % (2 * COLD["create"]))
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  one create + destroy %.3f s" % ("create", cold, failed, t_create))
    assert failed == list(range(1, cold + 1))
    env = Env()                                          # and the process goes on: a context after the failures works
    env.close()
    assert alloc_state()[1:3] == base[1:3]


# ------------------------------------------------------------------ the int32 drop-ins ---------------------------------
IPP = C.POINTER(C.c_int)
_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]
_libc.free.argtypes = [C.c_void_p]


def dropin_call(name, rp, ci, n, f):
    """one call: (status, Crow, col_idx copy or None, whether *Ccol is what the contract says after a failure)"""
    crow = np.zeros(n + 1, np.int32)
    if name == "SpGEMM_hip":
        cc = IPP()
        st = L().SpGEMM_hip(ci, rp.ctypes.data, n, ci, rp, n, C.byref(cc), crow, 0)
        kept = not cc                                    # *Ccol == NULL after a failure
    elif name == "SpGEMM_hip_mat":
        nnz = int(f)
        buf = np.full(max(nnz, 1), -1, np.int32)
        st = L().SpGEMM_hip_mat(ci, rp, n, ci, rp, n, buf, crow)
        return st, crow, buf[:nnz].copy() if st == OK else None, True
    else:
        mine = _libc.malloc(64)                          # too small: a successful call has to grow it
        cc, csize = C.cast(mine, IPP), C.c_int(16)
        if name == "SpGEMM_hip_bigslice":
            st = L().SpGEMM_hip_bigslice(ci, rp, n, ci, rp, n, C.byref(cc), crow, C.byref(csize), 0, n)
        else:
            st = L().SpGEMM_hip_masked(ci, rp, n, ci, rp, n, f[1], f[0], C.byref(cc), crow, C.byref(csize))
        kept = C.cast(cc, C.c_void_p).value == mine and csize.value == 16   # neither freed nor moved after a failure
    col = None
    if st == OK:
        col = np.ctypeslib.as_array(cc, shape=(max(int(crow[-1]), 1),))[:int(crow[-1])].copy()
    if cc:
        _libc.free(C.cast(cc, C.c_void_p))
    return st, crow, col, kept


@pytest.mark.parametrize("name", ["SpGEMM_hip", "SpGEMM_hip_bigslice", "SpGEMM_hip_mat", "SpGEMM_hip_masked"])
def test_dropin_alloc_failures(name):
    """The drop-ins' context is process-wide: no destroy.  The leak check compares the live count after a failed call plus
    one successful repeat with the live count after two successful calls."""
    rp, ci, n = memo("dropin", lambda: gen.uniform(300, 5, 13))
    f_rp, f_ci = memo("dropin_mask", lambda: gen.uniform_rect(300, 300, 40, 14))
    e_rp, e_ci = memo("dropin_ref", lambda: O.spgemm(rp, ci, rp, ci, n))
    if name == "SpGEMM_hip_masked":
        m_rp, m_ci, _ = product_ref(rp, ci, rp, ci, n, 0, n, "keep", (f_rp, f_ci))
        want, f = (m_rp.astype(np.int32), m_ci), (f_rp, f_ci)
    else:
        want, f = (e_rp.astype(np.int32), e_ci), e_ci.size
    gc.collect()
    L().bspgemm_debug_fail_alloc(0)
    t0 = time.time()

    def good(what):
        st, crow, col, _ = dropin_call(name, rp, ci, n, f)
        assert st == OK, "%s %s: status %d (%s)" % (name, what, st, last_error())
        assert same((crow, col), want), "%s %s: the result differs from the reference" % (name, what)

    good("warm-up")                                      # (creates the process-wide context on first use)
    good("first")
    good("second")
    steady = alloc_state()[1:3]
    failed, cold = [], None
    for k in range(1, 2 * COLD[name] + 1):
        before = alloc_state()
        L().bspgemm_debug_fail_alloc(k)
        st, crow, col, kept = dropin_call(name, rp, ci, n, f)
        L().bspgemm_debug_fail_alloc(0)
        fired = alloc_state()[3] - before[3]
        if not fired:
            assert st == OK and same((crow, col), want), "%s k=%d (hook not reached): status %d" % (name, k, st)
            cold = alloc_state()[0] - before[0]
            break
        if st == OK:                                     # (the retry after dropping the result cache)
            assert same((crow, col), want), "%s k=%d armed: the result differs from the reference" % (name, k)
        else:
            assert st == ERR_ALLOC, "%s k=%d: status %d (%s)" % (name, k, st, last_error())
            assert kept, "%s k=%d: *Ccol after a failure is not what the caller is promised" % (name, k)
            assert last_error()
            failed.append(k)
        good("k=%d repeated" % k)
        assert alloc_state()[1:3] == steady, ("%s k=%d: live (count, bytes) %r after the failed call and a repeat, %r after two "
                                              "successful calls" % (name, k, alloc_state()[1:3], steady))
    else:
        pytest.fail("%s: the hook still fires at k = %d" % (name, 2 * COLD[name]))
    print("ALLOCSWEEP %-28s cold %3d  ERR_ALLOC at %s  %.2f s" % (name, cold, failed, time.time() - t0))
    assert failed, "%s: no k ended in BSPGEMM_ERR_ALLOC" % name
