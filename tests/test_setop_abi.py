"""The on-device set operations, pattern equality and symmetrize at the ABI level, without a GPU: the header declares them
with the agreed argument lists, the library exports them, the Python view has them, a C99 caller compiles cleanly, NULL
arguments are refused by name -- and the tests' own reference (setop_ref.py) agrees with scipy and with ktruss_ref.
"""
import ctypes as C
import re

import numpy as np
import scipy.sparse as sp

import bspgemm
import gen
import ktruss_ref
from setop_ref import canonical_ref, setop_ref, symmetrize_ref, transpose_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, compile_c99, last_error


DECLARATIONS = {
    "bspgemm_matrix_setop":
        "bspgemm_status bspgemm_matrix_setop(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, "
        "bspgemm_setop op, bspgemm_matrix **out);",
    "bspgemm_matrix_equal":
        "bspgemm_status bspgemm_matrix_equal(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *B, int *equal);",
    "bspgemm_matrix_symmetrize":
        "bspgemm_status bspgemm_matrix_symmetrize(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags, "
        "bspgemm_matrix **out);",
}
NAMES = sorted(DECLARATIONS)


def test_header_declares_the_functions_and_the_enum():
    code = header_code()
    for name, decl in DECLARATIONS.items():
        assert re.sub(r"\s+", " ", decl) in code, "include/bspgemm.h does not declare %s as agreed" % name
    m = re.search(r"typedef enum bspgemm_setop \{(.*?)\} bspgemm_setop;", code)
    assert m, "bspgemm_setop"
    assert re.sub(r"\s", "", m.group(1)) == "BSPGEMM_SETOP_OR=1,BSPGEMM_SETOP_AND=2,BSPGEMM_SETOP_ANDNOT=3,BSPGEMM_SETOP_XOR=4"
    assert "#define BSPGEMM_SYMMETRIZE_DROP_DIAGONAL 1u" in code
    # after bspgemm_matrix_from_result_where, beside the selects
    assert code.index("bspgemm_matrix_from_result_where(") < code.index("bspgemm_matrix_setop(")


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    for name in NAMES:
        assert hasattr(L, name), "%s is not exported by libbspgemm.so" % name
        assert name in bspgemm.EXPORTS, "%s is missing from bspgemm.EXPORTS" % name
        assert getattr(L, name).argtypes, "%s has no argtypes" % name
    for method in ("setop", "matrix_equal", "symmetrize"):
        assert callable(getattr(bspgemm.Context, method, None)), "Context.%s" % method
    assert bspgemm.SETOPS == {"or": 1, "and": 2, "andnot": 3, "xor": 4}


C99_CALLER = r"""
#include "bspgemm.h"
/* a directed graph to its undirected truss, with the four set operations and the comparison on the way */
int truss_of_directed(bspgemm_context *ctx, const bspgemm_matrix *A, int k, int64_t *sizes)
{
    static const bspgemm_setop ops[4] = { BSPGEMM_SETOP_OR, BSPGEMM_SETOP_AND, BSPGEMM_SETOP_ANDNOT, BSPGEMM_SETOP_XOR };
    bspgemm_matrix *S = 0, *AT = 0, *R[4] = { 0, 0, 0, 0 }, *T = 0;
    int i, equal = 0, iterations = 0, converged = 0;
    if (bspgemm_matrix_symmetrize(ctx, A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL, &S) != BSPGEMM_OK) return 1;
    if (bspgemm_matrix_transpose(ctx, A, &AT) != BSPGEMM_OK) return 1;
    for (i = 0; i < 4; i++) {
        if (bspgemm_matrix_setop(ctx, A, AT, ops[i], &R[i]) != BSPGEMM_OK) return 1;
        sizes[i] = bspgemm_matrix_nnz(R[i]);
    }
    if (bspgemm_matrix_equal(ctx, R[0], S, &equal) != BSPGEMM_OK) return 1;
    if (bspgemm_ktruss(ctx, R[0], k, 0, &T, &iterations, &converged) != BSPGEMM_OK) return 1;
    for (i = 0; i < 4; i++) bspgemm_matrix_free(R[i]);
    bspgemm_matrix_free(T);
    bspgemm_matrix_free(AT);
    bspgemm_matrix_free(S);
    return converged && equal ? 0 : iterations;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        out = C.c_void_p(sentinel)
        assert L.bspgemm_matrix_setop(args[0], args[1], args[2], 1, C.byref(out)) == ERR_INVALID
        assert not out.value and "bspgemm_matrix_setop" in last(), last()
        eq = C.c_int(sentinel)
        assert L.bspgemm_matrix_equal(args[0], args[1], args[2], C.byref(eq)) == ERR_INVALID
        assert eq.value == sentinel and "bspgemm_matrix_equal" in last(), last()
    for args in ((None, fake), (fake, None)):
        out = C.c_void_p(sentinel)
        assert L.bspgemm_matrix_symmetrize(args[0], args[1], 0, C.byref(out)) == ERR_INVALID
        assert not out.value and "bspgemm_matrix_symmetrize" in last(), last()
    # NULL result pointers
    assert L.bspgemm_matrix_setop(fake, fake, fake, 1, None) == ERR_INVALID and "bspgemm_matrix_setop" in last()
    assert L.bspgemm_matrix_equal(fake, fake, fake, None) == ERR_INVALID and "bspgemm_matrix_equal" in last()
    assert L.bspgemm_matrix_symmetrize(fake, fake, 0, None) == ERR_INVALID and "bspgemm_matrix_symmetrize" in last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def _pattern(rp, ci, rows, cols):
    M = sp.csr_matrix((np.ones(np.asarray(ci).size, np.int64), np.array(ci), np.array(rp)), shape=(rows, cols))   # copies
    M.sum_duplicates()
    M.sort_indices()
    M.data[:] = 1
    return M


def _csr_of(M):
    M = M.tocsr()
    M.eliminate_zeros()
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.tolist(), M.indices.tolist()


def test_setop_ref_equals_scipy_on_a_hand_example():
    rows, cols = 4, 6
    a_rp, a_ci = np.array([0, 4, 4, 7, 9], np.int32), np.array([5, 0, 0, 3, 2, 1, 2, 4, 4], np.int32)   # unsorted, repeats
    b_rp, b_ci = np.array([0, 2, 3, 3, 7], np.int32), np.array([3, 1, 2, 4, 0, 5, 4], np.int32)
    A, B = _pattern(a_rp, a_ci, rows, cols), _pattern(b_rp, b_ci, rows, cols)
    both = A.multiply(B)
    expected = {"or": A + B, "and": both, "andnot": A - both, "xor": A + B - 2 * both}
    for op, M in expected.items():
        got = setop_ref(a_rp, a_ci, b_rp, b_ci, rows, cols, op)
        assert [got[0].tolist(), got[1].tolist()] == list(_csr_of(M)), op
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert [a.tolist() for a in setop_ref(a_rp, a_ci, b_rp, b_ci, rows, cols, "or")] == \
        [[0, 4, 5, 7, 10], [0, 1, 3, 5, 2, 1, 2, 0, 4, 5]]
    assert [a.tolist() for a in canonical_ref(a_rp, a_ci, rows, cols)] == [[0, 3, 3, 5, 6], [0, 3, 5, 1, 2, 4]]
    assert list(_csr_of(A.T)) == [a.tolist() for a in transpose_ref(a_rp, a_ci, rows, cols)]
    # degenerate shapes
    z = np.zeros(1, np.int32)
    assert [a.tolist() for a in setop_ref(z, [], z, [], 0, 0, "or")] == [[0], []]
    assert [a.tolist() for a in setop_ref([0, 0, 0], [], [0, 1, 1], [0], 2, 1, "xor")] == [[0, 1, 1], [0]]


def test_symmetrize_ref_equals_ktruss_ref():
    for rp, ci, n in (gen.rmat(8, 12, (0.57, 0.19, 0.19, 0.05), 8101), gen.dups_unsorted(300, 7, 8102)):
        s = symmetrize_ref(rp, ci, n, drop_diagonal=True)
        e = ktruss_ref.symmetrise(rp, ci, n)
        assert np.array_equal(s[0], e[0]) and np.array_equal(s[1], e[1])
        # with the diagonal: the same plus A's diagonal entries
        full = symmetrize_ref(rp, ci, n)
        rows = np.repeat(np.arange(n), np.diff(rp))
        assert full[1].size == s[1].size + np.unique(rows[rows == ci]).size
