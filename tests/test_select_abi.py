"""The on-device select, value sum, triangle count and k-truss at the ABI level, without a GPU: the header declares them
with the agreed argument lists, the library exports them, the Python view has them, a C99 caller of the k-truss loop
compiles cleanly, a NULL context is refused by name -- and the tests' own references (ktruss_ref.py) agree with networkx.
"""
import ctypes as C
import re

import numpy as np
import pytest

import bspgemm
import gen
import ktruss_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, compile_c99, last_error


DECLARATIONS = {
    "bspgemm_matrix_select":
        "bspgemm_status bspgemm_matrix_select(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_select op, bspgemm_matrix **out);",
    "bspgemm_matrix_from_result_where":
        "bspgemm_status bspgemm_matrix_from_result_where(bspgemm_context *ctx, const bspgemm_result *C, int cols, "
        "bspgemm_compare cmp, int threshold, bspgemm_matrix **out);",
    "bspgemm_result_values_sum":
        "bspgemm_status bspgemm_result_values_sum(bspgemm_context *ctx, const bspgemm_result *C, int64_t *sum);",
    "bspgemm_triangle_count":
        "bspgemm_status bspgemm_triangle_count(bspgemm_context *ctx, const bspgemm_matrix *A, int64_t *triangles);",
    "bspgemm_ktruss":
        "bspgemm_status bspgemm_ktruss(bspgemm_context *ctx, const bspgemm_matrix *A, int k, int max_iter, "
        "bspgemm_matrix **T, int *iterations, int *converged);",
}
NAMES = sorted(DECLARATIONS)


def test_header_declares_the_functions_and_enums():
    code = header_code()
    for name, decl in DECLARATIONS.items():
        assert re.sub(r"\s+", " ", decl) in code, "include/bspgemm.h does not declare %s as agreed" % name
    m = re.search(r"typedef enum bspgemm_select \{(.*?)\} bspgemm_select;", code)
    assert m, "bspgemm_select"
    assert re.sub(r"\s", "", m.group(1)) == "BSPGEMM_SELECT_TRIL=1,BSPGEMM_SELECT_TRIU=2,BSPGEMM_SELECT_OFFDIAG=3"
    m = re.search(r"typedef enum bspgemm_compare \{(.*?)\} bspgemm_compare;", code)
    assert m, "bspgemm_compare"
    assert re.sub(r"\s", "", m.group(1)) == \
        "BSPGEMM_CMP_GE=1,BSPGEMM_CMP_GT,BSPGEMM_CMP_LE,BSPGEMM_CMP_LT,BSPGEMM_CMP_EQ,BSPGEMM_CMP_NE"


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    for name in NAMES:
        assert hasattr(L, name), "%s is not exported by libbspgemm.so" % name
        assert name in bspgemm.EXPORTS, "%s is missing from bspgemm.EXPORTS" % name
    for method in ("select", "matrix_from_result_where", "triangle_count", "ktruss"):
        assert callable(getattr(bspgemm.Context, method, None)), "Context.%s" % method
    assert callable(getattr(bspgemm.Result, "values_sum", None)), "Result.values_sum"
    assert bspgemm.SELECT_OPS == {"tril": 1, "triu": 2, "offdiag": 3}
    assert bspgemm.COMPARES == {">=": 1, ">": 2, "<=": 3, "<": 4, "==": 5, "!=": 6}


C99_CALLER = r"""
#include "bspgemm.h"
/* the k-truss loop written against the primitives, and the drivers */
int truss(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int k, int64_t *triangles, int64_t *support)
{
    bspgemm_matrix *S = 0, *next = 0, *T = 0;
    bspgemm_result *C = 0;
    int iterations = 0, converged = 0;
    if (bspgemm_matrix_select(ctx, A, BSPGEMM_SELECT_OFFDIAG, &S) != BSPGEMM_OK) return 1;
    for (;;) {
        if (bspgemm_multiply_masked_count(ctx, S, S, S, 0, n, &C) != BSPGEMM_OK) return 1;
        if (bspgemm_result_values_sum(ctx, C, support) != BSPGEMM_OK) return 1;
        if (bspgemm_matrix_from_result_where(ctx, C, n, BSPGEMM_CMP_GE, k - 2, &next) != BSPGEMM_OK) return 1;
        bspgemm_result_free(C);
        if (bspgemm_matrix_nnz(next) == bspgemm_matrix_nnz(S) || bspgemm_matrix_nnz(next) == 0) break;
        bspgemm_matrix_free(S);
        S = next;
    }
    bspgemm_matrix_free(S);
    bspgemm_matrix_free(next);
    if (bspgemm_triangle_count(ctx, A, triangles) != BSPGEMM_OK) return 1;
    if (bspgemm_ktruss(ctx, A, k, 0, &T, &iterations, &converged) != BSPGEMM_OK) return 1;
    bspgemm_matrix_free(T);
    return converged ? 0 : iterations;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_context_is_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the NULL context is refused first
    sentinel, last = SENTINEL, last_error

    out = C.c_void_p(sentinel)
    assert L.bspgemm_matrix_select(None, fake, 1, C.byref(out)) == ERR_INVALID
    assert not out.value and "bspgemm_matrix_select" in last(), last()
    out = C.c_void_p(sentinel)
    assert L.bspgemm_matrix_from_result_where(None, fake, 10, 1, 1, C.byref(out)) == ERR_INVALID
    assert not out.value and "bspgemm_matrix_from_result_where" in last(), last()
    s = C.c_int64(sentinel)
    assert L.bspgemm_result_values_sum(None, fake, C.byref(s)) == ERR_INVALID
    assert s.value == sentinel and "bspgemm_result_values_sum" in last(), last()
    t = C.c_int64(sentinel)
    assert L.bspgemm_triangle_count(None, fake, C.byref(t)) == ERR_INVALID
    assert t.value == sentinel and "bspgemm_triangle_count" in last(), last()
    out, it, conv = C.c_void_p(sentinel), C.c_int(7), C.c_int(7)
    assert L.bspgemm_ktruss(None, fake, 3, 0, C.byref(out), C.byref(it), C.byref(conv)) == ERR_INVALID
    assert not out.value and "bspgemm_ktruss" in last(), last()
    # NULL operands and NULL result pointers likewise
    assert L.bspgemm_matrix_select(fake, None, 1, C.byref(out)) == ERR_INVALID
    assert L.bspgemm_matrix_select(fake, fake, 1, None) == ERR_INVALID
    assert L.bspgemm_ktruss(fake, None, 3, 0, C.byref(out), None, None) == ERR_INVALID
    assert L.bspgemm_ktruss(fake, fake, 3, 0, None, None, None) == ERR_INVALID


# ---------------------------------------------------------------- the references themselves --------------------------
def test_select_and_where_references_on_a_hand_example():
    rp = np.array([0, 3, 3, 7, 8], np.int32)
    ci = np.array([2, 0, 0, 3, 2, 0, 0, 3], np.int32)          # unsorted rows, repeats, diagonal entries
    assert [a.tolist() for a in ktruss_ref.select_ref(rp, ci, "tril")] == [[0, 0, 0, 2, 2], [0, 0]]
    assert [a.tolist() for a in ktruss_ref.select_ref(rp, ci, "triu")] == [[0, 1, 1, 2, 2], [2, 3]]
    assert [a.tolist() for a in ktruss_ref.select_ref(rp, ci, "offdiag")] == [[0, 1, 1, 4, 4], [2, 3, 0, 0]]
    v = np.array([5, 1, 2, 2, 9, 1, 3, 2], np.int32)
    assert [a.tolist() for a in ktruss_ref.where_ref(rp, ci, v, ">=", 2)] == [[0, 2, 2, 5, 6], [2, 0, 3, 2, 0, 3]]
    assert [a.tolist() for a in ktruss_ref.where_ref(rp, ci, v, "==", 2)] == [[0, 1, 1, 2, 3], [0, 3, 3]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_references_equal_networkx(seed):
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(seed)
    if seed == 3:
        rp, ci, n = gen.rmat(8, 12, (0.57, 0.19, 0.19, 0.05), 40 + seed)
    else:
        rp, ci, n = gen.uniform(150 * seed, 9 + 5 * seed, 40 + seed)
    s_rp, s_ci = ktruss_ref.symmetrise(rp, ci, n)
    rows = np.repeat(np.arange(n), np.diff(s_rp))
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(rows.tolist(), s_ci.tolist()))
    assert ktruss_ref.triangles_ref(s_rp, s_ci, n) == sum(nx.triangles(G).values()) // 3
    # the triangle count reads the strictly lower triangle only: self-loops and repeats on top change nothing
    loops = np.arange(n)
    noisy_rows = np.concatenate([rows, loops, rows[: n]])
    noisy_cols = np.concatenate([s_ci, loops, s_ci[: n]])
    perm = rng.permutation(noisy_rows.size)
    n_rp, n_ci = gen._csr_from_pairs(noisy_rows[perm], noisy_cols[perm], n, dedup=False, sort=False)
    assert ktruss_ref.triangles_ref(n_rp, n_ci, n) == ktruss_ref.triangles_ref(s_rp, s_ci, n)
    for k in (2, 3, 4, 5, 8, 50):
        (t_rp, t_ci), it, conv = ktruss_ref.ktruss_ref(n_rp, n_ci, n, k)
        assert conv and (it == 0) == (k == 2)
        H = nx.k_truss(G, k)
        assert t_ci.size == 2 * H.number_of_edges(), k
        t_rows = np.repeat(np.arange(n), np.diff(t_rp))
        assert {(int(a), int(b)) for a, b in zip(t_rows, t_ci) if a < b} == {(min(a, b), max(a, b)) for a, b in H.edges()}, k
