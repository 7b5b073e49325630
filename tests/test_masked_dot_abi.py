"""CPU-only checks of the masked dot product's C ABI (bspgemm_multiply_masked_dot, bspgemm_triangle_count_ex,
bspgemm_ktruss_ex, bspgemm_dot_info, bspgemm_support_method, BSPGEMM_OPT_DOT_LIGHT): the header declares them with the
documented argument lists, the library exports them, the Python binding lists them, a C caller compiles, a NULL context is
refused, and the scipy model of the product (tests/dot_ref.py) counts triangles through the L-identity."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import bspgemm
import dot_ref
import gen
import ktruss_ref
from abi_kit import ROOT, header_text

NAMES = ("bspgemm_multiply_masked_dot", "bspgemm_triangle_count_ex", "bspgemm_ktruss_ex")


def _code():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def _params(code, ret, name):
    m = re.search(r"%s\s*\*?\s*%s\s*\(([^;]*)\)\s*;" % (ret, name), code)
    assert m, "%s is not declared" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_functions_the_struct_the_enum_and_the_option():
    code = _code()
    p = _params(code, "bspgemm_status", "bspgemm_multiply_masked_dot")
    assert p == ["bspgemm_context *ctx", "const bspgemm_matrix *A", "const bspgemm_matrix *B", "const bspgemm_matrix *F",
                 "unsigned flags", "bspgemm_result **C", "bspgemm_dot_info *info"], p
    p = _params(code, "bspgemm_status", "bspgemm_triangle_count_ex")
    assert p == ["bspgemm_context *ctx", "const bspgemm_matrix *A", "bspgemm_support_method method", "int64_t *triangles"], p
    p = _params(code, "bspgemm_status", "bspgemm_ktruss_ex")
    assert p == ["bspgemm_context *ctx", "const bspgemm_matrix *A", "int k", "int max_iter", "bspgemm_support_method method",
                 "bspgemm_matrix **T", "int *iterations", "int *converged"], p
    flat = " ".join(code.split())
    m = re.search(r"typedef struct bspgemm_dot_info \{(.*?)\} bspgemm_dot_info;", flat)
    assert m, "bspgemm_dot_info is not declared"
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int64_t entries", "int64_t heavy_entries", "int64_t kept", "int canonicalised"], fields
    assert re.search(r"typedef enum bspgemm_support_method \{ BSPGEMM_SUPPORT_PRODUCT = 0, BSPGEMM_SUPPORT_DOT = 1 \} "
                     r"bspgemm_support_method;", flat)
    assert re.search(r"BSPGEMM_OPT_DOT_LIGHT\s*=\s*7\b", flat)
    text = header_text()
    doc = text.split("bspgemm_multiply_masked_dot(bspgemm_context")[0].split("bspgemm_ktruss(bspgemm_context")[-1]
    for word in ("serial tail", "BSPGEMM_ERR_ALLOC", "ONE synchronisation", "bspgemm_multiply_masked_count"):
        assert word in doc, word


def test_library_exports_them_and_the_binding_lists_them():
    L = bspgemm.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in bspgemm.EXPORTS, name
    assert bspgemm.OPTIONS["dot_light"] == 7
    assert bspgemm.SUPPORT_METHODS == {"product": 0, "dot": 1}
    assert callable(bspgemm.Context.multiply_masked_dot)
    assert [f[0] for f in bspgemm.DotInfo._fields_] == ["entries", "heavy_entries", "kept", "canonicalised"]
    assert C.sizeof(bspgemm.DotInfo) == 32
    import inspect
    for fn in (bspgemm.Context.triangle_count, bspgemm.Context.ktruss):
        assert inspect.signature(fn).parameters["method"].default == "product"


def test_c_caller_compiles():
    src = r'''#include <stddef.h>
#include "bspgemm.h"
long long triangles_by_dot(bspgemm_context *ctx, const bspgemm_matrix *L, const bspgemm_matrix *A, bspgemm_matrix **T)
{
    bspgemm_result *C = NULL;
    bspgemm_dot_info info;
    int64_t sum = 0, tri = 0;
    int it = 0, conv = 0;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_DOT_LIGHT, 16) != BSPGEMM_OK) return -1;
    if (bspgemm_multiply_masked_dot(ctx, L, L, L, 0u, &C, &info) != BSPGEMM_OK) return -1;
    if (info.kept != bspgemm_result_nnz(C) || info.heavy_entries > info.entries || info.canonicalised != 0) sum = -2;
    else if (bspgemm_result_values_sum(ctx, C, &sum) != BSPGEMM_OK) sum = -3;
    bspgemm_result_free(C);
    if (bspgemm_triangle_count_ex(ctx, A, BSPGEMM_SUPPORT_DOT, &tri) != BSPGEMM_OK || tri != sum) return -4;
    if (bspgemm_ktruss_ex(ctx, A, 4, 0, BSPGEMM_SUPPORT_PRODUCT, T, &it, &conv) != BSPGEMM_OK) return -5;
    return sum;
}
'''
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.c")
        open(path, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", path,
                        "-o", os.path.join(d, "t.o")], check=True)


def test_null_context_is_invalid_and_hands_back_nothing():
    L = bspgemm.lib()
    for F in (None, C.c_void_p(8)):    # (the context is checked before any operand is looked at)
        out, info = C.c_void_p(1), bspgemm.DotInfo(5, 5, 5, 5)
        assert L.bspgemm_multiply_masked_dot(None, None, None, F, 0, C.byref(out), C.byref(info)) == 1
        assert not out.value
        assert info.as_dict() == {"entries": 0, "heavy_entries": 0, "kept": 0, "canonicalised": 0}
        assert b"bspgemm_multiply_masked_dot" in L.bspgemm_last_error()
    for method in (0, 1):
        tri = C.c_int64(-7)
        assert L.bspgemm_triangle_count_ex(None, None, method, C.byref(tri)) == 1 and tri.value == -7
        T, it, conv = C.c_void_p(1), C.c_int(9), C.c_int(9)
        assert L.bspgemm_ktruss_ex(None, None, 4, 0, method, C.byref(T), C.byref(it), C.byref(conv)) == 1
        assert not T.value and (it.value, conv.value) == (0, 0)
    # an unknown method is refused before anything else is looked at
    T = C.c_void_p(1)
    assert L.bspgemm_ktruss_ex(None, None, 4, 0, 2, C.byref(T), None, None) == 1 and not T.value
    assert b"unknown method" in L.bspgemm_last_error()
    assert L.bspgemm_triangle_count_ex(None, None, -1, None) == 1 and b"unknown method" in L.bspgemm_last_error()
    # the knob without a context
    assert L.bspgemm_set_option(None, 7, 16) == 1 and L.bspgemm_get_option(None, 7) == -2 ** 31


def test_model_counts_triangles_through_the_lower_triangle():
    """a triangle i > j > k is the entry (i, j) of L with k in L_i n L_j: sum(dot_ref(L, L, L)) = triangles_ref"""
    rp, ci, n = gen.rmat(8, 8, (0.57, 0.19, 0.19, 0.05), 4401)
    s_rp, s_ci = ktruss_ref.symmetrise(rp, ci, n)
    lower = ktruss_ref.dedup_ref(*ktruss_ref.select_ref(s_rp, s_ci, "tril"), n)
    c_rp, c_ci, c_v = dot_ref.dot_ref(lower, lower, lower, n, n, n, n)
    expect = ktruss_ref.triangles_ref(s_rp, s_ci, n)
    assert expect > 100 and int(c_v.sum()) == expect
    assert c_rp[-1] == c_ci.size == c_v.size and (c_v > 0).all()
    # and the model on a graph small enough to count by hand: the 4-clique has 4 triangles; each lower entry (i, j) counts
    # the k < j adjacent to both
    k4 = dot_ref.csr([[], [0], [0, 1], [0, 1, 2]])
    c_rp, c_ci, c_v = dot_ref.dot_ref(k4, k4, k4, 4, 4, 4, 4)
    assert c_rp.tolist() == [0, 0, 0, 1, 3] and c_ci.tolist() == [1, 1, 2] and c_v.tolist() == [1, 1, 2]
    # repeats in any operand count once; a mask column at or above B.rows has no effect
    a = dot_ref.csr([[3, 1, 1, 3], [2]])
    b = dot_ref.csr([[1, 3, 3], [2, 2], []])
    f = dot_ref.csr([[0, 0, 1, 2, 5], [1, 7]])
    c_rp, c_ci, c_v = dot_ref.dot_ref(a, b, f, 2, 3, 4, 8)
    assert c_rp.tolist() == [0, 1, 2] and c_ci.tolist() == [0, 1] and c_v.tolist() == [2, 1]
    assert dot_ref.heavy_at_zero(a, b, f, 2, 3, 4, 8) == (3, 6)
