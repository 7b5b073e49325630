"""CPU-only checks of the counting masked product's C ABI (bspgemm_multiply_masked_count, bspgemm_result_values_device,
bspgemm_result_download_values): the header declares them with the documented signatures, the library exports them, the
Python binding lists them, a C caller compiles, and without a GPU the Python path fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bspgemm
from abi_kit import ROOT, header_text

NAMES = ("bspgemm_multiply_masked_count", "bspgemm_result_values_device", "bspgemm_result_download_values")


def _code():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def _params(code, ret, name):
    m = re.search(r"%s\s*\*?\s*%s\s*\(([^;]*)\)\s*;" % (ret, name), code)
    assert m, "%s is not declared" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_three_functions():
    code = _code()
    p = _params(code, "bspgemm_status", "bspgemm_multiply_masked_count")
    assert p == ["bspgemm_context *ctx", "const bspgemm_matrix *A", "const bspgemm_matrix *B", "const bspgemm_matrix *F",
                 "int row_begin", "int row_end", "bspgemm_result **C"], p
    p = _params(code, r"const\s+int", "bspgemm_result_values_device")
    assert p == ["const bspgemm_result *C"], p
    p = _params(code, "bspgemm_status", "bspgemm_result_download_values")
    assert p == ["bspgemm_context *ctx", "const bspgemm_result *C", "int *values"], p
    text = header_text()
    assert "PLUS_PAIR" in text and "final/SpGEMM_mpi_omp.c:232-288" in text
    assert "BSPGEMM_ERR_OVERFLOW" in text.split("bspgemm_multiply_masked_count(")[0].split("bspgemm_multiply_accumulate(")[-1]


def test_library_exports_them_and_the_binding_lists_them():
    L = bspgemm.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in bspgemm.EXPORTS, name
    assert callable(bspgemm.Context.multiply_masked_count)
    assert callable(bspgemm.Result.download_values)
    assert isinstance(bspgemm.Result.values_device, property)


def test_c_caller_compiles():
    src = r'''#include <stdlib.h>
#include "bspgemm.h"
long long triangles(bspgemm_context *ctx, const bspgemm_matrix *L)
{
    bspgemm_result *C = NULL;
    long long sum = 0;
    if (bspgemm_multiply_masked_count(ctx, L, L, L, 0, bspgemm_matrix_rows(L), &C) != BSPGEMM_OK) return -1;
    if (bspgemm_result_values_device(C) != NULL) {
        int *v = (int *)malloc(((size_t)bspgemm_result_nnz(C) + 1) * sizeof(int));
        if (v && bspgemm_result_download_values(ctx, C, v) == BSPGEMM_OK)
            for (int64_t k = 0; k < bspgemm_result_nnz(C); k++) sum += v[k];
        free(v);
    }
    bspgemm_result_free(C);
    return sum;
}
'''
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.c")
        open(path, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", path,
                        "-o", os.path.join(d, "t.o")], check=True)


def test_masked_count_refuses_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(bspgemm.BspgemmError) as e:
        bspgemm.Context(0)
    assert e.value.status == 4          # BSPGEMM_ERR_NO_DEVICE: no context, so no product of any kind


def test_null_context_is_invalid_and_hands_back_nothing():
    L = bspgemm.lib()
    for F in (None, C.c_void_p(8)):    # (the context is checked before any operand is looked at)
        out = C.c_void_p(1)
        assert L.bspgemm_multiply_masked_count(None, None, None, F, 0, 0, C.byref(out)) == 1
        assert not out.value
    assert L.bspgemm_result_values_device(None) is None
    assert L.bspgemm_result_download_values(None, None, None) == 1
