"""CPU-only checks of the operand transpose and download (bspgemm_matrix_transpose, bspgemm_matrix_download): the header
declares both, the library exports them, the Python binding lists them, a C caller compiles, and without a context both
calls refuse (BSPGEMM_ERR_INVALID, nothing handed back)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import bspgemm
from abi_kit import ROOT, ERR_INVALID, header_text


def _decl(name):
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"bspgemm_status\s+%s\s*\(([^;]*)\)\s*;" % name, code)
    assert m, "%s is not declared" % name
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_both_functions():
    t = _decl("bspgemm_matrix_transpose")
    assert len(t) == 3 and t[2].startswith("bspgemm_matrix **"), t
    d = _decl("bspgemm_matrix_download")
    assert len(d) == 4 and d[2].startswith("int *") and d[3].startswith("int *"), d
    text = header_text()
    assert "final/utils.c:77" in text and "final/coo2csc.c" in text


def test_library_exports_them_and_the_binding_lists_them():
    L = bspgemm.lib()
    for name in ("bspgemm_matrix_transpose", "bspgemm_matrix_download"):
        assert hasattr(L, name)
        assert name in bspgemm.EXPORTS
    assert callable(bspgemm.Context.transpose) and callable(bspgemm.Matrix.download)


def test_c_caller_compiles():
    src = r'''#include <stdlib.h>
#include "bspgemm.h"
/* pull-direction step: the in-neighbours of A's vertices are the rows of A^T */
int in_edges(bspgemm_context *ctx, const bspgemm_matrix *A, int **row_ptr, int **col_idx)
{
    bspgemm_matrix *AT = NULL;
    if (bspgemm_matrix_transpose(ctx, A, &AT) != BSPGEMM_OK) return 0;
    *row_ptr = (int *)malloc(((size_t)bspgemm_matrix_rows(AT) + 1) * sizeof(int));
    *col_idx = (int *)malloc(((size_t)bspgemm_matrix_nnz(AT) + 1) * sizeof(int));
    bspgemm_status st = bspgemm_matrix_download(ctx, AT, *row_ptr, *col_idx);
    bspgemm_matrix_free(AT);
    return st == BSPGEMM_OK;
}
'''
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.c")
        open(path, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", path,
                        "-o", os.path.join(d, "t.o")], check=True)


def test_null_context_refuses():
    L = bspgemm.lib()
    out = C.c_void_p(1)
    assert L.bspgemm_matrix_transpose(None, None, C.byref(out)) == ERR_INVALID
    assert not out.value
    assert "matrix_transpose" in L.bspgemm_last_error().decode()
    rp = np.full(4, -7, np.int32)
    ci = np.full(4, -7, np.int32)
    assert L.bspgemm_matrix_download(None, None, C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data)) == ERR_INVALID
    assert (rp == -7).all() and (ci == -7).all()          # nothing written
    assert "matrix_download" in L.bspgemm_last_error().decode()
