"""CPU-only checks of the OR-accumulating product's C ABI (bspgemm_multiply_accumulate) and of the transitive closure
(bspgemm_closure_ex, BSPGEMM_CLOSURE_TRANSITIVE): the header declares them, the library exports them, the Python binding
lists them, a C caller compiles, and without a GPU the Python path fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bspgemm
from abi_kit import ROOT, header_text


def _decl(code, name):
    m = re.search(r"bspgemm_status\s+%s\s*\(([^;]*)\)\s*;" % name, code)
    assert m, "%s is not declared" % name
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_accumulate_and_transitive_closure():
    text = header_text()
    assert re.search(r"#define\s+BSPGEMM_CLOSURE_TRANSITIVE\s+1u\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    params = _decl(code, "bspgemm_multiply_accumulate")
    assert len(params) == 7 and "bspgemm_matrix" in params[3] and params[6].startswith("bspgemm_result"), params
    params = _decl(code, "bspgemm_closure_ex")
    assert len(params) == 6 and params[2].startswith("unsigned"), params
    assert "old/BSpGEMM.c:75-126" in text and "SpGEMM_dor" in text


def test_library_exports_them_and_the_binding_lists_them():
    L = bspgemm.lib()
    for name in ("bspgemm_multiply_accumulate", "bspgemm_closure_ex"):
        assert hasattr(L, name)
        assert name in bspgemm.EXPORTS
    assert bspgemm.CLOSURE_TRANSITIVE == 1
    assert callable(bspgemm.Context.multiply_accumulate)


def test_c_caller_compiles():
    src = r'''#include "bspgemm.h"
int visit(bspgemm_context *ctx, const bspgemm_matrix *frontier, const bspgemm_matrix *A,
          const bspgemm_matrix *visited, bspgemm_result **next)
{
    return bspgemm_multiply_accumulate(ctx, frontier, A, visited, 0, bspgemm_matrix_rows(frontier), next) == BSPGEMM_OK;
}
int reach(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_result **T)
{
    int it = 0;
    return bspgemm_closure_ex(ctx, A, BSPGEMM_CLOSURE_TRANSITIVE, 64, T, &it) == BSPGEMM_OK ? it : -1;
}
'''
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.c")
        open(path, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", path,
                        "-o", os.path.join(d, "t.o")], check=True)


def test_accumulate_refuses_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(bspgemm.BspgemmError) as e:
        bspgemm.Context(0)
    assert e.value.status == 4          # BSPGEMM_ERR_NO_DEVICE: no context, so no product of any kind
    L = bspgemm.lib()
    out = C.c_void_p(1)
    assert L.bspgemm_multiply_accumulate(None, None, None, None, 0, 0, C.byref(out)) == 1
    assert not out.value
    for flags in (1, 0, 2):            # no context: invalid whatever the flags, and nothing is handed back
        T, it = C.c_void_p(1), C.c_int(7)
        assert L.bspgemm_closure_ex(None, None, flags, 8, C.byref(T), C.byref(it)) == 1
        assert not T.value
