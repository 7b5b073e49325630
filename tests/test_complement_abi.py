"""CPU-only checks of the complemented-mask product's C ABI (bspgemm_multiply_masked_ex, BSPGEMM_MASK_COMPLEMENT): the
header declares it, the library exports it, the Python binding lists it, a C caller compiles, and without a GPU the
Python path fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import bspgemm
from abi_kit import ROOT, header_text


def test_header_declares_the_complemented_product():
    text = header_text()
    assert re.search(r"#define\s+BSPGEMM_MASK_COMPLEMENT\s+1u\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"bspgemm_status\s+bspgemm_multiply_masked_ex\s*\(([^;]*)\)\s*;", code)
    assert m, "bspgemm_multiply_masked_ex is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8 and params[4].startswith("unsigned"), params
    assert "final/SpGEMM_mpi_omp.c:232-288" in text


def test_library_exports_it_and_the_binding_lists_it():
    L = bspgemm.lib()
    assert hasattr(L, "bspgemm_multiply_masked_ex")
    assert "bspgemm_multiply_masked_ex" in bspgemm.EXPORTS
    assert bspgemm.MASK_COMPLEMENT == 1


def test_c_caller_compiles():
    src = r'''#include "bspgemm.h"
int next_frontier(bspgemm_context *ctx, const bspgemm_matrix *frontier, const bspgemm_matrix *A,
                  const bspgemm_matrix *visited, bspgemm_result **next)
{
    return bspgemm_multiply_masked_ex(ctx, frontier, A, visited, BSPGEMM_MASK_COMPLEMENT, 0,
                                      bspgemm_matrix_rows(frontier), next) == BSPGEMM_OK;
}
'''
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.c")
        open(path, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", path,
                        "-o", os.path.join(d, "t.o")], check=True)


def test_complement_refuses_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(bspgemm.BspgemmError) as e:
        bspgemm.Context(0)
    assert e.value.status == 4          # BSPGEMM_ERR_NO_DEVICE: no context, so no product of any kind
    L = bspgemm.lib()
    out = C.c_void_p(1)
    for flags in (1, 0, 2):            # no context: invalid whatever the flags, and nothing is handed back
        assert L.bspgemm_multiply_masked_ex(None, None, None, None, flags, 0, 0, C.byref(out)) == 1
        assert not out.value
        out = C.c_void_p(1)
