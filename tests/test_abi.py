"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/bspgemm.h declares, and the product path FAILS LOUDLY without a GPU (no CPU fallback)."""
import os
import re

import pytest

import bspgemm
from abi_kit import ROOT


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "bspgemm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b(bspgemm_[a-zA-Z0-9_]+|SpGEMM_hip[a-zA-Z0-9_]*)\s*\(", text)
    return sorted(set(names))


def test_library_loads_and_exports_every_declared_symbol():
    L = bspgemm.lib()
    declared = _declared_functions()
    assert len(declared) >= 35
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, "declared in include/bspgemm.h but not exported: %s" % missing
    assert sorted(bspgemm.EXPORTS) == declared, "python binding list out of sync with the header"


def _declared_parameter_counts():
    """{function: number of parameters} from the prototypes of include/bspgemm.h (no prototype there has a function-pointer
    parameter: the callbacks of bspgemm_host_transport are struct fields, which the `;` inside the braces keeps apart)"""
    text = open(os.path.join(ROOT, "include", "bspgemm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {}
    for name, params in re.findall(r"\b(bspgemm_[a-zA-Z0-9_]+|SpGEMM_hip[a-zA-Z0-9_]*)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        counts[name] = 0 if params in ("", "void") else params.count(",") + 1
    return counts


def test_every_export_is_bound_with_the_header_parameter_count():
    """one table binds the ABI: every exported name has argtypes on bspgemm.lib(), as many as the header's prototype has
    parameters -- a name without them would pass a 64-bit handle as a C int"""
    L = bspgemm.lib()
    counts = _declared_parameter_counts()
    assert sorted(counts) == _declared_functions()
    for name in bspgemm.EXPORTS:
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None, "%s has no argtypes" % name
        assert len(argtypes) == counts[name], "%s: %d argtypes, %d parameters in the header" % (name, len(argtypes), counts[name])
    assert L.bspgemm_comm_inject_failure.restype is None
    import ctypes
    for name in ("bspgemm_last_error", "bspgemm_build_info", "bspgemm_status_string"):
        assert getattr(L, name).restype is ctypes.c_char_p


def test_info_as_dict_scalars_and_trailing_or_inner_arrays():
    """as_dict of the info structs: scalars as int, an array field as a list of int -- LpInfo's array comes last, PrInfo's
    in the middle"""
    import ctypes
    lp = bspgemm.LpInfo(3, 1, 7, 0, (ctypes.c_int64 * 4)(5, 6, 2 ** 40, 8))
    assert lp.as_dict() == {"iterations": 3, "converged": 1, "communities": 7, "changed": 0, "class_vertices": [5, 6, 2 ** 40, 8]}
    pr = bspgemm.PrInfo(2 ** 62, 9, 4, (ctypes.c_int64 * 4)(1, 2, 3, 4), 20, 0, 2, 1, 1)
    d = pr.as_dict()
    assert d == {"mass": 2 ** 62, "delta": 9, "dangling": 4, "class_vertices": [1, 2, 3, 4], "iterations": 20, "converged": 0,
                 "method": 2, "transposed": 1, "canonicalised": 1}
    assert all(type(v) is int for k, v in d.items() if k != "class_vertices") and all(type(v) is int for v in d["class_vertices"])
    assert bspgemm.MatchInfo(pairs=2, lanes=16).as_dict() == {"pairs": 2, "entries_walked": 0, "hub_chunks": 0, "rounds": 0, "lanes": 16}


def test_alloc_test_hooks_are_declared_and_idle_before_any_context():
    """the two test hooks of the device-memory gate: declared with these argument lists, exported, bound, and in a process
    that has created no context the gate has seen nothing (requests, live allocations, live bytes, injected failures)"""
    import subprocess
    import sys
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "bspgemm.h")).read())
    assert "void bspgemm_debug_fail_alloc(int nth);" in text
    assert "void bspgemm_debug_alloc_state(int64_t out[4]);" in text
    L = bspgemm.lib()
    for name in ("bspgemm_debug_fail_alloc", "bspgemm_debug_alloc_state"):
        assert name in bspgemm.EXPORTS and hasattr(L, name)
    assert L.bspgemm_debug_fail_alloc.restype is None and L.bspgemm_debug_alloc_state.restype is None
    state = bspgemm.debug_alloc_state()
    assert len(state) == 4 and all(v >= 0 for v in state) and state[3] <= state[0]
    code = ("import ctypes\n"
            "L = ctypes.CDLL(%r)\n"
            "out = (ctypes.c_int64 * 4)(7, 7, 7, 7)\n"
            "L.bspgemm_debug_alloc_state(out)\n"
            "assert list(out) == [0, 0, 0, 0], list(out)\n"
            "L.bspgemm_debug_fail_alloc(3)\n"                   # arming allocates nothing and fires nothing
            "L.bspgemm_debug_fail_alloc(0)\n"
            "L.bspgemm_debug_alloc_state(out)\n"
            "assert list(out) == [0, 0, 0, 0], list(out)\n"
            "print('idle')\n") % bspgemm.LIB_PATH
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "idle" in r.stdout, r.stdout + r.stderr


def test_poison_and_guard_hooks_are_declared_and_off_before_any_context():
    """the fill, guard and scribble hooks: declared with these argument lists, exported, bound with the header's types, and
    in a process that has created no context turning them on and off allocates nothing, finds no guard damaged and leaves
    no error text; scribble refuses a NULL context without touching a device"""
    import ctypes
    import subprocess
    import sys
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "bspgemm.h")).read())
    for proto in ("void bspgemm_debug_fill_alloc(int on, uint32_t word);", "void bspgemm_debug_guard_alloc(int on);",
                  "int64_t bspgemm_debug_check_guards(void);",
                  "bspgemm_status bspgemm_debug_scribble(bspgemm_context *ctx, uint32_t word);"):
        assert proto in text, proto
    assert "whole" in text.lower() and "d_err" in text          # what the guards do not see, and what scribble leaves out
    L = bspgemm.lib()
    assert L.bspgemm_debug_fill_alloc.restype is None and L.bspgemm_debug_fill_alloc.argtypes == [ctypes.c_int, ctypes.c_uint32]
    assert L.bspgemm_debug_guard_alloc.restype is None and L.bspgemm_debug_guard_alloc.argtypes == [ctypes.c_int]
    assert L.bspgemm_debug_check_guards.restype is ctypes.c_int64 and L.bspgemm_debug_check_guards.argtypes == []
    assert L.bspgemm_debug_scribble.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    code = ("import ctypes\n"
            "L = ctypes.CDLL(%r)\n"
            "L.bspgemm_debug_check_guards.restype = ctypes.c_int64\n"
            "L.bspgemm_last_error.restype = ctypes.c_char_p\n"
            "L.bspgemm_debug_scribble.argtypes = [ctypes.c_void_p, ctypes.c_uint32]\n"
            "out = (ctypes.c_int64 * 4)(7, 7, 7, 7)\n"
            "assert L.bspgemm_debug_check_guards() == 0\n"
            "L.bspgemm_debug_fill_alloc(1, 0xFFFFFFFF)\n"
            "L.bspgemm_debug_guard_alloc(1)\n"
            "assert L.bspgemm_debug_check_guards() == 0 and L.bspgemm_last_error() == b''\n"
            "L.bspgemm_debug_fill_alloc(0, 0)\n"
            "L.bspgemm_debug_guard_alloc(0)\n"
            "L.bspgemm_debug_alloc_state(out)\n"
            "assert list(out) == [0, 0, 0, 0], list(out)\n"
            "assert L.bspgemm_debug_scribble(None, 1) == 1 and b'ctx is NULL' in L.bspgemm_last_error()\n"   # BSPGEMM_ERR_INVALID
            "print('off')\n") % bspgemm.LIB_PATH
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "off" in r.stdout, r.stdout + r.stderr


def test_header_cites_the_reference_interfaces():
    text = open(os.path.join(ROOT, "include", "bspgemm.h")).read()
    for cite in ("final/SpGEMM_mpi_omp.c:71-74", "final/SpGEMM_mpi_omp.c:15-18", "final/utils.c:47-81",
                 "final/SpGEMM_mpi_omp_validity.c:290-302", "final/SpGEMM_mpi_omp.c:155-225",
                 "Matlab/inc/BSpGEMM.h:2-4", "final/SpGEMM_mpi_omp.c:232-235"):
        assert cite in text, cite


def test_header_compiles_as_c():
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "bspgemm.h"\nint main(void){bspgemm_stats s; (void)s; return BSPGEMM_OK;}\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                        "-o", os.path.join(d, "t.o")], check=True)


def test_product_refuses_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(bspgemm.BspgemmError) as e:
        bspgemm.Context(0)
    assert e.value.status == 4          # BSPGEMM_ERR_NO_DEVICE
    import numpy as np
    rp = np.array([0, 1, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    with pytest.raises(bspgemm.BspgemmError):
        bspgemm.SpGEMM_hip(ci, rp, 2, ci, rp, 2)


def test_product_never_touches_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may use oracle/."""
    pkg = os.path.join(ROOT, "binary-spgemm_amd")
    for base, _dirs, files in os.walk(pkg):
        if "build" in base:
            continue
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hpp", ".hip", "Makefile")):
                text = open(os.path.join(base, f), errors="replace").read()
                assert "oracle" not in text.lower(), "%s mentions the oracle" % os.path.join(base, f)
    assert "oracle" not in open(os.path.join(ROOT, "include", "bspgemm.h")).read().lower()


def test_one_hip_runtime_per_process():
    """bspgemm first, torch second, in a fresh process: exactly one libamdhip64 may be mapped
    (round 1's segfault in the RCCL stitch test was two of them: torch's bundled runtime and
    /opt/rocm's behind libbspgemm.so's rpath -- INTEGRATION.md section 2); and the guard refuses a
    process that already holds two."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import bspgemm; bspgemm.lib()\n"
            "import torch\n"
            "libs = bspgemm.check_single_hip_runtime()\n"
            "assert len(libs) == 1, libs\n"
            "print('one runtime:', libs[0])\n") % os.path.join(ROOT, "binary-spgemm_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "one runtime:" in r.stdout
    bad = ("import ctypes, sys; sys.path.insert(0, %r)\n"
           "ctypes.CDLL(%r)\n"                      # the library before torch: /opt/rocm's runtime comes with it
           "import torch\n"
           "import bspgemm\n"
           "try:\n"
           "    bspgemm.check_single_hip_runtime()\n"
           "except RuntimeError as e:\n"
           "    print('refused:', e)\n") % (os.path.join(ROOT, "binary-spgemm_amd"),
                                            os.path.join(ROOT, "binary-spgemm_amd", "libbspgemm.so"))
    r = subprocess.run([sys.executable, "-c", bad], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused: two HIP runtimes" in r.stdout, r.stdout + r.stderr


def test_shipped_library_has_no_ablation_paths():
    """the shipped .so was one -DBSP_ABLATE away from a silent wrong answer.  The timing-only
    ablation branches are gone from the kernel sources, the tuning constants are not overridable, and the
    library says so (bspgemm_build_info)."""
    import glob
    info = bspgemm.lib().bspgemm_build_info().decode()
    assert "BSP_ABLATE=0" in info and "gfx950" in info, info
    src = glob.glob(os.path.join(ROOT, "binary-spgemm_amd", "csrc", "*"))
    assert len(src) > 10
    for path in src:
        text = open(path).read()
        for word in ("BSP_ABLATE", "BSP_DENSE_ABLATE", "BSP_DENSE_NOEMIT", "BSP_COMPACT_NOSLOW"):
            if os.path.basename(path) == "context.hip" and word == "BSP_ABLATE":
                continue                                   # the text of bspgemm_build_info
            assert word not in text, "%s still mentions %s" % (path, word)
        assert "#ifndef BSP_" not in text, "%s has a -D overridable kernel switch" % path
    mk = open(os.path.join(ROOT, "binary-spgemm_amd", "Makefile")).read()
    assert "ABLATE" not in mk and "XDEF" not in mk
