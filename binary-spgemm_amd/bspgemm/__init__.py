"""Python view of libbspgemm.so (ctypes over the C ABI in include/bspgemm.h).

This module is plumbing for tests and bench.py: every compute call goes through the C ABI into
the HIP kernels.  There is no Python or CPU implementation of the product here -- if the shared
library is missing or no gfx950 device is visible the calls raise.

Mirrors the reference's interface names where they exist:
    SpGEMM_hip(...)        <-> SpGEMM_omp      final/SpGEMM_mpi_omp.c:71-74
    SpGEMM_hip_bigslice    <-> SpGEMM_bigslice final/SpGEMM_mpi_omp.c:15-18
    SpGEMM_hip_mat         <-> SpGEMM_mat      Matlab/inc/BSpGEMM.h:2-4
    readCOO                <-> readCOO         final/utils.c:47-81
    csr_equal              <-> SpGEMM_valid    final/SpGEMM_mpi_omp_validity.c:290-302
"""
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

# host-side OpenMP (generators): stay inside one GPU's CPU share on shared boxes
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, len(os.sched_getaffinity(0)))))
# The library runs its class launches on two HIP streams next to its main one; the ROCm runtime
# multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  Once RCCL
# and torch have created theirs, two of the library's streams end up on ONE queue and the class
# launches serialise (+9 % accumulate time, measured).  Read by the HIP runtime when it starts.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)                      # binary-spgemm_amd/
LIB_PATH = os.path.join(_ROOT, "libbspgemm.so")

_I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")

STATUS = {0: "OK", 1: "ERR_INVALID", 2: "ERR_ALLOC", 3: "ERR_HIP", 4: "ERR_NO_DEVICE",
          5: "ERR_OVERFLOW", 6: "ERR_IO", 7: "ERR_FORMAT", 8: "ERR_COMM", 9: "ERR_SIZE"}

class BspgemmError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = lib().bspgemm_last_error().decode(errors="replace") if _lib is not None else ""
        super().__init__("%s: %s %s" % (where, STATUS.get(status, status), msg))


MAX_BINS = 20      # BSPGEMM_MAX_BINS
FLOWS = {"auto": 0, "upper-bound": 1, "exact": 2}                                    # BSPGEMM_FLOW_*
MASK_COMPLEMENT = 1                                                                      # BSPGEMM_MASK_COMPLEMENT
CLOSURE_TRANSITIVE = 1                                                                   # BSPGEMM_CLOSURE_TRANSITIVE
SELECT_OPS = {"tril": 1, "triu": 2, "offdiag": 3}                                       # bspgemm_select
SETOPS = {"or": 1, "and": 2, "andnot": 3, "xor": 4}                                     # bspgemm_setop
SYMMETRIZE_DROP_DIAGONAL = 1                                                             # BSPGEMM_SYMMETRIZE_DROP_DIAGONAL
COMPARES = {">=": 1, ">": 2, "<=": 3, "<": 4, "==": 5, "!=": 6}                          # bspgemm_compare
OPTIONS = {"class_streams": 1, "blocked_extents": 2, "check": 3, "small_path": 4, "padded_rows": 5,
           "shared_slots": 6, "dot_light": 7, "bfs_alpha": 8, "bfs_beta": 9, "bfs_push_lanes": 10,
           "lp_min_class": 11, "pr_min_class": 12, "bc_lanes": 13, "extract_lanes": 14, "match_lanes": 15}                                                                         # bspgemm_option
SUPPORT_METHODS = {"product": 0, "dot": 1}                                              # bspgemm_support_method
BFS_DIRECTIONS = {"auto": 0, "push": 1, "pull": 2}                                      # bspgemm_bfs_direction
EXTRACT_KEEP_SHAPE = 1                                                                   # BSPGEMM_EXTRACT_KEEP_SHAPE
WEIGHTS_SYMMETRIC = 1                                                                    # BSPGEMM_WEIGHTS_SYMMETRIC
SSSP_DELTA_C = 32                                                                        # BSPGEMM_SSSP_DELTA_C
LCC_DIRECTED = 1                                                                         # BSPGEMM_LCC_DIRECTED
PR_AUTO, PR_PULL, PR_PUSH = 0, 1, 2                                                      # bspgemm_pr_method


class _Info(C.Structure):
    """what the bspgemm_*_info structs share: as_dict() with every scalar field as an int, every array field as a list of ints"""

    def as_dict(self):
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = [int(x) for x in v] if isinstance(v, C.Array) else int(v)
        return d


class DotInfo(_Info):
    """bspgemm_dot_info"""
    _fields_ = [("entries", C.c_int64), ("heavy_entries", C.c_int64), ("kept", C.c_int64), ("canonicalised", C.c_int)]


class BfsTreeInfo(_Info):
    """bspgemm_bfs_tree_info"""
    _fields_ = [("reached", C.c_int64), ("edges_pushed", C.c_int64), ("pull_mask", C.c_uint64), ("depth", C.c_int),
                ("complete", C.c_int), ("push_levels", C.c_int), ("pull_levels", C.c_int), ("transposed", C.c_int),
                ("canonicalised", C.c_int)]


class LpInfo(_Info):
    """bspgemm_lp_info"""
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("communities", C.c_int), ("changed", C.c_int),
                ("class_vertices", C.c_int64 * 4)]


class LccInfo(_Info):
    """bspgemm_lcc_info"""
    _fields_ = [("triangles", C.c_int64), ("entries", C.c_int64), ("heavy_entries", C.c_int64), ("reciprocal", C.c_int64)]


class PrInfo(_Info):
    """bspgemm_pr_info"""
    _fields_ = [("mass", C.c_uint64), ("delta", C.c_uint64), ("dangling", C.c_int64), ("class_vertices", C.c_int64 * 4),
                ("iterations", C.c_int), ("converged", C.c_int), ("method", C.c_int), ("transposed", C.c_int),
                ("canonicalised", C.c_int)]


class BcInfo(_Info):
    """bspgemm_bc_info"""
    _fields_ = [("sigma_max", C.c_uint64), ("reached", C.c_int64), ("edges_forward", C.c_int64), ("hub_chunks", C.c_int64),
                ("sources", C.c_int), ("depth_max", C.c_int), ("levels", C.c_int), ("canonicalised", C.c_int)]


class MatchInfo(_Info):
    """bspgemm_match_info"""
    _fields_ = [("pairs", C.c_int64), ("entries_walked", C.c_int64), ("hub_chunks", C.c_int64), ("rounds", C.c_int),
                ("lanes", C.c_int)]


class SsspInfo(_Info):
    """bspgemm_sssp_info"""
    _fields_ = [("delta", C.c_uint64), ("dist_max", C.c_uint64), ("reached", C.c_int64), ("entries_walked", C.c_int64),
                ("improved", C.c_int64), ("hub_chunks", C.c_int64), ("rounds", C.c_int), ("buckets", C.c_int),
                ("lanes", C.c_int), ("reserved", C.c_int)]


class SsspParams(C.Structure):
    """bspgemm_sssp_params"""
    _fields_ = [("delta", C.c_uint64), ("lanes", C.c_int), ("reserved", C.c_int)]


class ExtractInfo(_Info):
    """bspgemm_extract_info"""
    _fields_ = [("kept", C.c_int64), ("scanned", C.c_int64), ("hub_chunks", C.c_int64), ("lanes", C.c_int),
                ("cols_monotone", C.c_int), ("sorted_by", C.c_int), ("canonicalised", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("nnz_a", C.c_int64), ("products", C.c_int64), ("nnz_c", C.c_int64),
                ("bytes_alg", C.c_int64), ("bytes_read_alg", C.c_int64), ("rows_per_bin", C.c_int64 * MAX_BINS),
                ("ms_total", C.c_float), ("ms_symbolic", C.c_float), ("ms_prepass", C.c_float),
                ("ms_count", C.c_float), ("ms_numeric", C.c_float), ("ms_stitch", C.c_float),
                ("ms_bin", C.c_float * MAX_BINS), ("ms_bin_count", C.c_float * MAX_BINS),
                ("t_bin", C.c_float * MAX_BINS), ("t_bin_count", C.c_float * MAX_BINS), ("bins", C.c_int),
                ("bin_cap", C.c_int * MAX_BINS), ("flow", C.c_int), ("prepass_kernel", C.c_int),
                ("class_streams", C.c_int), ("small_path", C.c_int), ("checked", C.c_int), ("padded_rows", C.c_int)]

    def as_dict(self):
        arrays = ("rows_per_bin", "ms_bin", "ms_bin_count", "t_bin", "t_bin_count", "bin_cap")
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in arrays}
        for k in arrays:
            d[k] = list(getattr(self, k))[: self.bins]
        return d


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
GATHERV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.c_int)


class HostTransport(C.Structure):
    """bspgemm_host_transport: all-gather / gatherv callbacks on host buffers"""
    _fields_ = [("user", C.c_void_p), ("allgather", ALLGATHER_FN), ("gatherv", GATHERV_FN)]


_VP, _PVP = C.c_void_p, C.POINTER(C.c_void_p)
_IPP = C.POINTER(C.POINTER(C.c_int))
_U32PP = C.POINTER(C.POINTER(C.c_uint32))
_INT = C.c_int                                       # bspgemm_status and the plain int returns (ctypes' default)
# The C ABI, once: every symbol include/bspgemm.h declares (checked by tests/test_abi.py) -> (restype, argtypes).
# lib() binds them; EXPORTS is this table's names.
_SIGNATURES = {
    "bspgemm_status_string": (C.c_char_p, [C.c_int]),
    "bspgemm_last_error": (C.c_char_p, []),
    "bspgemm_create": (_INT, [C.c_int, _PVP]),
    "bspgemm_destroy": (None, [_VP]),
    "bspgemm_set_stream": (_INT, [_VP, _VP]),
    "bspgemm_synchronize": (_INT, [_VP]),
    "bspgemm_set_flow": (_INT, [_VP, C.c_int]),
    "bspgemm_set_class_timing": (_INT, [_VP, C.c_int]),
    "bspgemm_build_info": (C.c_char_p, []),
    "bspgemm_matrix_invalidate": (_INT, [_VP]),
    "bspgemm_set_option": (_INT, [_VP, C.c_int, C.c_int]),
    "bspgemm_get_option": (_INT, [_VP, C.c_int]),
    "bspgemm_matrix_uses_blocked_table": (_INT, [_VP]),
    "bspgemm_matrix_uses_padded_rows": (_INT, [_VP]),
    "bspgemm_matrix_upload": (_INT, [_VP, C.c_int, C.c_int, _VP, _VP, _PVP]),
    "bspgemm_matrix_wrap_device": (_INT, [_VP, C.c_int, C.c_int, C.c_int64, _VP, _VP, _PVP]),
    "bspgemm_matrix_free": (None, [_VP]),
    "bspgemm_matrix_transpose": (_INT, [_VP, _VP, _PVP]),
    "bspgemm_matrix_download": (_INT, [_VP, _VP, _VP, _VP]),
    "bspgemm_matrix_rows": (_INT, [_VP]),
    "bspgemm_matrix_cols": (_INT, [_VP]),
    "bspgemm_matrix_nnz": (C.c_int64, [_VP]),
    "bspgemm_multiply": (_INT, [_VP, _VP, _VP, C.c_int, C.c_int, _PVP]),
    "bspgemm_multiply_masked": (_INT, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, _PVP]),
    "bspgemm_multiply_masked_ex": (_INT, [_VP, _VP, _VP, _VP, C.c_uint, C.c_int, C.c_int, _PVP]),
    "bspgemm_result_rows": (_INT, [_VP]),
    "bspgemm_result_nnz": (C.c_int64, [_VP]),
    "bspgemm_result_row_ptr_device": (_VP, [_VP]),
    "bspgemm_result_col_idx_device": (_VP, [_VP]),
    "bspgemm_result_download": (_INT, [_VP, _VP, _VP, _VP]),
    "bspgemm_multiply_masked_count": (_INT, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, _PVP]),
    "bspgemm_result_values_device": (_VP, [_VP]),
    "bspgemm_result_download_values": (_INT, [_VP, _VP, _VP]),
    "bspgemm_result_free": (None, [_VP]),
    "bspgemm_matrix_from_result": (_INT, [_VP, _VP, C.c_int, _PVP]),
    "bspgemm_matrix_select": (_INT, [_VP, _VP, C.c_int, _PVP]),
    "bspgemm_matrix_from_result_where": (_INT, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP]),
    "bspgemm_result_values_sum": (_INT, [_VP, _VP, C.POINTER(C.c_int64)]),
    "bspgemm_triangle_count": (_INT, [_VP, _VP, C.POINTER(C.c_int64)]),
    "bspgemm_ktruss": (_INT, [_VP, _VP, C.c_int, C.c_int, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_multiply_masked_dot": (_INT, [_VP, _VP, _VP, _VP, C.c_uint, _PVP, C.POINTER(DotInfo)]),
    "bspgemm_triangle_count_ex": (_INT, [_VP, _VP, C.c_int, C.POINTER(C.c_int64)]),
    "bspgemm_ktruss_ex": (_INT, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_bfs": (_INT, [_VP, _VP, C.c_int, _VP, C.c_int, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_bfs_tree": (_INT, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, _PVP, C.POINTER(BfsTreeInfo)]),
    "bspgemm_connected_components": (_INT, [_VP, _VP, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_core_numbers": (_INT, [_VP, _VP, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_kcore": (_INT, [_VP, _VP, C.c_int, _PVP, C.POINTER(C.c_int)]),
    "bspgemm_strongly_connected_components": (_INT, [_VP, _VP, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_graph_coloring": (_INT, [_VP, _VP, C.c_int, C.c_uint, _PVP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bspgemm_label_propagation": (_INT, [_VP, _VP, _VP, C.c_int, _PVP, C.POINTER(LpInfo)]),
    "bspgemm_local_clustering": (_INT, [_VP, _VP, C.c_uint, _PVP, _VP, _VP, C.POINTER(LccInfo)]),
    "bspgemm_pagerank": (_INT, [_VP, _VP, _VP, C.c_int, C.c_double, C.c_int, C.c_double, _VP, _VP, C.POINTER(PrInfo)]),
    "bspgemm_betweenness": (_INT, [_VP, _VP, C.c_int, _VP, _VP, _VP, C.POINTER(BcInfo)]),
    "bspgemm_maximal_matching": (_INT, [_VP, _VP, C.c_int, C.c_uint, _PVP, _VP, C.POINTER(MatchInfo)]),
    "bspgemm_weights_upload": (_INT, [_VP, _VP, _VP, _PVP]),
    "bspgemm_weights_hashed": (_INT, [_VP, _VP, C.c_uint, C.c_uint32, C.c_uint32, C.c_uint, _PVP]),
    "bspgemm_weights_download": (_INT, [_VP, _VP, _VP]),
    "bspgemm_weights_nnz": (C.c_int64, [_VP]),
    "bspgemm_weights_sum": (C.c_uint64, [_VP]),
    "bspgemm_weights_free": (None, [_VP]),
    "bspgemm_sssp": (_INT, [_VP, _VP, _VP, C.c_int, C.POINTER(SsspParams), _VP, _VP, C.POINTER(SsspInfo)]),
    "bspgemm_matrix_extract": (_INT, [_VP, _VP, C.c_int, _VP, C.c_int, _VP, C.c_uint, _PVP, C.POINTER(ExtractInfo)]),
    "bspgemm_matrix_extract_rows_of": (_INT, [_VP, _VP, _VP, C.c_int, _VP, C.c_int, C.c_uint, _PVP, C.POINTER(ExtractInfo)]),
    "bspgemm_matrix_setop": (_INT, [_VP, _VP, _VP, C.c_int, _PVP]),
    "bspgemm_matrix_equal": (_INT, [_VP, _VP, _VP, C.POINTER(C.c_int)]),
    "bspgemm_matrix_symmetrize": (_INT, [_VP, _VP, C.c_uint, _PVP]),
    "bspgemm_closure": (_INT, [_VP, _VP, C.c_int, _PVP, C.POINTER(C.c_int)]),
    "bspgemm_multiply_accumulate": (_INT, [_VP, _VP, _VP, _VP, C.c_int, C.c_int, _PVP]),
    "bspgemm_closure_ex": (_INT, [_VP, _VP, C.c_uint, C.c_int, _PVP, C.POINTER(C.c_int)]),
    "bspgemm_row_work_prefix": (_INT, [_VP, _VP, _VP, _I64P]),
    "bspgemm_partition_rows": (_INT, [_VP, _VP, _VP, C.c_int, _I32P]),
    "bspgemm_last_stats": (_INT, [_VP, C.POINTER(Stats)]),
    "bspgemm_stats_at": (_INT, [_VP, C.c_int, C.POINTER(Stats)]),
    "SpGEMM_hip": (_INT, [_I32P, _VP, C.c_int, _I32P, _I32P, C.c_int, _IPP, _I32P, C.c_int]),
    "SpGEMM_hip_bigslice": (_INT, [_I32P, _I32P, C.c_int, _I32P, _I32P, C.c_int, _IPP, _I32P, C.POINTER(C.c_int), C.c_int, C.c_int]),
    "SpGEMM_hip_mat": (_INT, [_I32P, _I32P, C.c_int, _I32P, _I32P, C.c_int, _I32P, _I32P]),
    "SpGEMM_hip_masked": (_INT, [_I32P, _I32P, C.c_int, _I32P, _I32P, C.c_int, _I32P, _I32P, _IPP, _I32P, C.POINTER(C.c_int)]),
    "bspgemm_dropin_set_device": (_INT, [C.c_int]),
    "bspgemm_debug_fail_alloc": (None, [C.c_int]),
    "bspgemm_debug_alloc_state": (None, [_I64P]),
    "bspgemm_debug_fill_alloc": (None, [C.c_int, C.c_uint32]),
    "bspgemm_debug_guard_alloc": (None, [C.c_int]),
    "bspgemm_debug_check_guards": (C.c_int64, []),
    "bspgemm_debug_scribble": (_INT, [_VP, C.c_uint32]),
    "bspgemm_comm_unique_id": (_INT, [C.c_char_p]),
    "bspgemm_comm_create": (_INT, [_VP, C.c_char_p, C.c_int, C.c_int, _PVP]),
    "bspgemm_comm_destroy": (None, [_VP]),
    "bspgemm_comm_stitch_row_ptr": (_INT, [_VP, _VP, _I32P, _PVP, _VP]),
    "bspgemm_lengths_to_row_ptr": (_INT, [_VP, _VP, C.c_int, C.c_int, _I32P, _VP, _VP]),
    "bspgemm_readCOO": (_INT, [C.c_char_p, _U32PP, _U32PP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "bspgemm_readCOO_ex": (_INT, [C.c_char_p, C.c_uint, _U32PP, _U32PP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "bspgemm_comm_create_host": (_INT, [_VP, C.POINTER(HostTransport), C.c_int, C.c_int, _PVP]),
    "bspgemm_comm_rank": (_INT, [_VP]),
    "bspgemm_comm_size": (_INT, [_VP]),
    "bspgemm_comm_gather_col_idx": (_INT, [_VP, _VP, _I64P, C.c_int, _VP]),
    "SpGEMM_hip_multi": (_INT, [_VP, _I32P, _I32P, C.c_int, _I32P, _I32P, C.c_int, _IPP, _I32P, C.c_int]),
    "bspgemm_write_mtx": (_INT, [C.c_char_p, C.c_int, C.c_int, _I32P, _I32P]),
    "bspgemm_write_result_mtx": (_INT, [C.c_char_p, C.c_int, C.c_int, _I64P, _I32P]),
    "bspgemm_csr_equal": (_INT, [_I32P, _I32P, _I32P, _I32P, C.c_int]),
    "bspgemm_csr_equal64": (_INT, [_I32P, _I64P, _I32P, _I64P, C.c_int]),
    "bspgemm_gen_uniform": (_INT, [C.c_int, C.c_int, C.c_uint64, _IPP, _IPP]),
    "bspgemm_gen_rmat": (_INT, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint64, _IPP, _IPP]),
    "bspgemm_gen_powerlaw": (_INT, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint64, _IPP, _IPP]),
    "bspgemm_device_count": (_INT, []),
    "bspgemm_comm_agree": (_INT, [_VP, C.c_int]),
    "bspgemm_comm_inject_failure": (None, [_VP, C.c_int]),
}
EXPORTS = list(_SIGNATURES)


def build():
    """Compile libbspgemm.so in-tree (hipcc --offload-arch=gfx950 + gcc)."""
    subprocess.run(["make", "-C", _ROOT, "-j8"], check=True, stdout=subprocess.DEVNULL)


_lib = None


def hip_runtimes():
    """paths of the libamdhip64 copies mapped into this process (there must be exactly one)"""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    except OSError:
        return []


def check_single_hip_runtime():
    """Two HIP runtimes in one process (torch's bundled libamdhip64 + /opt/rocm's, which
    libbspgemm.so finds through its rpath when it is loaded BEFORE torch) each keep their own
    device state: handles of one are garbage to the other and the process segfaults on the first
    cross call (seen in round 1 as a crash in the RCCL stitch test).  Load order decides: whoever
    is first wins the soname.  Fail loudly instead of crashing later."""
    libs = hip_runtimes()
    if len(libs) > 1:
        raise RuntimeError("two HIP runtimes are mapped into this process: %s -- import torch BEFORE "
                           "loading libbspgemm.so (bspgemm.lib() does that itself), or do not import "
                           "torch at all" % libs)
    return libs


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError("%s is not built: run `make -C binary-spgemm_amd` "
                                "(or __graft_entry__.build())" % LIB_PATH)
    # a process that also uses torch must load torch's bundled HIP runtime first (one runtime only);
    # where torch is not installed at all the library simply uses /opt/rocm's
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401  (a broken torch install raises here: loudly, not a later segfault)
    L = C.CDLL(LIB_PATH)
    check_single_hip_runtime()
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _chk(st, where):
    if st != 0:
        raise BspgemmError(st, where)


def _take_i32(ptr, n):
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(max(int(n), 1),))[: int(n)].copy()
    _libc.free(C.cast(ptr, C.c_void_p))
    return out


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ------------------------------------------------------------------ host utilities --------
READ_EXPAND_SYMMETRIC = 1


def readCOO(path, expand_symmetric=False):
    """bspgemm_readCOO: (row_ptr int32[M+1], col_idx int32[nnz], M, N); CSR of the transposed file.
    expand_symmetric=True: bspgemm_readCOO_ex with BSPGEMM_READ_EXPAND_SYMMETRIC (opt-in, not the
    reference's behaviour)."""
    L = lib()
    rp, ci = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
    m, n, nz = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if expand_symmetric:
        st = L.bspgemm_readCOO_ex(os.fsencode(path), READ_EXPAND_SYMMETRIC, C.byref(rp), C.byref(ci), C.byref(m),
                                  C.byref(n), C.byref(nz))
    else:
        st = L.bspgemm_readCOO(os.fsencode(path), C.byref(rp), C.byref(ci), C.byref(m), C.byref(n), C.byref(nz))
    _chk(st, "readCOO(%s)" % path)
    # the CSR has one row per FILE COLUMN (N); the reference only ever reads square files (n = M)
    return _take_i32(rp, n.value + 1), _take_i32(ci, nz.value), m.value, n.value


def write_mtx(path, row_ptr, col_idx, cols=None):
    row_ptr, col_idx = _i32(row_ptr), _i32(col_idx)
    rows = row_ptr.size - 1
    _chk(lib().bspgemm_write_mtx(os.fsencode(path), rows, rows if cols is None else cols, row_ptr,
                                 col_idx if col_idx.size else np.zeros(1, np.int32)), "write_mtx")


def write_result_mtx(path, row_ptr64, col_idx, cols=None):
    row_ptr64 = np.ascontiguousarray(row_ptr64, dtype=np.int64)
    col_idx = _i32(col_idx)
    rows = row_ptr64.size - 1
    _chk(lib().bspgemm_write_result_mtx(os.fsencode(path), rows, rows if cols is None else cols, row_ptr64,
                                        col_idx if col_idx.size else np.zeros(1, np.int32)), "write_result_mtx")


def csr_equal(rp1, ci1, rp2, ci2):
    rp1 = np.ascontiguousarray(rp1, dtype=np.int64)
    rp2 = np.ascontiguousarray(rp2, dtype=np.int64)
    if rp1.size != rp2.size:
        return False
    return bool(lib().bspgemm_csr_equal64(_i32(ci1), rp1, _i32(ci2), rp2, rp1.size - 1))


def _gen(fn, n, *args):
    rp, ci = C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
    _chk(fn(*args, C.byref(rp), C.byref(ci)), "generator")
    row_ptr = _take_i32(rp, n + 1)
    return row_ptr, _take_i32(ci, row_ptr[-1]), n


def gen_uniform(n, d, seed=1):
    return _gen(lib().bspgemm_gen_uniform, n, n, d, seed)


def gen_rmat(scale, edge_factor=16, abc=(0.30, 0.25, 0.25), seed=1):
    return _gen(lib().bspgemm_gen_rmat, 1 << scale, scale, edge_factor, abc[0], abc[1], abc[2], seed)


def gen_powerlaw(n, mean_degree, alpha=2.1, max_degree=0, seed=1):
    return _gen(lib().bspgemm_gen_powerlaw, n, n, mean_degree, alpha, max_degree, seed)


# ------------------------------------------------------------------ test hooks -------------
def debug_fail_alloc(nth):
    """bspgemm_debug_fail_alloc: the nth device allocation from now (1 = the next) fails, once; 0 disarms"""
    lib().bspgemm_debug_fail_alloc(int(nth))


def debug_alloc_state():
    """bspgemm_debug_alloc_state: (requests so far, live allocations, live bytes, injected failures fired so far)"""
    out = np.zeros(4, dtype=np.int64)
    lib().bspgemm_debug_alloc_state(out)
    return tuple(int(v) for v in out)


def debug_fill_alloc(on, word=0):
    """bspgemm_debug_fill_alloc: while on, every device allocation is handed out filled with the 32-bit `word`"""
    lib().bspgemm_debug_fill_alloc(1 if on else 0, int(word) & 0xFFFFFFFF)


def debug_guard_alloc(on):
    """bspgemm_debug_guard_alloc: while on, every device allocation gets a 256-byte canary zone in front and behind"""
    lib().bspgemm_debug_guard_alloc(1 if on else 0)


def debug_check_guards():
    """bspgemm_debug_check_guards: (guarded allocations found damaged so far, live and freed; the first damage's description
    or "" when there is none)"""
    n = int(lib().bspgemm_debug_check_guards())
    return n, (lib().bspgemm_last_error().decode(errors="replace") if n else "")


# ------------------------------------------------------------------ native handle API -----
class Context:
    """bspgemm_context: one GPU, one stream, reusable workspaces."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        L = lib()
        check_single_hip_runtime()
        _chk(L.bspgemm_create(device, C.byref(self._h)), "bspgemm_create")
        self.device = device
        self._children = weakref.WeakSet()      # matrices/results must go before their context

    def close(self):
        if self._h:
            for ch in list(self._children):
                ch.free()
            lib().bspgemm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr):
        _chk(lib().bspgemm_set_stream(self._h, C.c_void_p(hip_stream_ptr)), "set_stream")

    def synchronize(self):
        _chk(lib().bspgemm_synchronize(self._h), "synchronize")

    def debug_scribble(self, word):
        """bspgemm_debug_scribble: every scratch array the context keeps between calls is filled with the 32-bit `word`"""
        _chk(lib().bspgemm_debug_scribble(self._h, int(word) & 0xFFFFFFFF), "debug_scribble")

    def set_flow(self, flow):
        """"auto" | "upper-bound" | "exact" (BSPGEMM_FLOW_*, include/bspgemm.h)"""
        _chk(lib().bspgemm_set_flow(self._h, FLOWS[flow]), "set_flow")

    def set_option(self, name, value):
        """bspgemm_set_option: "class_streams" 1..3, "blocked_extents" -1/0/1, "check" 0/1, "small_path" -1/0/1, "padded_rows" -1/0/1,
        "shared_slots" -1/0/k, "dot_light" T >= 0, "bfs_alpha" >= 1, "bfs_beta" >= 1, "bfs_push_lanes" 0/4/16/64,
        "lp_min_class" 0..3, "pr_min_class" 0..3, "bc_lanes" 0/4/16/64, "extract_lanes" 0/4/16/64, "match_lanes" 0/4/16/64"""
        _chk(lib().bspgemm_set_option(self._h, OPTIONS[name], int(value)), "set_option(%s)" % name)

    def get_option(self, name):
        return lib().bspgemm_get_option(self._h, OPTIONS[name])

    def set_class_timing(self, on):
        """event brackets around every class launch (stats: ms_bin, t_bin, ...); off by default: they cost ~1 %"""
        _chk(lib().bspgemm_set_class_timing(self._h, 1 if on else 0), "set_class_timing")

    def upload(self, row_ptr, col_idx, cols, row0=0, rows=None):
        """Host CSR -> device.  row0/rows select an interior row range (absolute row_ptr values)."""
        row_ptr, col_idx = _i32(row_ptr), _i32(col_idx)
        rows = row_ptr.size - 1 - row0 if rows is None else rows
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_upload(self._h, rows, cols, C.c_void_p(row_ptr.ctypes.data + 4 * row0),
                                         C.c_void_p(col_idx.ctypes.data), C.byref(m)), "matrix_upload")
        return Matrix(self, m, keep=None)

    def wrap_device(self, rows, cols, nnz, d_row_ptr, d_col_idx, keep=None):
        """Adopt device arrays (e.g. torch tensors' data_ptr()); `keep` holds their owners alive."""
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_wrap_device(self._h, rows, cols, nnz, C.c_void_p(d_row_ptr),
                                              C.c_void_p(d_col_idx), C.byref(m)), "matrix_wrap_device")
        return Matrix(self, m, keep=keep)

    def multiply(self, A, B, row_begin=0, row_end=None):
        row_end = A.rows if row_end is None else row_end
        r = C.c_void_p()
        _chk(lib().bspgemm_multiply(self._h, A._h, B._h, row_begin, row_end, C.byref(r)), "bspgemm_multiply")
        return Result(self, r)

    def multiply_masked(self, A, B, F, row_begin=0, row_end=None, complement=False):
        """C = F .* (A*B); complement=True: C = !F .* (A*B), the product's columns NOT in F's row
        (bspgemm_multiply_masked_ex with BSPGEMM_MASK_COMPLEMENT).  F is indexed by absolute row."""
        row_end = A.rows if row_end is None else row_end
        r = C.c_void_p()
        if complement:
            _chk(lib().bspgemm_multiply_masked_ex(self._h, A._h, B._h, F._h, MASK_COMPLEMENT, row_begin, row_end, C.byref(r)),
                 "bspgemm_multiply_masked_ex")
            return Result(self, r)
        _chk(lib().bspgemm_multiply_masked(self._h, A._h, B._h, F._h, row_begin, row_end, C.byref(r)),
             "bspgemm_multiply_masked")
        return Result(self, r)

    def multiply_accumulate(self, A, B, D, row_begin=0, row_end=None):
        """C = D | (A*B), the OR-accumulating product (bspgemm_multiply_accumulate): D's columns within [0, B.cols) join
        every row's products.  D is indexed by absolute row; C's row_ptr is slice-local."""
        row_end = A.rows if row_end is None else row_end
        r = C.c_void_p()
        _chk(lib().bspgemm_multiply_accumulate(self._h, A._h, B._h, D._h, row_begin, row_end, C.byref(r)),
             "bspgemm_multiply_accumulate")
        return Result(self, r)

    def multiply_masked_count(self, A, B, F, row_begin=0, row_end=None):
        """C = F .* (A*B) with path counts (bspgemm_multiply_masked_count): the masked product's pattern, and for every
        entry the number of products that land on it (Result.download_values).  F is indexed by absolute row."""
        row_end = A.rows if row_end is None else row_end
        r = C.c_void_p()
        _chk(lib().bspgemm_multiply_masked_count(self._h, A._h, B._h, F._h, row_begin, row_end, C.byref(r)),
             "bspgemm_multiply_masked_count")
        return Result(self, r)

    def matrix_from_result(self, result, cols):
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_from_result(self._h, result._h, cols, C.byref(m)), "matrix_from_result")
        return Matrix(self, m, keep=None)

    def matrix_from_result_where(self, result, cols, cmp, threshold):
        """bspgemm_matrix_from_result_where: the entries of a counted result whose count satisfies `count cmp threshold`
        (cmp: ">=" | ">" | "<=" | "<" | "==" | "!=") as a new operand, filtered on the device"""
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_from_result_where(self._h, result._h, cols, COMPARES[cmp], int(threshold), C.byref(m)),
             "matrix_from_result_where")
        return Matrix(self, m, keep=None)

    def select(self, A, op):
        """bspgemm_matrix_select: the entries of A below ("tril") / above ("triu") / off ("offdiag") the diagonal as a new
        operand; a stable filter on the device (order and repeats of every row kept)"""
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_select(self._h, A._h, SELECT_OPS[op], C.byref(m)), "matrix_select")
        return Matrix(self, m, keep=None)

    def setop(self, A, B, op):
        """bspgemm_matrix_setop: the patterns of A and B combined row by row, "or" | "and" | "andnot" | "xor" (or the
        bspgemm_setop value), as a new operand with sorted duplicate-free rows"""
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_setop(self._h, A._h, B._h, SETOPS[op] if isinstance(op, str) else int(op), C.byref(m)),
             "matrix_setop")
        return Matrix(self, m, keep=None)

    def matrix_equal(self, A, B):
        """bspgemm_matrix_equal: whether the two patterns are equal as sets, decided on the device"""
        eq = C.c_int()
        _chk(lib().bspgemm_matrix_equal(self._h, A._h, B._h, C.byref(eq)), "matrix_equal")
        return bool(eq.value)

    def symmetrize(self, A, drop_diagonal=False):
        """bspgemm_matrix_symmetrize: A | A^T of a square operand, without the diagonal when drop_diagonal"""
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_symmetrize(self._h, A._h, SYMMETRIZE_DROP_DIAGONAL if drop_diagonal else 0, C.byref(m)),
             "matrix_symmetrize")
        return Matrix(self, m, keep=None)

    def multiply_masked_dot(self, A, B, F):
        """C = F .* (A * B^T) with counts (bspgemm_multiply_masked_dot): C_ij = |A_i n B_j| for every entry (i, j) of F, one
        sorted-row intersection per mask entry.  Returns (Result, info dict: entries, heavy_entries, kept, canonicalised)."""
        r, info = C.c_void_p(), DotInfo()
        _chk(lib().bspgemm_multiply_masked_dot(self._h, A._h, B._h, F._h, 0, C.byref(r), C.byref(info)),
             "bspgemm_multiply_masked_dot")
        return Result(self, r), info.as_dict()

    def triangle_count(self, A, method="product"):
        """bspgemm_triangle_count: triangles of the undirected graph of A's strictly lower triangle, device-resident;
        method "product" (default) | "dot" (bspgemm_triangle_count_ex): how the support is counted"""
        t = C.c_int64()
        if method == "product":
            _chk(lib().bspgemm_triangle_count(self._h, A._h, C.byref(t)), "triangle_count")
        else:
            _chk(lib().bspgemm_triangle_count_ex(self._h, A._h, SUPPORT_METHODS[method], C.byref(t)), "triangle_count_ex")
        return t.value

    def ktruss(self, A, k, max_iter=0, method="product"):
        """bspgemm_ktruss: (T as a Matrix, counted products computed, converged) -- the maximal subgraph in which every
        edge lies in at least k - 2 triangles, by repeated counted products and on-device selects; max_iter <= 0: no cap;
        method "product" (default) | "dot" (bspgemm_ktruss_ex): how a step counts the support"""
        m, it, conv = C.c_void_p(), C.c_int(), C.c_int()
        if method == "product":
            _chk(lib().bspgemm_ktruss(self._h, A._h, int(k), int(max_iter), C.byref(m), C.byref(it), C.byref(conv)), "ktruss")
        else:
            _chk(lib().bspgemm_ktruss_ex(self._h, A._h, int(k), int(max_iter), SUPPORT_METHODS[method], C.byref(m),
                                         C.byref(it), C.byref(conv)), "ktruss_ex")
        return Matrix(self, m, keep=None), it.value, bool(conv.value)

    def bfs(self, A, sources, max_depth=0):
        """bspgemm_bfs: (levels as a Result, depth, complete) -- row s of the result holds the vertices reachable from
        sources[s] along A's out-edges, Result.download_values() their BFS levels; device-resident, one complement
        product per level; max_depth <= 0: no cap"""
        src = _i32(sources).ravel()
        r, depth, complete = C.c_void_p(), C.c_int(), C.c_int()
        _chk(lib().bspgemm_bfs(self._h, A._h, int(src.size), C.c_void_p(src.ctypes.data) if src.size else None,
                               int(max_depth), C.byref(r), C.byref(depth), C.byref(complete)), "bspgemm_bfs")
        return Result(self, r), depth.value, bool(complete.value)

    def bfs_tree(self, A, AT=None, source=0, direction="auto", max_depth=0):
        """bspgemm_bfs_tree: (tree as a Result, info dict) -- single-source direction-optimising BFS; row v of the result
        holds the one entry (v, parent(v)) with the value level(v) for every vertex reachable from `source` along A's
        out-edges, parent = the smallest vertex one level up, the source its own parent at level 0.  AT: the transpose of A
        (A itself for a symmetric canonical A), or None: the call transposes when it first pulls.  direction "auto" | "push"
        | "pull"; max_depth <= 0: no cap.  info: reached, edges_pushed, pull_mask, depth, complete, push_levels,
        pull_levels, transposed, canonicalised"""
        r, info = C.c_void_p(), BfsTreeInfo()
        _chk(lib().bspgemm_bfs_tree(self._h, A._h, AT._h if AT is not None else None, int(source), BFS_DIRECTIONS[direction],
                                    int(max_depth), C.byref(r), C.byref(info)), "bspgemm_bfs_tree")
        return Result(self, r), info.as_dict()

    def connected_components(self, A):
        """bspgemm_connected_components: (P as a Matrix, ncomponents, rounds) -- the weakly connected components of A's
        graph; P.download()[1] is the label array, label(v) = the smallest vertex id of v's component; device-resident,
        no product"""
        m, nc, rounds = C.c_void_p(), C.c_int(), C.c_int()
        _chk(lib().bspgemm_connected_components(self._h, A._h, C.byref(m), C.byref(nc), C.byref(rounds)),
             "bspgemm_connected_components")
        return Matrix(self, m, keep=None), nc.value, rounds.value

    def core_numbers(self, A):
        """bspgemm_core_numbers: (cores as a Result, degeneracy, rounds) -- row v of the result holds the one entry (v, v),
        Result.download_values()[v] is the core number of v in the simple undirected graph of A's entries; device-resident
        level-synchronous peeling, no product; rounds = peel launches"""
        r, top, rounds = C.c_void_p(), C.c_int(), C.c_int()
        _chk(lib().bspgemm_core_numbers(self._h, A._h, C.byref(r), C.byref(top), C.byref(rounds)), "bspgemm_core_numbers")
        return Result(self, r), top.value, rounds.value

    def kcore(self, A, k):
        """bspgemm_kcore: (T as a Matrix, degeneracy) -- the subgraph of A's simple undirected graph induced by the vertices
        of core number >= k, symmetric with sorted rows and no diagonal; empty for k > degeneracy"""
        m, top = C.c_void_p(), C.c_int()
        _chk(lib().bspgemm_kcore(self._h, A._h, int(k), C.byref(m), C.byref(top)), "bspgemm_kcore")
        return Matrix(self, m, keep=None), top.value

    def strongly_connected_components(self, A):
        """bspgemm_strongly_connected_components: (P as a Matrix, ncomponents, rounds, sweeps) -- the strongly connected
        components of the directed graph whose row u lists u's out-neighbours; P.download()[1] is the label array,
        label(v) = the smallest vertex id of v's component; device-resident trimming and min-colour propagation, no product
        and no transpose; rounds = colouring rounds, sweeps = entry-parallel launches"""
        m, nc, rounds, sweeps = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        _chk(lib().bspgemm_strongly_connected_components(self._h, A._h, C.byref(m), C.byref(nc), C.byref(rounds),
                                                         C.byref(sweeps)), "bspgemm_strongly_connected_components")
        return Matrix(self, m, keep=None), nc.value, rounds.value, sweeps.value

    COLOR_ORDERS = {"natural": 1, "random": 2, "largest": 3, "largest_first": 3}

    def graph_coloring(self, A, order="random", seed=0):
        """bspgemm_graph_coloring: (P as a Matrix, ncolors, rounds) -- the greedy colouring of the simple undirected graph
        of A's entries; P.download()[1] is the colour array, colour(v) = what sequential first fit gives in the order of
        the keys that include/bspgemm.h defines for order ("natural", "random", "largest") and seed; class 0 is a maximal
        independent set; device-resident Jones-Plassmann sweep, no product; rounds = frontier launches"""
        if order not in self.COLOR_ORDERS:
            raise ValueError("order must be one of %s" % sorted(self.COLOR_ORDERS))
        m, nc, rounds = C.c_void_p(), C.c_int(), C.c_int()
        _chk(lib().bspgemm_graph_coloring(self._h, A._h, self.COLOR_ORDERS[order], int(seed) & 0xFFFFFFFF, C.byref(m),
                                          C.byref(nc), C.byref(rounds)), "bspgemm_graph_coloring")
        return Matrix(self, m, keep=None), nc.value, rounds.value

    def label_propagation(self, A, max_iter=10, initial=None):
        """bspgemm_label_propagation: (P as a Matrix, info dict) -- community detection by synchronous label propagation on
        the simple undirected graph of A's entries; P.download()[1] is the label array after max_iter iterations (or at the
        first iteration that changes nothing): every vertex takes the most frequent label among its neighbours, ties to the
        smallest.  initial: n host ints in [0, n), or None for label(v) = v.  info: iterations, converged, communities,
        changed, class_vertices"""
        if initial is not None:
            initial = np.ascontiguousarray(initial, dtype=np.int32)
            if initial.shape != (A.rows,):
                raise ValueError("initial must hold one label per vertex")
        m, info = C.c_void_p(), LpInfo()
        _chk(lib().bspgemm_label_propagation(self._h, A._h, initial.ctypes.data if initial is not None else None, int(max_iter),
                                             C.byref(m), C.byref(info)), "bspgemm_label_propagation")
        return Matrix(self, m, keep=None), info.as_dict()

    def local_clustering(self, A, directed=False):
        """bspgemm_local_clustering: (counts as a Result, degree int32[n], lcc float64[n], info dict) -- the local clustering
        coefficient of every vertex of the simple undirected graph S of A's entries; row v of the result holds the one entry
        (v, v), Result.download_values()[v] = num(v): the ordered pairs of distinct neighbours of v that are joined in S
        (twice the triangles at v), or with directed=True (BSPGEMM_LCC_DIRECTED) joined by an entry of A.  degree = |S_v|,
        lcc = num / (d (d - 1)) in double, 0 where d < 2.  info: triangles, entries, heavy_entries, reciprocal"""
        r, info = C.c_void_p(), LccInfo()
        degree, lcc = np.zeros(A.rows, np.int32), np.zeros(A.rows, np.float64)
        _chk(lib().bspgemm_local_clustering(self._h, A._h, LCC_DIRECTED if directed else 0, C.byref(r),
                                            degree.ctypes.data if A.rows else None, lcc.ctypes.data if A.rows else None,
                                            C.byref(info)), "bspgemm_local_clustering")
        return Result(self, r), degree, lcc, info.as_dict()

    def pagerank(self, A, AT=None, method=PR_AUTO, damping=0.85, max_iter=20, tolerance=0.0):
        """bspgemm_pagerank: (fixed uint64[n], rank float64[n], info dict) -- PageRank of the directed graph whose row u
        lists u's out-neighbours, exact in unsigned 64-bit fixed point (2^62 = 1.0; include/bspgemm.h holds the definition):
        the same bits on every run and under either method.  AT: the transpose of A (A itself for a symmetric canonical A),
        or None: a PULL call transposes A itself.  method PR_AUTO | PR_PULL | PR_PUSH; tolerance 0: exactly max_iter
        iterations, else the loop ends at the first iteration whose L1 change is at most tolerance.  rank = fixed * 2**-62.
        info: mass, delta, dangling, class_vertices, iterations, converged, method, transposed, canonicalised"""
        fixed, rank, info = np.zeros(A.rows, np.uint64), np.zeros(A.rows, np.float64), PrInfo()
        _chk(lib().bspgemm_pagerank(self._h, A._h, AT._h if AT is not None else None, int(method), float(damping), int(max_iter),
                                    float(tolerance), fixed.ctypes.data if A.rows else None,
                                    rank.ctypes.data if A.rows else None, C.byref(info)), "bspgemm_pagerank")
        return fixed, rank, info.as_dict()

    def betweenness(self, A, sources):
        """bspgemm_betweenness: (fixed uint64[n], bc float64[n], info dict) -- Brandes' unnormalised betweenness centrality of
        the directed graph whose row u lists u's out-neighbours, restricted to the given sources (a vertex named twice
        counts twice), exact in 64-bit integers with 2^32 = 1.0 (include/bspgemm.h holds the definition): the same bits on
        every run and under every "bc_lanes".  For a symmetric A and all n sources it is twice the undirected betweenness.
        bc = fixed * 2**-32.  info: sigma_max, reached, edges_forward, hub_chunks, sources, depth_max, levels, canonicalised"""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        fixed, bc, info = np.zeros(A.rows, np.uint64), np.zeros(A.rows, np.float64), BcInfo()
        _chk(lib().bspgemm_betweenness(self._h, A._h, int(src.size), src.ctypes.data if src.size else None,
                                       fixed.ctypes.data if A.rows else None, bc.ctypes.data if A.rows else None,
                                       C.byref(info)), "bspgemm_betweenness")
        return fixed, bc, info.as_dict()

    MATCH_ORDERS = {"natural": 1, "random": 2, "light": 3}

    def maximal_matching(self, A, order="random", seed=0, mate=False):
        """bspgemm_maximal_matching: (P as a Matrix, mate int32[n] or None, info dict) -- the maximal matching of the simple
        undirected graph of A's entries that sequential greedy gives in the edge order that include/bspgemm.h defines for
        order ("natural", "random", "light") and seed: the same bits on every run and under every "match_lanes".
        P.download()[1][v] = min(v, mate(v)), v itself when v is unmatched, so P^T * S * P is the contracted graph; mate=True
        also returns the partners, -1 = unmatched.  info: pairs, entries_walked, hub_chunks, rounds, lanes"""
        if order not in self.MATCH_ORDERS:
            raise ValueError("order must be one of %s" % sorted(self.MATCH_ORDERS))
        m, info = C.c_void_p(), MatchInfo()
        mates = np.zeros(A.rows, np.int32) if mate else None
        _chk(lib().bspgemm_maximal_matching(self._h, A._h, self.MATCH_ORDERS[order], int(seed) & 0xFFFFFFFF, C.byref(m),
                                            mates.ctypes.data if mate and A.rows else None, C.byref(info)),
             "bspgemm_maximal_matching")
        return Matrix(self, m, keep=None), mates, info.as_dict()

    def weights_upload(self, A, w):
        """bspgemm_weights_upload: a Weights handle with w[k] (uint32) as the length of stored entry k of A, that is of
        A.download()[1][k]"""
        w = np.ascontiguousarray(w, dtype=np.uint32).reshape(-1)
        if w.size != A.nnz:
            raise ValueError("%d weights for an operand of %d entries" % (w.size, A.nnz))
        h = C.c_void_p()
        _chk(lib().bspgemm_weights_upload(self._h, A._h, w.ctypes.data if w.size else None, C.byref(h)), "bspgemm_weights_upload")
        return Weights(self, h, A)

    def weights_hashed(self, A, seed, wmin, wmax, symmetric=False):
        """bspgemm_weights_hashed: a Weights handle with the hashed lengths of include/bspgemm.h in [wmin, wmax], generated on
        the device; symmetric=True: both directions of an edge weigh the same"""
        h = C.c_void_p()
        _chk(lib().bspgemm_weights_hashed(self._h, A._h, int(seed) & 0xFFFFFFFF, int(wmin), int(wmax),
                                          WEIGHTS_SYMMETRIC if symmetric else 0, C.byref(h)), "bspgemm_weights_hashed")
        return Weights(self, h, A)

    def sssp(self, A, W, source, delta=0, lanes=0, parents=False):
        """bspgemm_sssp: (dist uint64[n], parent int32[n] or None, info dict) -- the exact shortest distances from `source`
        under the lengths W (2**64 - 1 = unreached) and, with parents=True, the smallest tight predecessor of every
        vertex (-1 = unreached): the same bits on every run and under every delta (0 = the default bucket width) and lanes
        (0, 4, 16, 64).  info: delta, dist_max, reached, entries_walked, improved, hub_chunks, rounds, buckets, lanes, reserved"""
        dist = np.zeros(A.rows, np.uint64)
        parent = np.zeros(A.rows, np.int32) if parents else None
        params, info = SsspParams(int(delta), int(lanes), 0), SsspInfo()
        _chk(lib().bspgemm_sssp(self._h, A._h, W._h, int(source), C.byref(params), dist.ctypes.data if A.rows else None,
                                parent.ctypes.data if parents and A.rows else None, C.byref(info)), "bspgemm_sssp")
        return dist, parent, info.as_dict()

    def extract(self, A, rows=None, cols=None, keep_shape=False):
        """bspgemm_matrix_extract: (Matrix, info dict) -- out = A[rows, cols] on the device.  rows / cols: int sequences, None =
        all in order.  Default: out is len(rows) x len(cols), entry (r, c) where A has (rows[r], cols[c]); rows may repeat, cols
        must not.  keep_shape=True: A's shape, the entries (i, j) of A with i in rows and j in cols (D_I * A * D_J).  The rows
        of out are ascending and duplicate-free.  info: kept, scanned, hub_chunks, lanes, cols_monotone, sorted_by,
        canonicalised."""
        I = None if rows is None else _i32(np.asarray(rows).reshape(-1))
        J = None if cols is None else _i32(np.asarray(cols).reshape(-1))
        keep = (C.c_int * 1)()                              # (an empty array's data pointer may be NULL, which means "all")
        pi = None if I is None else C.c_void_p(I.ctypes.data if I.size else C.addressof(keep))
        pj = None if J is None else C.c_void_p(J.ctypes.data if J.size else C.addressof(keep))
        m, info = C.c_void_p(), ExtractInfo()
        _chk(lib().bspgemm_matrix_extract(self._h, A._h, 0 if I is None else int(I.size), pi, 0 if J is None else int(J.size), pj,
                                          EXTRACT_KEEP_SHAPE if keep_shape else 0, C.byref(m), C.byref(info)),
             "bspgemm_matrix_extract")
        return Matrix(self, m, keep=None), info.as_dict()

    def extract_rows_of(self, A, MI=None, ri=-1, MJ=None, rj=-1, keep_shape=False):
        """bspgemm_matrix_extract_rows_of: (Matrix, info dict) -- as extract, with the lists read on the device: the stored
        col_idx of row ri of MI and of row rj of MJ (-1: the operand's whole col_idx in storage order; None: all)."""
        m, info = C.c_void_p(), ExtractInfo()
        _chk(lib().bspgemm_matrix_extract_rows_of(self._h, A._h, None if MI is None else MI._h, int(ri),
                                                  None if MJ is None else MJ._h, int(rj),
                                                  EXTRACT_KEEP_SHAPE if keep_shape else 0, C.byref(m), C.byref(info)),
             "bspgemm_matrix_extract_rows_of")
        return Matrix(self, m, keep=None), info.as_dict()

    def transpose(self, A):
        """bspgemm_matrix_transpose: pattern(A)^T as a new operand on the device (rows ascending, duplicates dropped)"""
        m = C.c_void_p()
        _chk(lib().bspgemm_matrix_transpose(self._h, A._h, C.byref(m)), "matrix_transpose")
        return Matrix(self, m, keep=None)

    def closure(self, A, max_iter=64, transitive=False):
        """reflexive-transitive closure A* by repeated squaring; transitive=True: A+ (paths of length >= 1) by
        T = T | T*T (bspgemm_closure_ex with BSPGEMM_CLOSURE_TRANSITIVE).  Returns (Result, products computed)"""
        r, it = C.c_void_p(), C.c_int()
        if transitive:
            _chk(lib().bspgemm_closure_ex(self._h, A._h, CLOSURE_TRANSITIVE, max_iter, C.byref(r), C.byref(it)),
                 "bspgemm_closure_ex")
        else:
            _chk(lib().bspgemm_closure(self._h, A._h, max_iter, C.byref(r), C.byref(it)), "bspgemm_closure")
        return Result(self, r), it.value

    def lengths_to_row_ptr(self, d_lengths, world, width, bounds, d_row_ptr, hip_stream=None):
        """gathered int32 row lengths (device) -> global int64 row_ptr (device); see bspgemm.h"""
        b = np.ascontiguousarray(bounds, dtype=np.int32)
        _chk(lib().bspgemm_lengths_to_row_ptr(self._h, C.c_void_p(int(d_lengths)), int(world), int(width), b,
                                              C.c_void_p(int(d_row_ptr)), C.c_void_p(hip_stream or 0)), "lengths_to_row_ptr")

    def stats(self, age=0):
        """counters and HIP-event times of the last multiply (age 0) or of an earlier one (age <= 15)"""
        s = Stats()
        _chk(lib().bspgemm_stats_at(self._h, age, C.byref(s)), "stats_at")
        return s.as_dict()

    def row_work_prefix(self, A, B):
        out = np.zeros(A.rows + 1, dtype=np.int64)
        _chk(lib().bspgemm_row_work_prefix(self._h, A._h, B._h, out), "row_work_prefix")
        return out

    def partition_rows(self, A, B, parts):
        out = np.zeros(parts + 1, dtype=np.int32)
        _chk(lib().bspgemm_partition_rows(self._h, A._h, B._h, parts, out), "partition_rows")
        return out


class Matrix:
    def __init__(self, ctx, handle, keep):
        self.ctx, self._h, self._keep = ctx, handle, keep
        ctx._children.add(self)
        self.rows = lib().bspgemm_matrix_rows(handle)
        self.cols = lib().bspgemm_matrix_cols(handle)
        self.nnz = lib().bspgemm_matrix_nnz(handle)

    def invalidate(self):
        """bspgemm_matrix_invalidate: the wrapped device arrays were rewritten in place; derived tables are rebuilt"""
        _chk(lib().bspgemm_matrix_invalidate(self._h), "matrix_invalidate")

    @property
    def uses_blocked_table(self):
        """1 / 0 once the operand has been used as B (which prepass kernel it gets), -1 before"""
        return lib().bspgemm_matrix_uses_blocked_table(self._h)

    @property
    def uses_padded_rows(self):
        """1 / 0 once the operand has been used as B (whether its rows are gathered from the padded copy), -1 before"""
        return lib().bspgemm_matrix_uses_padded_rows(self._h)

    def download(self):
        """bspgemm_matrix_download: (row_ptr int32[rows+1], col_idx int32[nnz]) as stored on the device"""
        rp = np.zeros(self.rows + 1, dtype=np.int32)
        ci = np.zeros(self.nnz, dtype=np.int32)
        _chk(lib().bspgemm_matrix_download(self.ctx._h, self._h, C.c_void_p(rp.ctypes.data),
                                           C.c_void_p(ci.ctypes.data) if self.nnz else None), "matrix_download")
        return rp, ci

    def free(self):
        if self._h:
            lib().bspgemm_matrix_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Weights:
    """bspgemm_weights: one uint32 per stored entry of the operand A, on the device"""

    def __init__(self, ctx, handle, A):
        self.ctx, self._h, self._A = ctx, handle, A             # (A must outlive its weights)
        ctx._children.add(self)
        self.nnz = lib().bspgemm_weights_nnz(handle)
        self.sum = lib().bspgemm_weights_sum(handle)

    def download(self):
        """bspgemm_weights_download: uint32[nnz], aligned with A.download()[1]"""
        w = np.zeros(self.nnz, dtype=np.uint32)
        _chk(lib().bspgemm_weights_download(self.ctx._h, self._h, w.ctypes.data if self.nnz else None), "weights_download")
        return w

    def free(self):
        if self._h:
            lib().bspgemm_weights_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Result:
    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        ctx._children.add(self)
        self.rows = lib().bspgemm_result_rows(handle)
        self.nnz = lib().bspgemm_result_nnz(handle)

    @property
    def row_ptr_device(self):
        return lib().bspgemm_result_row_ptr_device(self._h)

    @property
    def col_idx_device(self):
        return lib().bspgemm_result_col_idx_device(self._h)

    @property
    def values_device(self):
        """device pointer of the counts of a counted result (Context.multiply_masked_count); None for a pattern-only one"""
        return lib().bspgemm_result_values_device(self._h)

    def values_sum(self):
        """bspgemm_result_values_sum: the exact sum of a counted result's counts, reduced on the device"""
        t = C.c_int64()
        _chk(lib().bspgemm_result_values_sum(self.ctx._h, self._h, C.byref(t)), "result_values_sum")
        return t.value

    def download_values(self):
        """the counts of a counted result, aligned with download()'s col_idx, as np.int32"""
        v = np.zeros(self.nnz, dtype=np.int32)
        _chk(lib().bspgemm_result_download_values(self.ctx._h, self._h, C.c_void_p(v.ctypes.data)), "result_download_values")
        return v

    def download(self, col_idx=True):
        rp = np.zeros(self.rows + 1, dtype=np.int64)
        ci = np.zeros(self.nnz if col_idx else 0, dtype=np.int32)
        _chk(lib().bspgemm_result_download(self.ctx._h, self._h, C.c_void_p(rp.ctypes.data),
                                           C.c_void_p(ci.ctypes.data) if (col_idx and self.nnz) else None),
             "result_download")
        return rp, ci

    def free(self):
        if self._h:
            lib().bspgemm_result_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ------------------------------------------------------------------ int32 drop-ins --------
def SpGEMM_hip(Acol, Arow, An, Bcol, Brow, Bm, tBlock=0, row0=0):
    """SpGEMM_omp-shaped call (final/SpGEMM_mpi_omp.c:71-74).  Returns (Crow int32[An+1], Ccol)."""
    Acol, Arow, Bcol, Brow = map(_i32, (Acol, Arow, Bcol, Brow))
    crow = np.zeros(An + 1, dtype=np.int32)
    cc = C.POINTER(C.c_int)()
    st = lib().SpGEMM_hip(Acol, C.c_void_p(Arow.ctypes.data + 4 * row0), An, Bcol, Brow, Bm, C.byref(cc), crow, tBlock)
    _chk(st, "SpGEMM_hip")
    return crow, _take_i32(cc, crow[-1])


def SpGEMM_hip_bigslice(Acol, Arow, An, Bcol, Brow, Bm, start_row, end_row):
    Acol, Arow, Bcol, Brow = map(_i32, (Acol, Arow, Bcol, Brow))
    crow = np.zeros(end_row - start_row + 1, dtype=np.int32)
    csize = C.c_int(max(Bm, 1))
    _libc.malloc.restype = C.c_void_p
    _libc.malloc.argtypes = [C.c_size_t]
    cc = C.cast(_libc.malloc(csize.value * 4), C.POINTER(C.c_int))
    st = lib().SpGEMM_hip_bigslice(Acol, Arow, An, Bcol, Brow, Bm, C.byref(cc), crow, C.byref(csize), start_row, end_row)
    _chk(st, "SpGEMM_hip_bigslice")
    return crow, _take_i32(cc, crow[-1])


def SpGEMM_hip_mat(Acol, Arow, An, Bcol, Brow, Bm, nnz_c):
    Acol, Arow, Bcol, Brow = map(_i32, (Acol, Arow, Bcol, Brow))
    crow = np.zeros(An + 1, dtype=np.int32)
    ccol = np.zeros(max(int(nnz_c), 1), dtype=np.int32)
    _chk(lib().SpGEMM_hip_mat(Acol, Arow, An, Bcol, Brow, Bm, ccol, crow), "SpGEMM_hip_mat")
    return crow, ccol[: int(nnz_c)]


def SpGEMM_hip_masked(Acol, Arow, An, Bcol, Brow, Bm, Fcol, Frow):
    """SpGEMM_masked-shaped call (final/SpGEMM_mpi_omp.c:232-235): C = F .* (A*B)."""
    Acol, Arow, Bcol, Brow, Fcol, Frow = map(_i32, (Acol, Arow, Bcol, Brow, Fcol, Frow))
    crow = np.zeros(An + 1, dtype=np.int32)
    csize = C.c_int(max(An, 1))
    _libc.malloc.restype = C.c_void_p
    _libc.malloc.argtypes = [C.c_size_t]
    cc = C.cast(_libc.malloc(csize.value * 4), C.POINTER(C.c_int))
    st = lib().SpGEMM_hip_masked(Acol, Arow, An, Bcol, Brow, Bm, Fcol, Frow, C.byref(cc), crow, C.byref(csize))
    _chk(st, "SpGEMM_hip_masked")
    return crow, _take_i32(cc, crow[-1])
