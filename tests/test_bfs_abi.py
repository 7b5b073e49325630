"""The device-resident multi-source BFS (bspgemm_bfs) at the ABI level, without a GPU: the header declares it with the
agreed argument list behind bspgemm_ktruss, the library exports it, the Python view has it, a C99 caller compiles cleanly,
NULL arguments and nsources = 0 are refused by name -- and the tests' own reference (bfs_ref.py) agrees with a hand example.
"""
import ctypes as C

import numpy as np

import bfs_ref
import bspgemm
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, compile_c99, last_error


DECLARATION = ("bspgemm_status bspgemm_bfs(bspgemm_context *ctx, const bspgemm_matrix *A, int nsources, const int *sources, "
               "int max_depth, bspgemm_result **levels, int *depth, int *complete);")


def test_header_declares_bfs_behind_ktruss():
    code = header_code()
    assert DECLARATION in code, "include/bspgemm.h does not declare bspgemm_bfs as agreed"
    assert code.index("bspgemm_ktruss(") < code.index("bspgemm_bfs(") < code.index("bspgemm_closure(")


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, "bspgemm_bfs"), "bspgemm_bfs is not exported by libbspgemm.so"
    assert "bspgemm_bfs" in bspgemm.EXPORTS
    assert len(L.bspgemm_bfs.argtypes) == 8
    assert callable(getattr(bspgemm.Context, "bfs", None)), "Context.bfs"


C99_CALLER = r"""
#include "bspgemm.h"
/* the sum of the levels of the vertices at distance d from any source, and how many there are */
int level_d(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int nsources, const int *sources, int d, int64_t *count,
            int64_t *sum)
{
    bspgemm_result *levels = 0;
    bspgemm_matrix *frontier = 0;
    int depth = 0, complete = 0;
    if (bspgemm_bfs(ctx, A, nsources, sources, 0, &levels, &depth, &complete) != BSPGEMM_OK) return 1;
    if (bspgemm_matrix_from_result_where(ctx, levels, n, BSPGEMM_CMP_EQ, d, &frontier) != BSPGEMM_OK) return 1;
    if (bspgemm_result_values_sum(ctx, levels, sum) != BSPGEMM_OK) return 1;
    *count = bspgemm_matrix_nnz(frontier);
    bspgemm_matrix_free(frontier);
    bspgemm_result_free(levels);
    if (bspgemm_bfs(ctx, A, nsources, sources, d, &levels, 0, 0) != BSPGEMM_OK) return 1;
    bspgemm_result_free(levels);
    return complete ? 0 : depth;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_and_no_sources_are_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the NULL argument or the count is refused first
    src = (C.c_int * 2)(0, 1)
    sentinel, last = SENTINEL, last_error

    for ctx, A, sources in ((None, fake, src), (fake, None, src), (fake, fake, None)):
        out, depth, complete = C.c_void_p(sentinel), C.c_int(7), C.c_int(7)
        assert L.bspgemm_bfs(ctx, A, 2, sources, 0, C.byref(out), C.byref(depth), C.byref(complete)) == ERR_INVALID
        assert not out.value and "bspgemm_bfs" in last() and "NULL" in last(), last()
    assert L.bspgemm_bfs(fake, fake, 2, src, 0, None, None, None) == ERR_INVALID and "bspgemm_bfs" in last()
    for nsources in (0, -3):
        out = C.c_void_p(sentinel)
        assert L.bspgemm_bfs(fake, fake, nsources, src, 0, C.byref(out), None, None) == ERR_INVALID
        assert not out.value and "bspgemm_bfs" in last() and "nsources" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def test_bfs_ref_on_a_hand_example():
    # 0 -> 1, 0 -> 2, 1 -> 3, 2 -> 3, 3 -> 0, 4 -> 3, 4 -> 5 (5 has no out-edge); row 0 is unsorted and repeats an entry
    rp = np.array([0, 3, 4, 5, 6, 8, 8], np.int32)
    ci = np.array([2, 1, 2, 3, 3, 0, 5, 3], np.int32)
    (r, c, v), depth, complete = bfs_ref.bfs_ref(rp, ci, 6, [0, 4, 5, 0])
    assert r.tolist() == [0, 4, 10, 11, 15]
    assert c.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 5, 0, 1, 2, 3]
    assert v.tolist() == [0, 1, 1, 2, 2, 3, 3, 1, 0, 1, 0, 0, 1, 1, 2]
    assert (depth, complete) == (3, 1)
    assert bfs_ref.frontier_sizes(bfs_ref.distances(rp, ci, 6, [0, 4, 5, 0])) == [4, 6, 3, 2]
    # the cut at one edge: the cap ends the search; at three: the last level is in, the cap still ended it
    (r, c, v), depth, complete = bfs_ref.bfs_ref(rp, ci, 6, [0, 4, 5, 0], max_depth=1)
    assert (r.tolist(), c.tolist(), v.tolist()) == ([0, 3, 6, 7, 10], [0, 1, 2, 3, 4, 5, 5, 0, 1, 2], [0, 1, 1, 1, 0, 1, 0, 0, 1, 1])
    assert (depth, complete) == (1, 0)
    assert bfs_ref.bfs_ref(rp, ci, 6, [0, 4, 5, 0], max_depth=3)[1:] == (3, 0)
    assert bfs_ref.bfs_ref(rp, ci, 6, [0, 4, 5, 0], max_depth=4)[1:] == (3, 1)
    # every source reaches every vertex: complete even when the cap is the depth
    c_rp, c_ci, n = bfs_ref.complete(5)
    (r, c, v), depth, complete = bfs_ref.bfs_ref(c_rp, c_ci, n, np.arange(n), max_depth=1)
    assert r.tolist() == [0, 5, 10, 15, 20, 25] and v.sum() == 20 and (depth, complete) == (1, 1)


def test_layered_graph_has_the_layers_it_promises():
    layers = [1, 62, 1, 1, 4030, 1, 1, 3, 4095]
    rp, ci, n, ids = bfs_ref.layered(layers, 2, 11)
    assert n == sum(layers) + 2 and n % 4 != 0
    dist = bfs_ref.distances(rp, ci, n, [ids[0][0]])
    assert bfs_ref.frontier_sizes(dist) == layers
    for k, members in enumerate(ids):
        assert (dist[0, members] == k).all()
