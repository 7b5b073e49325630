"""The device-resident k-core decomposition (bspgemm_core_numbers, bspgemm_kcore) at the ABI level, without a GPU: the
header declares both with the agreed argument lists between bspgemm_connected_components and bspgemm_closure, the library
exports them, the Python view has them, a C99 caller compiles cleanly, NULL arguments are refused by name -- and the tests'
own reference (kcore_ref.py) agrees with networkx on every named graph and with a hand example, and the graph builders have
the shapes they promise.
"""
import ctypes as C
import functools

import networkx as nx
import numpy as np
import pytest

import bspgemm
import kcore_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, compile_c99, last_error


DECLARATIONS = {
    "bspgemm_core_numbers":
        "bspgemm_status bspgemm_core_numbers(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_result **cores, "
        "int *degeneracy, int *rounds);",
    "bspgemm_kcore":
        "bspgemm_status bspgemm_kcore(bspgemm_context *ctx, const bspgemm_matrix *A, int k, bspgemm_matrix **T, "
        "int *degeneracy);",
}


def test_header_declares_them_between_components_and_closure():
    code = header_code()
    for name, decl in DECLARATIONS.items():
        assert decl in code, "include/bspgemm.h does not declare %s as agreed" % name
    assert (code.index("bspgemm_connected_components(") < code.index("bspgemm_core_numbers(") < code.index("bspgemm_kcore(")
            < code.index("bspgemm_closure("))


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    for name in DECLARATIONS:
        assert hasattr(L, name), "%s is not exported by libbspgemm.so" % name
        assert name in bspgemm.EXPORTS
        assert len(getattr(L, name).argtypes) == 5
    assert callable(getattr(bspgemm.Context, "core_numbers", None)), "Context.core_numbers"
    assert callable(getattr(bspgemm.Context, "kcore", None)), "Context.kcore"


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the edges (stored both ways) of the innermost core; *size = its vertices */
long long innermost_core(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int *size)
{
    bspgemm_result *cores = 0;
    bspgemm_matrix *shell = 0, *T = 0;
    int degeneracy = 0, rounds = 0, again = 0;
    long long edges;
    if (bspgemm_core_numbers(ctx, A, &cores, &degeneracy, &rounds) != BSPGEMM_OK) return -1;
    if (bspgemm_matrix_from_result_where(ctx, cores, n, BSPGEMM_CMP_EQ, degeneracy, &shell) != BSPGEMM_OK) {
        bspgemm_result_free(cores);
        return -1;
    }
    *size = (int)bspgemm_matrix_nnz(shell);
    bspgemm_matrix_free(shell);
    bspgemm_result_free(cores);
    if (bspgemm_core_numbers(ctx, A, &cores, 0, 0) != BSPGEMM_OK) return -1;
    bspgemm_result_free(cores);
    if (bspgemm_kcore(ctx, A, degeneracy, &T, &again) != BSPGEMM_OK || again != degeneracy) return -1;
    edges = (long long)bspgemm_matrix_nnz(T);
    bspgemm_matrix_free(T);
    if (bspgemm_kcore(ctx, A, degeneracy + 1, &T, 0) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(T);
    return edges;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    for ctx, A in ((None, fake), (fake, None)):
        out, top, rounds = C.c_void_p(sentinel), C.c_int(7), C.c_int(7)
        assert L.bspgemm_core_numbers(ctx, A, C.byref(out), C.byref(top), C.byref(rounds)) == ERR_INVALID
        assert not out.value and "bspgemm_core_numbers" in last() and "NULL" in last(), last()
        assert (top.value, rounds.value) == (0, 0)
        out, top = C.c_void_p(sentinel), C.c_int(7)
        assert L.bspgemm_kcore(ctx, A, 2, C.byref(out), C.byref(top)) == ERR_INVALID
        assert not out.value and "bspgemm_kcore" in last() and "NULL" in last(), last()
    assert L.bspgemm_core_numbers(fake, fake, None, None, None) == ERR_INVALID
    assert "bspgemm_core_numbers" in last() and "NULL" in last(), last()
    assert L.bspgemm_kcore(fake, fake, 2, None, None) == ERR_INVALID
    assert "bspgemm_kcore" in last() and "NULL" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
@functools.lru_cache(maxsize=None)
def _ref(name):
    """(core, degeneracy, rounds) of the named graph; computed once and read-only"""
    core, top, rounds = kcore_ref.core_numbers(*kcore_ref.GRAPHS[name]())
    core.setflags(write=False)
    return core, top, rounds


def _max_degree(name):
    rp, ci, n = kcore_ref.GRAPHS[name]()
    return int(np.diff(kcore_ref.simple(rp, ci, n)[0]).max())


@pytest.mark.parametrize("name", list(kcore_ref.GRAPHS))
def test_reference_equals_networkx(name):
    rp, ci, n = kcore_ref.GRAPHS[name]()
    srp, sci = kcore_ref.simple(rp, ci, n)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(np.repeat(np.arange(n), np.diff(srp)).tolist(), sci.tolist()))
    by_vertex = nx.core_number(G)
    core, top, rounds = _ref(name)
    assert core.dtype == np.int32 and core.tolist() == [by_vertex[v] for v in range(n)]
    assert top == (max(by_vertex.values()) if n else 0)
    assert (rounds == 0) == (sci.size == 0)


def test_reference_on_a_hand_example():
    # a triangle 0-1-2 with the tail 2-3-4, the edge 5-6 stored both ways and twice, a self-loop on 7, 8 alone; row 2 is
    # unsorted.  Level 0: {7, 8}.  Level 1: {4, 5, 6}, then {3}.  Level 2: {0, 1, 2}.
    rp = np.array([0, 2, 3, 5, 6, 6, 8, 9, 10, 10], np.int32)
    ci = np.array([1, 2, 2, 3, 0, 4, 6, 6, 5, 7], np.int32)
    srp, sci = kcore_ref.simple(rp, ci, 9)
    assert srp.tolist() == [0, 2, 4, 7, 9, 10, 11, 12, 12, 12]
    assert sci.tolist() == [1, 2, 0, 2, 0, 1, 3, 2, 4, 3, 6, 5]
    core, top, rounds = kcore_ref.core_numbers(rp, ci, 9)
    assert core.dtype == np.int32 and core.tolist() == [2, 2, 2, 1, 1, 1, 1, 0, 0] and (top, rounds) == (2, 4)
    k_rp, k_ci = kcore_ref.kcore(rp, ci, 9, 2)
    assert k_rp.tolist() == [0, 2, 4, 6, 6, 6, 6, 6, 6, 6] and k_ci.tolist() == [1, 2, 0, 2, 0, 1]
    k_rp, k_ci = kcore_ref.kcore(rp, ci, 9, 1)
    assert k_rp.tolist() == srp.tolist() and k_ci.tolist() == sci.tolist()          # the isolated vertices had no entries
    assert kcore_ref.kcore(rp, ci, 9, 3)[1].size == 0
    core, top, rounds = kcore_ref.core_numbers(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)
    assert core.size == 0 and (top, rounds) == (0, 0)
    assert kcore_ref.core_numbers(np.zeros(4, np.int32), np.zeros(0, np.int32), 3)[0].tolist() == [0, 0, 0]


def test_builders_have_the_shapes_they_promise():
    core, top, rounds = _ref("path200")
    assert (core == 1).all() and rounds == 100
    assert _ref("path200_reversed")[2] == 100
    assert _ref("path4099_permuted")[2] == 2050
    core, top, rounds = _ref("cycle200")
    assert (core == 2).all() and rounds == 1
    for name in ("star_hub_last", "star_hub_middle", "star_leaf_rows"):
        core, top, rounds = _ref(name)
        assert (core == 1).all() and rounds == 2 and _max_degree(name) == 5000
    for m in (63, 65, 257):
        rp, ci, n = kcore_ref.GRAPHS["spider%d" % m]()
        core, top, rounds = _ref("spider%d" % m)
        assert n == 2 * m + 1 and (core == 1).all() and rounds == 3
        deg = np.diff(kcore_ref.simple(rp, ci, n)[0])
        assert int((deg == 1).sum()) == m and int((deg == 2).sum()) == m and deg[0] == m    # frontiers: m leaves, m children
    core, top, rounds = _ref("cliques64_66")
    assert core.tolist() == [63] * 64 + [64] * 65 + [65] * 66 and rounds == 3
    assert sorted(set(np.diff(kcore_ref.simple(*kcore_ref.GRAPHS["cliques64_66"]())[0]).tolist())) == [63, 64, 65]
    core, top, rounds = _ref("cliques2_40")
    assert core.size == 819 and np.unique(core).tolist() == list(range(1, 40)) and rounds == 39
    core, top, rounds = _ref("clique70_tail130")
    assert int((core == 1).sum()) == 130 and int((core == 69).sum()) == 70 and core.size == 200 and rounds == 131
    assert np.unique(core).tolist() == [1, 69]                                       # the level jumps 1 -> 69
    core, top, rounds = _ref("rmat12")
    assert (top, np.unique(core).size, rounds, _max_degree("rmat12")) == (43, 35, 95, 954)
    assert _ref("rmat10")[1:] == (22, 68)
    core, top, rounds = _ref("powerlaw")
    assert (top, rounds, _max_degree("powerlaw")) == (13, 52, 1839)
    assert _ref("uniform4096_d8")[1:] == (12, 37)
    core, top, rounds = _ref("untidy300")
    assert (top, np.unique(core).size, rounds) == (2, 3, 14)
    for n in (257, 1023, 4099):
        core, top, rounds = _ref("chains%d" % n)
        longest = (n + 2) // 3                                                       # vertices of the chain v = 0 mod 3
        assert n % 4 and n % 64 and n % 256 and (core == 1).all() and rounds == (longest + 1) // 2
    for name in ("empty0", "empty1", "empty4", "empty1000", "self_loop"):
        core, top, rounds = _ref(name)
        assert not core.any() and (top, rounds) == (0, 0)
