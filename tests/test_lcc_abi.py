"""The device-resident local clustering coefficient (bspgemm_local_clustering) at the ABI level, without a GPU: the header
declares the flag, the info struct and the function with the agreed argument list between bspgemm_label_propagation and
bspgemm_closure, the library exports it, the Python view has it, a C99 caller compiles cleanly, NULL arguments and unknown
flags are refused by name before anything is dereferenced -- and the tests' own reference (lcc_ref.py) equals a naive
set-per-vertex implementation on every small graph, reproduces the examples worked by hand, and has the symmetries the
header promises.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import cc_ref
import gen
import kcore_ref
import lcc_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, header_text, compile_c99, last_error, dirtied, is_zeroed

NAME = "bspgemm_local_clustering"

FLAG = "#define BSPGEMM_LCC_DIRECTED 1u"
STRUCT = ("typedef struct bspgemm_lcc_info { int64_t triangles; int64_t entries; int64_t heavy_entries; int64_t reciprocal; } "
          "bspgemm_lcc_info;")
DECLARATION = ("bspgemm_status bspgemm_local_clustering(bspgemm_context *ctx, const bspgemm_matrix *A, unsigned flags, "
               "bspgemm_result **counts, int *degree_host, double *lcc_host, bspgemm_lcc_info *info);")


def test_header_declares_it_between_label_propagation_and_closure():
    code = header_code()
    assert FLAG in code and STRUCT in code, "include/bspgemm.h does not declare BSPGEMM_LCC_DIRECTED and bspgemm_lcc_info as agreed"
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_label_propagation(") < code.index(FLAG) < code.index(STRUCT) < code.index(NAME + "(") \
        < code.index("bspgemm_closure(")
    comment = header_text().split("#define BSPGEMM_LCC_DIRECTED")[0].rsplit("/*", 1)[1]
    # the definition is the contract
    for word in ("BSPGEMM_SYMMETRIZE_DROP_DIAGONAL", "2 * triangles(v)", "BSPGEMM_LCC_DIRECTED", "repeats count once",
                 "union of in- and out-neighbours", "invariant under", "in-edges", "symmetric A", "0.0 when d(v) < 2",
                 "(double)num / ((double)d * (double)(d - 1))", "no tolerance", "INT_MAX", "BSPGEMM_OPT_DOT_LIGHT",
                 "BSPGEMM_LCC_TIMING", "zeros are stored", "bspgemm_matrix_from_result_where", "nnz(S) == 0",
                 "statistics", "Nothing is leaked"):
        assert word in comment, word


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 7
    assert callable(getattr(bspgemm.Context, "local_clustering", None)), "Context.local_clustering"
    assert bspgemm.LCC_DIRECTED == 1
    assert C.sizeof(bspgemm.LccInfo) == 4 * 8
    assert [f for f, _ in bspgemm.LccInfo._fields_] == ["triangles", "entries", "heavy_entries", "reciprocal"]


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the vertices whose directed count is at least `least`, as a diagonal selector; *mean = the mean coefficient */
int clustered(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int least, bspgemm_matrix **D, double *mean)
{
    bspgemm_result *counts = 0;
    bspgemm_lcc_info info;
    int64_t sum = 0;
    int v;
    int *degree = malloc(((size_t)n + 1) * sizeof(int));
    double *lcc = malloc(((size_t)n + 1) * sizeof(double));
    *mean = 0;
    if (!degree || !lcc) return -1;
    if (bspgemm_local_clustering(ctx, A, BSPGEMM_LCC_DIRECTED, &counts, degree, lcc, &info) != BSPGEMM_OK) return -1;
    for (v = 0; v < n; v++) *mean += lcc[v] / n + 0 * degree[v];
    free(degree);
    free(lcc);
    if (bspgemm_result_values_sum(ctx, counts, &sum) != BSPGEMM_OK
        || bspgemm_matrix_from_result_where(ctx, counts, n, BSPGEMM_CMP_GE, least, D) != BSPGEMM_OK) {
        bspgemm_result_free(counts);
        return -1;
    }
    bspgemm_result_free(counts);
    if (bspgemm_local_clustering(ctx, A, 0, &counts, 0, 0, 0) != BSPGEMM_OK) return -1;
    bspgemm_result_free(counts);
    return (int)(sum + 0 * (info.triangles + info.entries + info.heavy_entries + info.reciprocal));
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_and_unknown_flags_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the bad argument is refused first
    sentinel, last = SENTINEL, last_error

    def dirty():
        return dirtied(bspgemm.LccInfo, 0x5A)

    zeroed = is_zeroed

    for ctx, A in ((None, fake), (fake, None)):
        out, info = C.c_void_p(sentinel), dirty()
        assert fn(ctx, A, 0, C.byref(out), None, None, C.byref(info)) == ERR_INVALID
        assert not out.value and NAME in last() and "NULL" in last(), last()
        assert zeroed(info)
    info = dirty()
    assert fn(fake, fake, 0, None, None, None, C.byref(info)) == ERR_INVALID
    assert NAME in last() and "NULL" in last() and zeroed(info), last()
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):                          # refused before the operand is looked at
        out, info = C.c_void_p(sentinel), dirty()
        assert fn(fake, fake, flags, C.byref(out), None, None, C.byref(info)) == ERR_INVALID
        assert not out.value and NAME in last() and "flag" in last() and zeroed(info), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def _small_random():
    """small random graphs of every kind the generators make, and the named small ones"""
    out = {}
    for i in range(12):
        rng = np.random.default_rng(5520 + i)
        kind = ("rmat", "uniform", "dups_unsorted", "untidy")[i % 4]
        if kind == "rmat":
            out["rmat_%d" % i] = gen.rmat(int(rng.integers(4, 8)), int(rng.integers(2, 8)), kcore_ref.SKEW, 5530 + i)
        elif kind == "uniform":
            out["uniform_%d" % i] = gen.uniform(int(rng.integers(5, 120)), int(rng.integers(1, 9)), 5530 + i)
        elif kind == "dups_unsorted":
            out["dups_%d" % i] = gen.dups_unsorted(int(rng.integers(20, 150)), int(rng.integers(1, 8)), 5530 + i)
        else:
            n = int(rng.integers(10, 100))
            out["untidy_%d" % i] = lcc_ref.untidy(n, 6 * n, 5530 + i)
    for name in ("empty0", "empty1", "self_loops5", "untidy150", "k70_oriented", "tile_plus_1", "rmat8"):
        out[name] = lcc_ref.GRAPHS[name]()
    return out


SMALL = _small_random()


def _lcc(pairs, n, directed=False):
    rp, ci, n = cc_ref.csr([p[0] for p in pairs], [p[1] for p in pairs], n)
    return lcc_ref.local_clustering(rp, ci, n, directed)


@pytest.mark.parametrize("name", list(SMALL))
def test_model_equals_the_naive_implementation(name):
    rp, ci, n = SMALL[name]
    und = None
    for directed in (False, True):
        num, d, lcc, triangles, reciprocal = lcc_ref.local_clustering(rp, ci, n, directed)
        e_num, e_d = lcc_ref.naive(rp, ci, n, directed)
        assert num.dtype == np.int32 and d.dtype == np.int32 and lcc.dtype == np.float64
        assert np.array_equal(num, e_num) and np.array_equal(d, e_d), (name, directed)
        exp = [0.0 if e_d[v] < 2 else float(e_num[v]) / (float(e_d[v]) * float(e_d[v] - 1)) for v in range(n)]
        assert lcc.tolist() == exp, (name, directed)                     # the bits: Python's floats are C doubles
        if not directed:
            und = num
            assert num.sum() == 6 * triangles and reciprocal == 0 and not (num % 2).any()
        else:
            assert (num <= und).all() and (2 * num >= und).all() and triangles == und.sum() // 6
        # the transpose: the same graph, and the directed count does not see the difference
        t_num, t_d, t_lcc, _, t_reciprocal = lcc_ref.local_clustering(*lcc_ref.transposed(rp, ci, n), directed)
        assert np.array_equal(t_num, num) and np.array_equal(t_d, d) and np.array_equal(t_lcc, lcc) and t_reciprocal == reciprocal
    # directed on a symmetric matrix equals undirected
    S = lcc_ref.graph(rp, ci, n)
    s_num, s_d, s_lcc, _, s_reciprocal = lcc_ref.local_clustering(S.indptr, S.indices, n, True)
    assert np.array_equal(s_num, und) and s_reciprocal == S.nnz // 2


def test_hand_examples_undirected():
    num, d, lcc, triangles, _ = _lcc([(0, 1), (1, 2), (2, 0)], 3)
    assert num.tolist() == [2, 2, 2] and d.tolist() == [2, 2, 2] and lcc.tolist() == [1.0, 1.0, 1.0] and triangles == 1
    num, d, lcc, triangles, _ = lcc_ref.local_clustering(*lcc_ref.complete(4))
    assert num.tolist() == [6] * 4 and d.tolist() == [3] * 4 and lcc.tolist() == [1.0] * 4 and triangles == 4
    num, d, lcc, triangles, _ = lcc_ref.local_clustering(*cc_ref.star(6, 0))
    assert not num.any() and d.tolist() == [5, 1, 1, 1, 1, 1] and not lcc.any() and triangles == 0
    num, d, lcc, triangles, _ = lcc_ref.local_clustering(*cc_ref.path(5))
    assert not num.any() and d.tolist() == [1, 2, 2, 2, 1] and not lcc.any() and triangles == 0
    # a triangle with a tail: vertex 2 has three neighbours, one joined pair among them (both orders)
    num, d, lcc, _, _ = _lcc([(0, 1), (1, 2), (2, 0), (2, 3)], 4)
    assert num.tolist() == [2, 2, 2, 0] and d.tolist() == [2, 2, 3, 1] and lcc.tolist() == [1.0, 1.0, 2.0 / 6.0, 0.0]


def test_hand_examples_directed():
    # a directed 3-cycle: each vertex sees one of the two ordered pairs of its neighbours
    cyc = [(0, 1), (1, 2), (2, 0)]
    num, d, lcc, triangles, reciprocal = _lcc(cyc, 3, True)
    assert num.tolist() == [1, 1, 1] and d.tolist() == [2, 2, 2] and lcc.tolist() == [0.5, 0.5, 0.5]
    assert (triangles, reciprocal) == (1, 0)
    # the same with the edge {0, 1} stored both ways: only the opposite corner, 2, gains
    num, d, lcc, triangles, reciprocal = _lcc(cyc + [(1, 0)], 3, True)
    assert num.tolist() == [1, 1, 2] and lcc.tolist() == [0.5, 0.5, 1.0] and (triangles, reciprocal) == (1, 1)
    # all three both ways: the undirected triangle
    num, _, lcc, _, reciprocal = _lcc(cyc + [(1, 0), (2, 1), (0, 2)], 3, True)
    assert num.tolist() == [2, 2, 2] and lcc.tolist() == [1.0, 1.0, 1.0] and reciprocal == 3
    # repeats count once, in the degree and in the count
    num, d, lcc, _, _ = _lcc(cyc + cyc + [(0, 1)], 3, True)
    assert num.tolist() == [1, 1, 1] and d.tolist() == [2, 2, 2]


def test_a_vertex_whose_only_neighbours_come_from_a_repeat_or_a_self_loop():
    # vertex 3: the entry (3, 0) three times and a self-loop -- one neighbour, d = 1, lcc 0; vertex 4: a self-loop alone
    pairs = [(0, 1), (1, 2), (2, 0), (3, 0), (3, 0), (3, 0), (3, 3), (4, 4)]
    for directed in (False, True):
        num, d, lcc, _, _ = _lcc(pairs, 5, directed)
        assert d.tolist() == [3, 2, 2, 1, 0] and num[3] == 0 and num[4] == 0 and lcc[3] == 0.0 and lcc[4] == 0.0
        assert lcc[0] == (1.0 if directed else 2.0) / 6.0


def test_the_graphs_ask_what_they_say():
    T, tile, deep = lcc_ref.LIGHT_DEFAULT, lcc_ref.K_SEL_TILE, lcc_ref.K_DEEP
    assert (tile, lcc_ref.K_SEL_STAGE, deep, T) == (4096, 4096, 4, 32)
    for name, entries in (("tile_minus_1", tile - 1), ("tile_exact", tile), ("tile_plus_1", tile + 1)):
        assert lcc_ref.half_entries(*lcc_ref.GRAPHS[name]()) == entries
    rp, ci, n = lcc_ref.GRAPHS["k258"]()
    S = lcc_ref.graph(rp, ci, n).tocoo()
    lower = np.bincount(S.row[S.col < S.row], minlength=n)                # the oriented rows: every length 0 .. 257
    for length in (T, T + 1, 63, 64, 65, 64 * deep - 1, 64 * deep, 64 * deep + 1):
        assert length in lower
    assert lcc_ref.heavy_entries(rp, ci, n, T) > 0 and lcc_ref.heavy_entries(rp, ci, n, 2**30) == 0
    assert lcc_ref.heavy_entries(*lcc_ref.GRAPHS["k70"](), T) == sum(i - (T + 1) for i in range(T + 2, 70))
    for name, hub in (("friendship_hub_first", 0), ("friendship_hub_last", 6000)):
        rp, ci, n = lcc_ref.GRAPHS[name]()
        num, d, lcc, triangles, _ = lcc_ref.local_clustering(rp, ci, n)
        assert n == 6001 and d[hub] == 6000 > tile and num[hub] == 6000 and triangles == 3000
        assert (np.delete(num, hub) == 2).all() and (np.delete(lcc, hub) == 1.0).all()
    num, d, _, _, _ = lcc_ref.local_clustering(*lcc_ref.GRAPHS["star5000"]())
    assert not num.any() and d[0] == 5000
    rp, ci, n = lcc_ref.GRAPHS["far_triangles"]()
    assert n > lcc_ref.K_SEL_STAGE + 3 and lcc_ref.half_entries(rp, ci, n) < tile
    assert lcc_ref.local_clustering(rp, ci, n)[3] == 3
    rp, ci, n = lcc_ref.GRAPHS["rmat11"]()
    und, dire = lcc_ref.local_clustering(rp, ci, n), lcc_ref.local_clustering(rp, ci, n, True)
    assert n == 2048 and und[3] > 1000 and not np.array_equal(und[0], dire[0]) and 0 < dire[4] < lcc_ref.half_entries(rp, ci, n)
    assert 0 < lcc_ref.heavy_entries(rp, ci, n, T) < lcc_ref.heavy_entries(rp, ci, n, 0) <= lcc_ref.half_entries(rp, ci, n)
