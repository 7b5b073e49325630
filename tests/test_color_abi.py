"""The device-resident graph colouring (bspgemm_graph_coloring) at the ABI level, without a GPU: the header declares the
enum and the function with the agreed argument list between bspgemm_strongly_connected_components and bspgemm_closure, the
library exports it, the Python view has it, a C99 caller compiles cleanly, NULL arguments are refused by name -- and the
tests' own reference (color_ref.py) equals networkx's greedy colouring driven with the same vertex order, has the four
properties of a greedy colouring on every graph, and breaks ties of the key by the vertex id.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import color_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, header_text, compile_c99, last_error

NAME = "bspgemm_graph_coloring"

ENUM = ("typedef enum bspgemm_color_order { BSPGEMM_COLOR_NATURAL = 1, BSPGEMM_COLOR_RANDOM = 2, "
        "BSPGEMM_COLOR_LARGEST_FIRST = 3 } bspgemm_color_order;")
DECLARATION = ("bspgemm_status bspgemm_graph_coloring(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_color_order order, "
               "unsigned seed, bspgemm_matrix **P, int *ncolors, int *rounds);")


def test_header_declares_it_between_scc_and_closure():
    code = header_code()
    assert ENUM in code, "include/bspgemm.h does not declare bspgemm_color_order as agreed"
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_strongly_connected_components(") < code.index(ENUM) < code.index(NAME + "(") \
        < code.index("bspgemm_closure(")
    comment = header_text().split(NAME + "(")[0].rsplit("/*", 1)[1]
    for word in ("0x7feb352d", "0x846ca68b", "0x7fffffff - deg_S(v)", "maximal independent set", "BSPGEMM_COLOR_TIMING"):
        assert word in header_text(), word
    assert "mix32" in comment and "lexicographically" in comment          # the formula is part of the contract


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 7
    assert callable(getattr(bspgemm.Context, "graph_coloring", None)), "Context.graph_coloring"


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the size of a maximal independent set of A's graph: class 0 of the colouring; *colors = how many classes there are */
int independent_set(bspgemm_context *ctx, const bspgemm_matrix *A, int n, unsigned seed, int *colors)
{
    bspgemm_matrix *P = 0, *classes = 0;
    bspgemm_color_order order = BSPGEMM_COLOR_LARGEST_FIRST;
    int rounds = 0, size = -1;
    int *row_ptr;
    if (bspgemm_graph_coloring(ctx, A, order, seed, &P, colors, &rounds) != BSPGEMM_OK) return -1;
    if (bspgemm_matrix_transpose(ctx, P, &classes) != BSPGEMM_OK) { bspgemm_matrix_free(P); return -1; }
    row_ptr = malloc(((size_t)n + 1) * sizeof(int));
    if (row_ptr && bspgemm_matrix_download(ctx, classes, row_ptr, 0) == BSPGEMM_OK) size = n ? row_ptr[1] - row_ptr[0] : 0;
    free(row_ptr);
    bspgemm_matrix_free(classes);
    bspgemm_matrix_free(P);
    if (bspgemm_graph_coloring(ctx, A, BSPGEMM_COLOR_NATURAL, 0u, &P, 0, 0) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(P);
    if (bspgemm_graph_coloring(ctx, A, BSPGEMM_COLOR_RANDOM, 7u, &P, 0, 0) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(P);
    return size + 0 * rounds;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    for ctx, A in ((None, fake), (fake, None)):
        out, colors, rounds = C.c_void_p(sentinel), C.c_int(7), C.c_int(7)
        assert fn(ctx, A, 2, 0, C.byref(out), C.byref(colors), C.byref(rounds)) == ERR_INVALID
        assert not out.value and NAME in last() and "NULL" in last(), last()
        assert (colors.value, rounds.value) == (0, 0)
    assert fn(fake, fake, 2, 0, None, None, None) == ERR_INVALID
    assert NAME in last() and "NULL" in last(), last()
    for order in (0, 4, -1):                                              # refused before the operand is looked at
        out = C.c_void_p(sentinel)
        assert fn(fake, fake, order, 0, C.byref(out), None, None) == ERR_INVALID
        assert not out.value and NAME in last() and "order" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def test_mix32_and_the_keys():
    # worked by hand from the formula: mix32(0) = 0; mix32 is a bijection of uint32 (xor-shifts and odd multipliers)
    assert int(color_ref.mix32(np.uint32(0))) == 0
    x = 1
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(color_ref.mix32(np.uint32(1))) == x
    h = color_ref.mix32(np.arange(1 << 16, dtype=np.uint32) ^ np.uint32(12345))
    assert h.dtype == np.uint32 and np.unique(h).size == h.size           # no ties among distinct vertices
    deg = np.array([3, 0, 3, 1])
    assert color_ref.keys(4, "natural", 99, deg).tolist() == [0, 1, 2, 3]
    lo = color_ref.mix32(np.arange(4, dtype=np.uint32) ^ np.uint32(99)).astype(np.uint64)
    assert np.array_equal(color_ref.keys(4, "random", 99, deg), lo)
    k = color_ref.keys(4, "largest", 99, deg)
    assert k.dtype == np.uint64 and np.array_equal(k >> np.uint64(32), 0x7fffffff - deg) and np.array_equal(k & np.uint64(0xFFFFFFFF), lo)
    order = color_ref.visit_order(k).tolist()
    assert set(order[:2]) == {0, 2} and order[2:] == [3, 1]               # larger degrees first


def test_key_ties_are_broken_by_the_vertex_id(monkeypatch):
    """mix32 has no ties among distinct vertices (above), so one is forced: with a constant hash every key is equal under
    RANDOM and the order is the ids'; under LARGEST_FIRST equal degrees fall back to the ids"""
    assert color_ref.visit_order(np.array([5, 3, 5, 3, 3], np.uint64)).tolist() == [1, 3, 4, 0, 2]
    assert color_ref.rank_of(np.array([5, 3, 5, 3, 3], np.uint64)).tolist() == [3, 0, 4, 1, 2]
    rp, ci, n = color_ref.GRAPHS["rmat10"]()
    natural = color_ref.coloring(rp, ci, n, "natural")
    monkeypatch.setattr(color_ref, "mix32", lambda x: np.full(np.asarray(x).shape, 77, np.uint32))
    tied = color_ref.coloring(rp, ci, n, "random", 5)
    assert np.array_equal(tied[0], natural[0]) and tied[1:] == natural[1:]
    srp, sci = color_ref.simple(rp, ci, n)
    deg = np.diff(srp)
    largest = color_ref.coloring(rp, ci, n, "largest", 5)[0]
    assert np.array_equal(largest, color_ref.first_fit(srp, sci, n, np.lexsort((np.arange(n), -deg))))


@functools.lru_cache(maxsize=None)
def _graph(name):
    rp, ci, n = color_ref.GRAPHS[name]()
    return (rp, ci, n) + color_ref.simple(rp, ci, n)


@pytest.mark.parametrize("name", color_ref.SMALL)
def test_model_equals_networkx_and_has_the_properties(name):
    import networkx as nx
    rp, ci, n, srp, sci = _graph(name)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(np.repeat(np.arange(n), np.diff(srp)).tolist(), sci.tolist()))
    for order in color_ref.ORDERS:
        key = color_ref.keys(n, order, 11, np.diff(srp))
        colour, ncolors, rounds = color_ref.coloring(rp, ci, n, order, 11)
        assert colour.dtype == np.int32 and colour.shape == (n,)
        visit = color_ref.visit_order(key).tolist()
        theirs = nx.greedy_color(G, strategy=lambda g, c: visit)
        assert colour.tolist() == [theirs[v] for v in range(n)], (name, order)
        assert np.array_equal(colour, color_ref.first_fit(srp, sci, n, visit))
        color_ref.check_properties(srp, sci, n, colour, key)
        assert ncolors == (int(colour.max()) + 1 if n else 0)
        # rounds: the vertices on the longest chain of ascending (key, id) along edges
        depth = np.zeros(n, np.int64)
        rank = color_ref.rank_of(key)
        for v in visit:
            nb = sci[srp[v]:srp[v + 1]]
            nb = nb[rank[nb] < rank[v]]
            depth[v] = 1 + (depth[nb].max() if nb.size else 0)
        assert rounds == (int(depth.max()) if sci.size else 0), (name, order)
        if sci.size == 0:
            assert not colour.any() and (ncolors, rounds) == (min(n, 1), 0)


def test_model_on_a_hand_example():
    # a path 0 - 1 - 2 - 3 and a triangle 4 5 6 with a self-loop, a repeat and one-direction storage; 7 alone
    rp = np.array([0, 1, 2, 3, 3, 6, 8, 8, 8], np.int32)
    ci = np.array([1, 2, 3, 5, 6, 4, 6, 6], np.int32)
    colour, ncolors, rounds = color_ref.coloring(rp, ci, 8, "natural")
    assert colour.tolist() == [0, 1, 0, 1, 0, 1, 2, 0] and (ncolors, rounds) == (3, 4)
    t_rp, t_ci = np.array([0, 0, 1, 2, 3, 4, 5, 8, 8], np.int32), np.array([0, 1, 2, 4, 4, 4, 5, 5], np.int32)   # in-edges
    assert np.array_equal(color_ref.coloring(t_rp, t_ci, 8, "natural")[0], colour)


def test_window_graphs_have_the_colours_they_promise():
    """the model on the graphs with more colours than one bitmap window: about a second each"""
    W, K = color_ref.WINDOW, color_ref.CLIQUE
    rp, ci, n = color_ref.WINDOW_GRAPHS["cliques2048_2060"]()
    colour, ncolors, rounds = color_ref.coloring(rp, ci, n, "natural")
    assert (ncolors, rounds) == (K, K) and np.array_equal(colour, np.concatenate([np.arange(W), np.arange(K)]))
    rp, ci, n = color_ref.WINDOW_GRAPHS["window_above"]()
    colour, ncolors, rounds = color_ref.coloring(rp, ci, n, "natural")
    assert np.array_equal(colour[:K], np.arange(K)) and colour[K] == 10 and (ncolors, rounds) == (K, K + 1)
    rp, ci, n = color_ref.WINDOW_GRAPHS["window_below"]()
    colour, ncolors, rounds = color_ref.coloring(rp, ci, n, "natural")
    assert np.array_equal(colour[:K], np.arange(K)) and colour[K:].tolist() == [10, W, 0] and (ncolors, rounds) == (K, K + 1)
