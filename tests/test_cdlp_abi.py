"""The device-resident label propagation (bspgemm_label_propagation) at the ABI level, without a GPU: the header declares
the info struct and the function with the agreed argument list between bspgemm_graph_coloring and bspgemm_closure, the
library exports it, the Python view has it, a C99 caller compiles cleanly, NULL arguments and a negative max_iter are
refused by name before anything is dereferenced -- and the tests' own reference (cdlp_ref.py) equals a naive Counter-per-
vertex implementation on every small graph, reproduces the examples worked by hand, and gives the figures recorded for the
named graphs.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import cc_ref
import cdlp_ref
import kcore_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, header_text, compile_c99, last_error, dirtied, is_zeroed

NAME = "bspgemm_label_propagation"

STRUCT = ("typedef struct bspgemm_lp_info { int iterations; int converged; int communities; int changed; "
          "int64_t class_vertices[4]; } bspgemm_lp_info;")
DECLARATION = ("bspgemm_status bspgemm_label_propagation(bspgemm_context *ctx, const bspgemm_matrix *A, const int *initial_labels, "
               "int max_iter, bspgemm_matrix **P, bspgemm_lp_info *info);")


def test_header_declares_it_between_coloring_and_closure():
    code = header_code()
    assert STRUCT in code, "include/bspgemm.h does not declare bspgemm_lp_info as agreed"
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_graph_coloring(") < code.index(STRUCT) < code.index(NAME + "(") < code.index("bspgemm_closure(")
    assert "BSPGEMM_OPT_LP_MIN_CLASS = 11" in code
    comment = header_text().split("typedef struct bspgemm_lp_info")[0].rsplit("/*", 1)[1]
    # the definition is part of the contract, and so is the warning about the oscillation
    for word in ("synchronously", "smallest label among those that occur most often", "OSCILLATES with period 2", "bipartite",
                 "fixpoint", "BSPGEMM_SYMMETRIZE_DROP_DIAGONAL", "BSPGEMM_OPT_LP_MIN_CLASS", "BSPGEMM_LP_TIMING", "max_iter == 0"):
        assert word in comment, word


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 6
    assert callable(getattr(bspgemm.Context, "label_propagation", None)), "Context.label_propagation"
    assert bspgemm.OPTIONS["lp_min_class"] == 11
    assert C.sizeof(bspgemm.LpInfo) == 4 * 4 + 4 * 8
    assert [f for f, _ in bspgemm.LpInfo._fields_] == ["iterations", "converged", "communities", "changed", "class_vertices"]


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the size of the community of vertex 0 after at most k iterations from a warm start; *communities = how many there are */
int community_of_zero(bspgemm_context *ctx, const bspgemm_matrix *A, int n, const int *warm, int k, int *communities)
{
    bspgemm_matrix *P = 0, *members = 0;
    bspgemm_lp_info info;
    int size = -1;
    int *row_ptr, *label;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_LP_MIN_CLASS, 1) != BSPGEMM_OK) return -1;
    if (bspgemm_label_propagation(ctx, A, warm, k, &P, &info) != BSPGEMM_OK) return -1;
    *communities = info.communities + 0 * (info.iterations + info.converged + info.changed + (int)info.class_vertices[3]);
    if (bspgemm_matrix_transpose(ctx, P, &members) != BSPGEMM_OK) { bspgemm_matrix_free(P); return -1; }
    row_ptr = malloc(((size_t)n + 1) * sizeof(int));
    label = malloc(((size_t)n + 1) * sizeof(int));
    if (row_ptr && label && bspgemm_matrix_download(ctx, P, 0, label) == BSPGEMM_OK
        && bspgemm_matrix_download(ctx, members, row_ptr, 0) == BSPGEMM_OK)
        size = n ? row_ptr[label[0] + 1] - row_ptr[label[0]] : 0;
    free(row_ptr);
    free(label);
    bspgemm_matrix_free(members);
    bspgemm_matrix_free(P);
    if (bspgemm_label_propagation(ctx, A, 0, 10, &P, 0) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(P);
    return size;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_and_a_negative_cap_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the bad argument is refused first
    sentinel, last = SENTINEL, last_error

    def dirty():
        return dirtied(bspgemm.LpInfo, 0x5A)

    zeroed = is_zeroed

    for ctx, A in ((None, fake), (fake, None)):
        out, info = C.c_void_p(sentinel), dirty()
        assert fn(ctx, A, None, 3, C.byref(out), C.byref(info)) == ERR_INVALID
        assert not out.value and NAME in last() and "NULL" in last(), last()
        assert zeroed(info)
    info = dirty()
    assert fn(fake, fake, None, 3, None, C.byref(info)) == ERR_INVALID
    assert NAME in last() and "NULL" in last() and zeroed(info), last()
    for cap in (-1, -2**31):                                              # refused before the operand is looked at
        out, info = C.c_void_p(sentinel), dirty()
        assert fn(fake, fake, None, cap, C.byref(out), C.byref(info)) == ERR_INVALID
        assert not out.value and NAME in last() and "max_iter" in last() and zeroed(info), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
SMALL = [name for name in cdlp_ref.GRAPHS if cdlp_ref.GRAPHS[name]()[2] <= 1100]


def test_the_small_graphs_are_the_ones_meant():
    assert {"path200", "cycle200", "spider63", "spider65", "spider257", "cliques64_66", "cliques2_40", "clique70_tail130", "rmat10",
            "untidy300", "chains257", "chains1023", "empty0", "empty1", "empty4", "empty1000", "self_loop"} <= set(SMALL)


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_the_naive_implementation(name):
    rp, ci, n = cdlp_ref.GRAPHS[name]()
    rng = np.random.default_rng(5461)
    for max_iter, initial in ((0, None), (1, None), (2, None), (3, None), (4, rng.integers(0, max(n, 1), size=n))):
        got = cdlp_ref.label_propagation(rp, ci, n, max_iter, initial)
        exp = cdlp_ref.naive(rp, ci, n, max_iter, initial)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], exp[0]), (name, max_iter)
        assert got[1:] == exp[1:], (name, max_iter, got[1:], exp[1:])
        if np.diff(kcore_ref.simple(rp, ci, n)[0]).sum() == 0:          # no edges: the first labels, no iteration, converged
            first = np.arange(n) if initial is None else initial
            assert np.array_equal(got[0], first) and got[1:4] == (0, 1, 0), (name, got[1:])


def test_a_path_of_four_is_synchronous_and_oscillates():
    # worked on paper.  An asynchronous sweep in id order would give L1 = [1, 0, 0, 0]: vertex 1 would see the new label of 0
    rp, ci, n = cc_ref.path(4)
    Ls, changed, converged = cdlp_ref.trajectory(rp, ci, n, 6)
    assert [L.tolist() for L in Ls[:4]] == [[0, 1, 2, 3], [1, 0, 1, 2], [0, 1, 0, 1], [1, 0, 1, 0]]
    assert [L.tolist() for L in Ls[4:]] == [[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1]] and not converged    # period 2
    assert changed == [4, 4, 4, 4, 4, 4]
    assert cdlp_ref.label_propagation(rp, ci, n, 3)[0].tolist() == [1, 0, 1, 0]
    assert cdlp_ref.label_propagation(rp, ci, n, 4)[1:] == (4, 0, 4, 2)


def test_a_triangle_converges_at_the_third_iteration():
    rp, ci, n = kcore_ref.cliques([3])
    Ls, changed, converged = cdlp_ref.trajectory(rp, ci, n, 10)
    assert [L.tolist() for L in Ls] == [[0, 1, 2], [1, 0, 0], [0, 0, 0], [0, 0, 0]] and changed == [3, 1, 0] and converged
    assert cdlp_ref.label_propagation(rp, ci, n, 10)[1:] == (3, 1, 0, 1)
    assert cdlp_ref.label_propagation(rp, ci, n, 2)[1:] == (2, 0, 1, 1)      # the fixpoint is there, but nobody has seen it


def test_two_cliques_joined_by_an_edge_stay_two_communities():
    rp, ci, n = kcore_ref.cliques([5, 5])
    rows = np.repeat(np.arange(n), np.diff(rp))
    rp, ci, n = cc_ref.csr(np.append(rows, 4), np.append(ci, 5), n)
    labels, iterations, converged, changed, communities = cdlp_ref.label_propagation(rp, ci, n, 10)
    assert labels.tolist() == [0] * 5 + [5] * 5 and (iterations, converged, changed, communities) == (3, 1, 0, 2)


def test_the_recorded_figures_of_the_named_graphs():
    def run(name, max_iter=10):
        rp, ci, n = cdlp_ref.GRAPHS[name]()
        return n, cdlp_ref.trajectory(rp, ci, n, max_iter), cdlp_ref.label_propagation(rp, ci, n, max_iter)

    _, (_, changed, converged), (_, iterations, _, _, communities) = run("cliques64_66")
    assert (iterations, converged, communities) == (3, True, 3) and changed == [195, 3, 0]
    _, (_, changed, converged), (_, iterations, _, _, communities) = run("uniform4096_d8")
    assert (iterations, converged, communities) == (8, True, 1)
    assert changed == [4096, 4090, 4001, 3619, 2463, 751, 29, 0]
    _, (_, changed, converged), _ = run("rmat10", 12)
    assert changed == [769, 481, 49, 5] + [4] * 8 and not converged
    # every star, spider, path and chain is bipartite and connected through every vertex: all labels move, for ever
    for name in cdlp_ref.GRAPHS:
        if name.startswith(("star", "spider", "path", "chains")):
            n, (_, changed, converged), _ = run(name, 5)
            assert changed == [n] * 5 and not converged, name


# ---------------------------------------------------------------- the classes and the star union ---------------------
def test_class_caps_and_boundaries():
    assert cdlp_ref.CAPS == (8, 256, 4096)
    assert [cdlp_ref.class_of(d) for d in (1, 8, 9, 256, 257, 4096, 4097, 10**6)] == [0, 0, 1, 1, 2, 2, 3, 3]
    for d in (1, 2, 63, 64, 65, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097):
        assert d in cdlp_ref.DEGREES
    rp, ci, n = cc_ref.star(10, 0)
    assert cdlp_ref.class_vertices(rp, ci, n) == [9, 1, 0, 0] and cdlp_ref.class_vertices(rp, ci, n, 2) == [0, 0, 10, 0]
    rp, ci, n = kcore_ref.GRAPHS["empty4"]()
    assert cdlp_ref.class_vertices(rp, ci, n, 3) == [0, 0, 0, 0]           # isolated vertices are in no class


def test_the_star_union_asks_what_it_says():
    rp, ci, n, initial, hubs, expected = cdlp_ref.star_union()
    stars = len(cdlp_ref.MULTISETS) * len(cdlp_ref.DEGREES)
    assert hubs.size == stars and n == sum(d + 1 for d in cdlp_ref.DEGREES) * len(cdlp_ref.MULTISETS)
    assert cdlp_ref.class_vertices(rp, ci, n) == [n - stars + 4 * 8, 6 * 8, 3 * 8, 8]   # lane: the leaves and the hubs of degree 1, 2, 7, 8
    labels, iterations, converged, changed, _ = cdlp_ref.label_propagation(rp, ci, n, 1, initial)
    assert np.array_equal(labels[hubs], expected) and (iterations, converged) == (1, 0)
    at = i = 0
    for kind in cdlp_ref.MULTISETS:
        for d in cdlp_ref.DEGREES:
            got = np.sort(initial[at + 1:at + 1 + d])
            assert hubs[i] == at and np.array_equal(got, np.sort(cdlp_ref.multiset(kind, d, n))) and cdlp_ref.mode(got) == expected[i]
            at, i = at + d + 1, i + 1
    d = 4097
    # what each multiset is for
    assert np.unique(cdlp_ref.multiset("distinct", d, n)).size == d and np.unique(cdlp_ref.multiset("equal", d, n)).size == 1
    h = cdlp_ref.multiset("halves", 64, n)
    assert np.bincount(h)[[3, 9]].tolist() == [32, 32] and cdlp_ref.mode(h) == 3
    a = cdlp_ref.multiset("ahead_by_one", 65, n)
    assert np.bincount(a)[[2, 11]].tolist() == [32, 33] and cdlp_ref.mode(a) == 11
    p = cdlp_ref.multiset("pairs_and_a_triple", 257, n)
    assert cdlp_ref.mode(p) == n - 1 and sorted(np.bincount(p)[np.bincount(p) > 0].tolist())[-2:] == [2, 3]
    assert cdlp_ref.mode(cdlp_ref.multiset("zero_wins", d, n)) == 0 and cdlp_ref.mode(cdlp_ref.multiset("zero_loses", d, n)) == 6
    for d in (64, 257, 4097):
        c = cdlp_ref.multiset("colliding", d, n)
        same = np.unique(c[:4])
        assert same.size == 4 and np.unique(cdlp_ref.hub_start(same, d)).size == 1, d
    # the padded variant: the large ids, and first labels of their own on the isolated vertices
    rp, ci, n, initial, hubs, expected = cdlp_ref.star_union(200_000, high=True)
    assert n == 200_000 and initial.max() == n - 1 and expected.max() > n - 100
