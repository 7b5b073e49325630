"""The device-resident maximal matching (bspgemm_maximal_matching) at the ABI level, without a GPU: the header declares the
enum, the info struct and the function with the agreed argument list between bspgemm_betweenness and bspgemm_closure, the
option has its number, the library exports it, the Python view has it, a C99 caller compiles cleanly, NULL arguments and
unknown orders are refused by name -- and the tests' own reference (match_ref.py): its round model equals plain sequential
greedy over the sorted edges and is a maximal matching (by its own check and by networkx's) on every graph and order,
gives the mates written out by hand on a small example, breaks ties of the key by the edge's ends, and takes the rounds
the graphs are built for.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import match_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, header_text, compile_c99, last_error, dirtied

NAME = "bspgemm_maximal_matching"

ENUM = ("typedef enum bspgemm_match_order { BSPGEMM_MATCH_NATURAL = 1, BSPGEMM_MATCH_RANDOM = 2, "
        "BSPGEMM_MATCH_LIGHT_FIRST = 3 } bspgemm_match_order;")
STRUCT = ("typedef struct bspgemm_match_info { int64_t pairs; int64_t entries_walked; int64_t hub_chunks; int rounds; "
          "int lanes; } bspgemm_match_info;")
DECLARATION = ("bspgemm_status bspgemm_maximal_matching(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_match_order order, "
               "unsigned seed, bspgemm_matrix **P, int *mate_host, bspgemm_match_info *info);")


def test_header_declares_it_between_betweenness_and_closure():
    code = header_code()
    assert ENUM in code, "include/bspgemm.h does not declare bspgemm_match_order as agreed"
    assert STRUCT in code, "include/bspgemm.h does not declare bspgemm_match_info as agreed"
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_betweenness(") < code.index(ENUM) < code.index(STRUCT) < code.index(NAME + "(") \
        < code.index("bspgemm_closure(")
    assert "BSPGEMM_OPT_MATCH_LANES = 15" in code
    text = header_text()
    comment = text.split(NAME + "(")[0].rsplit("/*", 6)[1]               # (the struct's five field comments follow it)
    for word in ("0x7feb352d", "0x846ca68b", "0xffff", "lexicographically", "mix32", "(key32, a, b)", "min(v, mate(v))",
                 "BSPGEMM_OPT_MATCH_LANES", "BSPGEMM_MATCH_TIMING", "statistics", "walked AGAIN"):
        assert word in comment, word
    assert "MATCH_LANES" in text.split("typedef enum bspgemm_option")[0]
    assert "BSPGEMM_MATCH_TIMING" in text.split("typedef struct bspgemm_context")[0]


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 7
    assert callable(getattr(bspgemm.Context, "maximal_matching", None)), "Context.maximal_matching"
    assert bspgemm.OPTIONS["match_lanes"] == 15
    assert bspgemm.Context.MATCH_ORDERS == {"natural": 1, "random": 2, "light": 3}
    assert [f for f, _ in bspgemm.MatchInfo._fields_] == ["pairs", "entries_walked", "hub_chunks", "rounds", "lanes"]
    assert C.sizeof(bspgemm.MatchInfo) == 32


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* one level of coarsening: the contracted graph P^T * A * P of a matching of A's graph; *pairs = the edges contracted */
bspgemm_result *coarsen(bspgemm_context *ctx, const bspgemm_matrix *A, int n, unsigned seed, long long *pairs)
{
    bspgemm_matrix *P = 0, *PT = 0, *M = 0;
    bspgemm_result *R = 0, *Q = 0;
    bspgemm_match_order order = BSPGEMM_MATCH_LIGHT_FIRST;
    bspgemm_match_info info;
    int *mate = malloc(((size_t)n + 1) * sizeof(int));
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_MATCH_LANES, 16) != BSPGEMM_OK) return 0;
    if (!mate || bspgemm_maximal_matching(ctx, A, order, seed, &P, mate, &info) != BSPGEMM_OK) { free(mate); return 0; }
    *pairs = (long long)info.pairs + 0 * (info.entries_walked + info.hub_chunks + info.rounds + info.lanes);
    free(mate);
    if (bspgemm_matrix_transpose(ctx, P, &PT) == BSPGEMM_OK && bspgemm_multiply(ctx, PT, A, 0, n, &R) == BSPGEMM_OK &&
        bspgemm_matrix_from_result(ctx, R, n, &M) == BSPGEMM_OK)
        (void)bspgemm_multiply(ctx, M, P, 0, n, &Q);
    bspgemm_matrix_free(M);
    bspgemm_result_free(R);
    bspgemm_matrix_free(PT);
    bspgemm_matrix_free(P);
    if (bspgemm_maximal_matching(ctx, A, BSPGEMM_MATCH_NATURAL, 0u, &P, 0, 0) != BSPGEMM_OK) return Q;
    bspgemm_matrix_free(P);
    if (bspgemm_maximal_matching(ctx, A, BSPGEMM_MATCH_RANDOM, 7u, &P, 0, 0) != BSPGEMM_OK) return Q;
    bspgemm_matrix_free(P);
    return Q;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_and_unknown_orders_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    def info7():
        return dirtied(bspgemm.MatchInfo, 7)

    for ctx, A in ((None, fake), (fake, None)):
        out, info = C.c_void_p(sentinel), info7()
        assert fn(ctx, A, 2, 0, C.byref(out), None, C.byref(info)) == ERR_INVALID
        assert not out.value and NAME in last() and "NULL" in last(), last()
        assert not any(info.as_dict().values()), info.as_dict()
    info = info7()
    assert fn(fake, fake, 2, 0, None, None, C.byref(info)) == ERR_INVALID
    assert NAME in last() and "NULL" in last(), last()
    assert not any(info.as_dict().values()), info.as_dict()
    for order in (0, 4, -1):                                              # refused before the operand is looked at
        out, info = C.c_void_p(sentinel), info7()
        assert fn(fake, fake, order, 0, C.byref(out), None, C.byref(info)) == ERR_INVALID
        assert not out.value and NAME in last() and "order" in last(), last()
        assert not any(info.as_dict().values()), info.as_dict()


# ---------------------------------------------------------------- the reference itself -------------------------------
def test_the_edge_keys():
    a, b, deg = np.array([0, 0, 2, 5]), np.array([1, 7, 3, 6]), np.array([2, 1, 1, 1, 0, 70000, 3, 1])
    assert match_ref.edge_keys(a, b, "natural", 99, deg).tolist() == [0, 0, 0, 0]
    h = match_ref.edge_keys(a, b, "random", 99, deg)
    expect = [int(match_ref.mix32(np.uint32(int(match_ref.mix32(np.uint32(x ^ 99))) ^ y))) for x, y in zip(a.tolist(), b.tolist())]
    assert h.dtype == np.uint32 and h.tolist() == expect
    assert not np.array_equal(h, match_ref.edge_keys(a, b, "random", 100, deg))
    light = match_ref.edge_keys(a, b, "light", 99, deg)
    assert light.dtype == np.uint32
    assert (light >> 16).tolist() == [3, 3, 2, 0xffff] and np.array_equal(light & 0xffff, h >> 16)   # 70003 saturates
    # a pair is one edge however it is met: the smaller end goes into the inner hash
    big = np.arange(1 << 12)
    k = match_ref.edge_keys(np.zeros(big.size - 1, np.int64), big[1:], "random", 5, None)
    assert np.unique(k).size == k.size


@functools.lru_cache(maxsize=None)
def _graph(name):
    rp, ci, n = (match_ref.GRAPHS.get(name) or match_ref.GROUP_GRAPHS.get(name) or match_ref.HUB_GRAPHS[name])()
    return (rp, ci, n) + match_ref.simple(rp, ci, n)


ALL_GRAPHS = list(match_ref.SMALL) + [g for g in match_ref.GROUP_GRAPHS if g not in match_ref.SMALL] + list(match_ref.HUB_GRAPHS)


@pytest.mark.parametrize("name", ALL_GRAPHS)
def test_model_equals_greedy_and_is_a_maximal_matching(name):
    import networkx as nx
    rp, ci, n, srp, sci = _graph(name)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(np.repeat(np.arange(n), np.diff(srp)).tolist(), sci.tolist()))
    deg = np.diff(srp)
    for order in match_ref.ORDERS:
        r = match_ref.matching(rp, ci, n, order, 11)
        assert r.mate.dtype == np.int32 and r.mate.shape == (n,) and r.labels.dtype == np.int32
        assert np.array_equal(r.mate, match_ref.greedy(srp, sci, n, order, 11)), (name, order)
        match_ref.check_properties(srp, sci, n, r.mate)
        pairs = {(v, int(r.mate[v])) for v in range(n) if r.mate[v] > v}
        assert len(pairs) == r.pairs and nx.is_maximal_matching(G, pairs), (name, order)
        v = np.arange(n)
        assert np.array_equal(r.labels, np.where(r.mate >= 0, np.minimum(v, r.mate), v))
        assert np.bincount(r.labels, minlength=n).max(initial=0) <= 2
        # the chunk size and the lanes change the counts they are about and nothing else
        small = match_ref.matching(rp, ci, n, order, 11, chunk=3, lanes=64)
        assert np.array_equal(small.mate, r.mate) and small[2:5] == r[2:5] and small.hub_chunks >= r.hub_chunks
        assert small.lanes == (64 if sci.size else 0)
        assert r.entries_walked >= sci.size and (r.rounds > 0) == (sci.size > 0) and r.rounds <= n // 2 + 1
        assert r.lanes == match_ref.lanes_for(sci.size, int((deg > 0).sum()))
        if sci.size == 0:
            assert (r.mate == -1).all() and np.array_equal(r.labels, v) and r[2:] == (0, 0, 0, 0, 0)


def test_model_on_a_hand_example():
    # a path 0 - 1 - 2 - 3 and a triangle 4 5 6 with a self-loop, a repeat and one-direction storage; 7 alone
    rp = np.array([0, 1, 2, 3, 3, 6, 8, 8, 8], np.int32)
    ci = np.array([1, 2, 3, 5, 6, 4, 6, 6], np.int32)
    # NATURAL: the edges in the order (0,1) (1,2) (2,3) (4,5) (4,6) (5,6): greedy takes (0,1), (2,3) and (4,5).  Round 1: 0 and
    # 1, 4 and 5 point at each other; 2 points at 1, 3 at 2, 6 at 4.  Round 2: 2 and 3 point at each other, 6 retires
    r = match_ref.matching(rp, ci, 8, "natural")
    assert r.mate.tolist() == [1, 0, 3, 2, 5, 4, -1, -1] and r.labels.tolist() == [0, 0, 2, 2, 4, 4, 6, 7]
    assert (r.pairs, r.rounds, r.entries_walked, r.hub_chunks, r.lanes) == (3, 2, 12 + 5, 0, 4)
    t_rp, t_ci = np.array([0, 0, 1, 2, 3, 4, 5, 8, 8], np.int32), np.array([0, 1, 2, 4, 4, 4, 5, 5], np.int32)   # in-edges
    t = match_ref.matching(t_rp, t_ci, 8, "natural")
    assert np.array_equal(t.mate, r.mate) and t[2:] == r[2:]
    # with chunks of one entry every row of two entries is a hub of two chunks: 5 such rows in round 1, 2 in round 2
    assert match_ref.matching(rp, ci, 8, "natural", chunk=1).hub_chunks == 2 * 5 + 2 * 2


def test_key_ties_are_broken_by_the_ends(monkeypatch):
    """mix32 gives few ties, so they are forced: with a constant hash every key is equal under RANDOM and the order is
    that of (a, b), which is NATURAL; under LIGHT_FIRST equal degree sums fall back to (a, b)"""
    rp, ci, n = match_ref.GRAPHS["rmat10"]()
    natural = match_ref.matching(rp, ci, n, "natural")
    distinct = match_ref.matching(rp, ci, n, "random", 5)
    assert not np.array_equal(distinct.mate, natural.mate)
    monkeypatch.setattr(match_ref, "mix32", lambda x: np.full(np.asarray(x).shape, 77, np.uint32))
    tied = match_ref.matching(rp, ci, n, "random", 5)
    assert np.array_equal(tied.mate, natural.mate) and tied[2:] == natural[2:]
    srp, sci = match_ref.simple(rp, ci, n)
    a, b = match_ref.edges_of(srp, sci, n)
    deg = np.diff(srp)
    light = match_ref.matching(rp, ci, n, "light", 5)
    mate = np.full(n, -1, np.int32)
    for i in np.lexsort((b, a, np.minimum(deg[a] + deg[b], 0xffff))).tolist():
        if mate[a[i]] < 0 and mate[b[i]] < 0:
            mate[a[i]], mate[b[i]] = b[i], a[i]
    assert np.array_equal(light.mate, mate)


def test_the_graphs_take_the_rounds_they_are_built_for():
    def rounds(name, order):
        rp, ci, n, _, _ = _graph(name)
        return match_ref.matching(rp, ci, n, order, 11).rounds

    assert rounds("path200", "natural") == 100                         # one pair per round, from the low end
    assert rounds("chains4099", "natural") == 684
    for star in ("star_hub_last", "star_hub_middle", "star_leaf_rows"):
        assert [rounds(star, order) for order in match_ref.ORDERS] == [2, 2, 2]   # the hub's pair, then 4999 retirements
    assert max(rounds(name, "random") for name in match_ref.SMALL) <= 8
    # the hub stays live for three rounds: two chunk records in each
    rp, ci, n, _, _ = _graph("hub_live3")
    r = match_ref.matching(rp, ci, n, "natural")
    assert (r.rounds, r.hub_chunks, r.pairs) == (3, 6, 2 * (match_ref.CHUNK + 1)) and r.mate[n - 1] == -1
