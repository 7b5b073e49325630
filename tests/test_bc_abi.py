"""The device-resident betweenness centrality (bspgemm_betweenness) at the ABI level, without a GPU: the header declares the
info struct, the function and the option as agreed, between bspgemm_pagerank and bspgemm_closure, and carries the definition;
the library exports it, the Python view has it, a C99 caller compiles cleanly, bad arguments are refused by name before
anything is dereferenced -- and the tests' own reference (bc_ref.py) equals a naive model in Python integers, reproduces the
examples worked by hand, and stays within the derived bound of networkx's float64 Brandes.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
import bc_ref as B
from abi_kit import ERR_INVALID, FAKE, header_code, header_text, compile_c99, last_error, dirtied

NAME = "bspgemm_betweenness"

STRUCT = ("typedef struct bspgemm_bc_info { uint64_t sigma_max; int64_t reached; int64_t edges_forward; int64_t hub_chunks; "
          "int sources; int depth_max; int levels; int canonicalised; } bspgemm_bc_info;")
DECLARATION = ("bspgemm_status bspgemm_betweenness(bspgemm_context *ctx, const bspgemm_matrix *A, int nsources, "
               "const int *sources, uint64_t *bc_fixed_host, double *bc_host, bspgemm_bc_info *info);")


def test_header_declares_it_between_pagerank_and_closure():
    code = header_code()
    assert STRUCT in code, "include/bspgemm.h does not declare bspgemm_bc_info as agreed"
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_pagerank(") < code.index(STRUCT) < code.index(NAME + "(") < code.index("bspgemm_closure(")
    assert "BSPGEMM_OPT_BC_LANES = 13" in code
    text = header_text()
    comment = text.split("typedef struct bspgemm_bc_info")[0].rsplit("/*", 1)[1]
    # the definition is the contract
    for word in ("ONE = 2^32", "level(s) = 0, sigma(s) = 1", "BFS distance", "level(u) == level(v) - 1", "sigma(v) >= 2^63",
                 "BSPGEMM_ERR_OVERFLOW", "the index of the source", "bit 63", "(double)(ONE + delta(w)) / (double) sigma(w)",
                 "(uint64) floor( c(w) * (double) sigma(v) )", "round to nearest even", "nothing that could fuse",
                 "np.floor", "last level have delta = 0", "bc(v) += delta_s(v) for every reached v != s", "repeats count once",
                 "never lie on a shortest path", "named twice counts twice", "(1 + 2^-51)", "n * ONE * (1 + 2^-40)",
                 "nsources * n >= 2^31", "ldexp((double) bc(v), -32)", "bc.astype(np.float64) * 2.0**-32", "endpoints are excluded",
                 "TWICE the undirected betweenness", "no normalisation flag", "m_s * 2^-32 + depth * 2^-50 * exact",
                 "networkx 3.4.2", "canonicalised = 1", "BSPGEMM_OPT_BC_LANES", "BSPGEMM_BC_TIMING", "statistics",
                 "Nothing is leaked", "No kernel waits for another workgroup", "one read-back per level",
                 "nsources == 0, n == 0 and nnz == 0 are valid"):
        assert word in comment, word
    assert "BC_LANES" in text.split("typedef enum bspgemm_option")[0] and "BSPGEMM_BC_TIMING" in text.split("typedef struct bspgemm_context")[0]


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 7
    assert callable(getattr(bspgemm.Context, "betweenness", None)), "Context.betweenness"
    assert bspgemm.OPTIONS["bc_lanes"] == 13
    assert C.sizeof(bspgemm.BcInfo) == 4 * 8 + 4 * 4
    assert [f for f, _ in bspgemm.BcInfo._fields_] == ["sigma_max", "reached", "edges_forward", "hub_chunks", "sources",
                                                       "depth_max", "levels", "canonicalised"]
    assert [getattr(bspgemm.BcInfo, f).offset for f, _ in bspgemm.BcInfo._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the vertex of the highest centrality from the first k vertices as sources, or -1 */
int top_vertex(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int k, double *bc_of_top)
{
    bspgemm_bc_info info;
    int v, best = 0;
    uint64_t *fixed = malloc(((size_t)n + 1) * sizeof(uint64_t));
    double *bc = malloc(((size_t)n + 1) * sizeof(double));
    int *sources = malloc(((size_t)k + 1) * sizeof(int));
    if (!fixed || !bc || !sources) return -1;
    for (v = 0; v < k; v++) sources[v] = v;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_BC_LANES, 16) != BSPGEMM_OK) return -1;
    if (bspgemm_betweenness(ctx, A, k, sources, fixed, bc, &info) != BSPGEMM_OK) return -1;
    if (bspgemm_betweenness(ctx, A, 0, 0, 0, 0, 0) != BSPGEMM_OK) return -1;
    if (bspgemm_betweenness(ctx, A, k, sources, fixed, 0, &info) != BSPGEMM_OK) return -1;
    for (v = 1; v < n; v++) if (fixed[v] > fixed[best]) best = v;
    *bc_of_top = n > 0 ? bc[best] : 0.0;
    free(fixed);
    free(bc);
    free(sources);
    return best + 0 * (int)(info.sigma_max + (uint64_t)info.reached + (uint64_t)info.edges_forward + (uint64_t)info.hub_chunks)
           + 0 * (info.sources + info.depth_max + info.levels + info.canonicalised);
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the bad argument is refused first
    three = (C.c_int * 3)(0, 1, 2)
    negative = (C.c_int * 3)(0, -1, 2)

    last = last_error

    def call(ctx, A, nsources, sources):
        info = dirtied(bspgemm.BcInfo, 0x5A)
        st = fn(ctx, A, nsources, sources, None, None, C.byref(info))
        assert bytes(info) == bytes(C.sizeof(info)), "info is not zeroed"
        return st

    for ctx, A in ((None, fake), (fake, None)):
        assert call(ctx, A, 3, three) == ERR_INVALID and NAME in last() and "NULL" in last(), last()
    for k in (-1, -1000):
        assert call(fake, fake, k, three) == ERR_INVALID and NAME in last() and "nsources" in last(), last()
    assert call(fake, fake, 3, None) == ERR_INVALID and NAME in last() and "sources" in last() and "NULL" in last(), last()
    assert call(fake, fake, 3, negative) == ERR_INVALID and NAME in last() and "source -1" in last() \
        and "sources[1]" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def _small_random():
    out = {}
    for seed in range(12):
        rng = np.random.default_rng(5900 + seed)
        n = int(rng.integers(2, 40))
        out["uniform_%d" % seed] = gen.uniform(n, int(rng.integers(1, 5)), 5920 + seed) if seed % 2 \
            else gen.dups_unsorted(n, int(rng.integers(1, 5)), 5920 + seed)
    return out


@pytest.mark.parametrize("name", sorted(B.GRAPHS))
def test_model_equals_the_naive_one(name):
    rp, ci, n = B.graph(name)
    sources = B.sources_of(name)
    assert [int(x) for x in B.expected(name)["fixed"]] == B.naive(rp, ci, n, sources), name
    if n:                                                     # a repeated source counts twice
        again = np.concatenate([sources[:3], sources[:1], sources[:3]])
        assert [int(x) for x in B.model(rp, ci, n, again)["fixed"]] == B.naive(rp, ci, n, again), name


def test_model_equals_the_naive_one_on_random_graphs():
    for name, (rp, ci, n) in _small_random().items():
        for sources in (np.arange(n), np.array([n - 1, 0, n - 1, n // 2])):
            res = B.model(rp, ci, n, sources)
            assert [int(x) for x in res["fixed"]] == B.naive(rp, ci, n, sources), name
            assert res["bc"].tobytes() == np.array([np.ldexp(float(int(x)), -32) for x in res["fixed"]]).tobytes()
            assert res["sources"] == len(sources) and res["reached"] >= len(sources)


@pytest.mark.parametrize("name", sorted(B.REFUSED))
def test_model_and_naive_refuse_2p63(name):
    rp, ci, n = B.graph(name)
    for fn in (B.model, B.naive):
        with pytest.raises(B.Overflow) as e:
            fn(rp, ci, n, [1, 0])                              # (vertex 1, of the first layer, passes: its counts are an eighth)
        assert (e.value.index, e.value.level) == (1, B.REFUSED[name][1]), name


def test_hand_examples():
    assert (B.model(*B.graph("path5"), range(5))["fixed"] == np.array([0, 6, 8, 6, 0], np.uint64) * np.uint64(B.ONE)).all()
    assert not B.expected("star_out")["fixed"].any()
    res = B.expected("diamond_ladder")
    assert res["fixed"].any() and not (res["fixed"] % np.uint64(B.ONE)).any() and res["sigma_max"] == 1 << 12
    # star_in: every leaf's one path to the tail runs through the hub
    assert B.expected("star_in")["fixed"].tolist() == [48 * B.ONE] + [0] * 49
    # two sources of a directed path: vertex v lies between s and everything behind v
    assert (B.model(*B.graph("dipath6"), [0, 2, 0])["fixed"] // np.uint64(B.ONE)).tolist() == [0, 8, 6, 6, 3, 0]
    assert B.expected("layers_2p62")["sigma_max"] == 1 << 62 and B.expected("layers_3p39")["sigma_max"] == 3 ** 39
    res = B.expected("empty0")
    assert res["fixed"].size == 0 and res["sources"] == 0 and res["reached"] == 0
    res = B.model(*B.graph("rmat11"), [])
    assert not res["fixed"].any() and res["fixed"].size == 2011 and res["levels"] == 0 and res["sigma_max"] == 0
    assert B.to_double(np.array([B.ONE, B.ONE // 2], np.uint64)).tolist() == [1.0, 0.5]


def _why_next():
    import networkx as nx
    return {
        "directed G(n,p)": B.from_networkx(nx.gnp_random_graph(300, 0.0305, seed=5931, directed=True), True),
        "Barabasi-Albert": B.from_networkx(nx.barabasi_albert_graph(2000, 4, seed=5932), False),
        "30x30 grid": B.grid(30),
        "powerlaw-cluster": B.from_networkx(nx.powerlaw_cluster_graph(4000, 6, 0.3, seed=5933), False),
    }


def test_deviation_from_networkx_brandes():
    """|fixed * 2^-32 - ref| <= k * m * 2^-32 + n * 2^-50 * ref for every vertex, k the number of sources and m the stored
    edges: the first term is the definition's derived bound (each summand loses under 2^-32, and a source has at most m of
    them), the second covers both sides' double rounding over at most n levels.  Sources: every vertex where n <= 600,
    else 8 seeded ones.  Measured: the largest |fixed * 2^-32 - ref| / max(ref, 1) was 2.2e-9 over the named graphs
    (symmetric_rmat9) and 2.1e-9 over the four others (powerlaw-cluster); every |diff| was at least two orders inside the bound."""
    cases = [(name, B.graph(name), np.unique(B.sources_of(name))) for name in sorted(B.GRAPHS) if B.graph(name)[2] >= 2]
    for name, (rp, ci, n) in _why_next().items():
        rng = np.random.default_rng(5940)
        cases.append((name, (rp, ci, n), np.arange(n) if n <= B.ALL_SOURCES_UP_TO else np.unique(rng.integers(0, n, 8))))
    worst = 0.0
    for name, (rp, ci, n), sources in cases:
        m = B.edges(rp, ci, n)[0].size
        ref = B.networkx_bc(rp, ci, n, sources)
        got = B.model(rp, ci, n, sources)["bc"]
        diff = np.abs(got - ref)
        bound = len(sources) * m * 2.0 ** -32 + n * 2.0 ** -50 * ref
        dev = float((diff / np.maximum(ref, 1.0)).max())
        print("%-18s n %5d, %6d stored edges, %4d sources: largest deviation %.3g, largest |diff| %.3g (bound there %.3g)"
              % (name, n, m, len(sources), dev, float(diff.max()), float(bound[np.argmax(diff)])))
        worst = max(worst, dev)
        assert (diff <= bound).all(), name
    print("largest deviation overall: %.3g" % worst)


def test_named_graphs_straddle_what_they_claim():
    out = {name: np.diff(B.canonical(*B.graph(name))[0]) for name in B.GRAPHS}
    for name, longest, chunks in (("hub_4095", 4095, 0), ("hub_4096", 4096, 0), ("hub_4097", 4097, 2),
                                  ("hub_chunks", 3 * B.HUB_CHUNK + 1, 4)):
        rp, ci, n = B.graph(name)
        assert out[name].max() == longest and (out[name] == longest).sum() == 1, name
        res = B.expected(name)
        k = len(B.sources_of(name))
        # the long row is walked by both sweeps of every source: it is in a frontier, with successors beyond it
        assert res["hub_chunks"] == 2 * k * chunks and res["reached"] == k * n and res["depth_max"] == 5, name
        assert res["fixed"][1] > 0 and res["sigma_max"] == 2, name
    assert B.graph("hub_chunks")[2] > 3 * B.HUB_CHUNK and B.HUB_CHUNK == 4096
    for name in ("path5", "symmetric_rmat9"):
        assert B.symmetric(*B.graph(name)) and B.is_canonical(*B.graph(name)), name
    assert not B.symmetric(*B.graph("dipath6")) and not B.symmetric(*B.graph("rmat11"))
    rp, ci, n = B.graph("rmat11")
    assert n % 64 and B.edges(rp, ci, n)[0].size % 64 and B.is_canonical(rp, ci, n)
    assert B.expected("rmat11")["depth_max"] >= 3 and B.expected("rmat11")["sigma_max"] > 1
    rp, ci, n = B.graph("n_4097")
    assert n == 4097 and ci.size < 4096 and rp[4097] - rp[4096] > 0
    for name in ("dups_unsorted", "untidy"):
        rp, ci, n = B.graph(name)
        assert not B.is_canonical(rp, ci, n) and B.expected(name)["canonicalised"] == 1
        assert B.edges(rp, ci, n)[0].size < ci.size, name                       # repeats
        assert any(np.any(np.diff(ci[rp[u]:rp[u + 1]]) < 0) for u in range(n)), name
    src, dst = B.edges(*B.graph("self_loops"))
    assert (src == dst).sum() == 37
    assert B.expected("disconnected")["reached"] < 2 * 20 and B.expected("disconnected")["fixed"].any()
    assert (out["star_out"] > 0).sum() == 1 and (out["star_in"] > 0).sum() == 49
    # the sizes at which a sweep takes another path: levels whose mean out-degree asks for 4, 16 and 64 lanes per vertex
    # under BC_LANES 0 (a quarter of the mean: up to 16, up to 64, above)
    assert out["dipath6"].max() <= 16 and 16 < out["star_out"][0] <= 64 and out["hub_4095"][:3].mean() > 64
    # sigma above 2^53: the conversions to double round
    assert B.expected("layers_3p39")["sigma_max"] > 1 << 53 and B.expected("layers_3p39")["sigma_max"] % 2 == 1
    assert B.expected("layers_2p62")["sigma_max"] == 1 << 62
    for name, (widths, level) in B.REFUSED.items():
        assert level <= len(widths) + 1 and B.graph(name)[2] == sum(widths) + 2
    assert B.graph("empty0")[2] == 0 and B.graph("empty1")[2] == 1 and B.graph("loop1")[1].tolist() == [0]
