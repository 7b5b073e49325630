"""The device-resident fixed-point PageRank (bspgemm_pagerank) at the ABI level, without a GPU: the header declares the enum,
the info struct and the function with the agreed argument list between bspgemm_local_clustering and bspgemm_closure and
carries the definition, the library exports it, the Python view has it, a C99 caller compiles cleanly, bad arguments are
refused by name before anything is dereferenced -- and the tests' own reference (pagerank_ref.py) equals a naive model in
Python integers, reproduces the examples worked by hand, keeps the mass under 2^62 and stays within 1e-9 of a float64
power iteration.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
import kcore_ref
import pagerank_ref as P
from abi_kit import ERR_INVALID, FAKE, header_code, header_text, compile_c99, last_error, dirtied

NAME = "bspgemm_pagerank"

ENUM = "typedef enum bspgemm_pr_method { BSPGEMM_PR_AUTO = 0, BSPGEMM_PR_PULL = 1, BSPGEMM_PR_PUSH = 2 } bspgemm_pr_method;"
STRUCT = ("typedef struct bspgemm_pr_info { uint64_t mass; uint64_t delta; int64_t dangling; int64_t class_vertices[4]; "
          "int iterations, converged; int method; int transposed; int canonicalised; } bspgemm_pr_info;")
DECLARATION = ("bspgemm_status bspgemm_pagerank(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT, "
               "bspgemm_pr_method method, double damping, int max_iter, double tolerance, uint64_t *rank_fixed_host, "
               "double *rank_host, bspgemm_pr_info *info);")


def test_header_declares_it_between_local_clustering_and_closure():
    code = header_code()
    assert ENUM in code and STRUCT in code, "include/bspgemm.h does not declare bspgemm_pr_method and bspgemm_pr_info as agreed"
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_local_clustering(") < code.index(ENUM) < code.index(STRUCT) < code.index(NAME + "(") \
        < code.index("bspgemm_closure(")
    assert "BSPGEMM_OPT_PR_MIN_CLASS = 12" in code
    text = header_text()
    comment = text.split("typedef enum bspgemm_pr_method")[0].rsplit("/*", 1)[1]
    # the definition is the contract
    for word in ("ONE = 2^62", "q = floor(ONE / n)", "floor(damping * 4294967296.0 + 0.5)", "B = ((2^32 - D) * q) >> 32",
                 "r_0(v) = q", "floor(r_{t-1}(u) / outdeg(u))", "0 for a dangling u", "B + floor(D * s(v) / 2^32)",
                 "D*(s>>32) + ((D*(s & 0xffffffff))>>32)", "Repeats count once".lower(), "self-loops are kept as stored",
                 "at most ONE", "under 2^63", "floor(tolerance * 2^62)", "ldexp((double) r(v), -62)",
                 "r.astype(np.float64) * 2.0**-62", "less than 2^-62", "2.0e-13", "1e-4", "AUTO is PULL",
                 "memory-safely", "BSPGEMM_OPT_PR_MIN_CLASS", "BSPGEMM_PR_TIMING", "out of", "statistics",
                 "Nothing is leaked", "no synchronisation", "8-byte read-back"):
        assert word in comment, word
    assert "PR_MIN_CLASS" in text.split("typedef enum bspgemm_option")[0] and "BSPGEMM_PR_TIMING" in text.split("typedef struct bspgemm_context")[0]


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 10
    assert callable(getattr(bspgemm.Context, "pagerank", None)), "Context.pagerank"
    assert (bspgemm.PR_AUTO, bspgemm.PR_PULL, bspgemm.PR_PUSH) == (0, 1, 2)
    assert bspgemm.OPTIONS["pr_min_class"] == 12
    assert C.sizeof(bspgemm.PrInfo) == 3 * 8 + 4 * 8 + 5 * 4 + 4              # (padded to the 8-byte alignment)
    assert [f for f, _ in bspgemm.PrInfo._fields_] == ["mass", "delta", "dangling", "class_vertices", "iterations", "converged",
                                                       "method", "transposed", "canonicalised"]
    assert bspgemm.PrInfo.iterations.offset == 56 and bspgemm.PrInfo.canonicalised.offset == 72


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the highest-ranked vertex after 20 pull iterations, or -1 */
int top_vertex(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT, int n, double *rank_of_top)
{
    bspgemm_pr_info info;
    int v, best = 0;
    uint64_t *fixed = malloc(((size_t)n + 1) * sizeof(uint64_t));
    double *rank = malloc(((size_t)n + 1) * sizeof(double));
    if (!fixed || !rank) return -1;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_PR_MIN_CLASS, 0) != BSPGEMM_OK) return -1;
    if (bspgemm_pagerank(ctx, A, AT, BSPGEMM_PR_PULL, 0.85, 20, 0.0, fixed, rank, &info) != BSPGEMM_OK) return -1;
    if (bspgemm_pagerank(ctx, A, 0, BSPGEMM_PR_AUTO, 0.85, 100, 1e-9, 0, 0, 0) != BSPGEMM_OK) return -1;
    if (bspgemm_pagerank(ctx, A, 0, BSPGEMM_PR_PUSH, 0.5, 1, 0.0, fixed, 0, &info) != BSPGEMM_OK) return -1;
    for (v = 1; v < n; v++) if (fixed[v] > fixed[best]) best = v;
    *rank_of_top = n > 0 ? rank[best] : 0.0;
    free(fixed);
    free(rank);
    return best + 0 * (int)(info.mass + info.delta + (uint64_t)info.dangling + (uint64_t)info.class_vertices[3])
           + 0 * (info.iterations + info.converged + info.method + info.transposed + info.canonicalised);
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the bad argument is refused first
    nan = float("nan")

    last = last_error

    def call(ctx, A, method=1, damping=0.85, max_iter=20, tolerance=0.0):
        info = dirtied(bspgemm.PrInfo, 0x5A)
        st = fn(ctx, A, None, method, damping, max_iter, tolerance, None, None, C.byref(info))
        assert bytes(info) == bytes(C.sizeof(info)), "info is not zeroed"
        return st

    for ctx, A in ((None, fake), (fake, None)):
        assert call(ctx, A) == ERR_INVALID and NAME in last() and "NULL" in last(), last()
    for method in (3, -1, 99):
        assert call(fake, fake, method=method) == ERR_INVALID and NAME in last() and "method" in last(), last()
    for damping in (-0.1, 1.5, nan):
        assert call(fake, fake, damping=damping) == ERR_INVALID and NAME in last() and "damping" in last(), last()
    assert call(fake, fake, max_iter=-1) == ERR_INVALID and NAME in last() and "max_iter" in last(), last()
    for tolerance in (-1.0, nan):
        assert call(fake, fake, tolerance=tolerance) == ERR_INVALID and NAME in last() and "tolerance" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def _small_random():
    out = {name: P.graph(name) for name in P.SMALL}
    for seed in range(12):
        rng = np.random.default_rng(5700 + seed)
        n = int(rng.integers(2, 40))
        out["uniform_%d" % seed] = gen.uniform(n, int(rng.integers(1, 5)), 5720 + seed) if seed % 2 \
            else gen.dups_unsorted(n, int(rng.integers(1, 5)), 5720 + seed)
    return out


@pytest.mark.parametrize("damping", P.DAMPINGS)
def test_model_equals_the_naive_one(damping):
    for name, (rp, ci, n) in _small_random().items():
        for tolerance, max_iter in ((0.0, 7), (1e-3, 30)):
            rs, deltas, conv = P.trajectory(rp, ci, n, damping, max_iter, tolerance)
            r, nd, nconv = P.naive(rp, ci, n, damping, max_iter, tolerance)
            assert [int(x) for x in rs[-1]] == r and deltas == nd and conv == nconv, (name, damping, tolerance)


def test_hand_examples():
    # two_cycle under damping 1: every r_t = q (B = 0, D = 2^32, c = r)
    rs, deltas, _ = P.trajectory(*P.graph("two_cycle"), 1.0, 9)
    assert all((r == np.uint64(1 << 61)).all() for r in rs) and deltas == [0] * 9
    # n = 1: r = B + ((D q) >> 32), dangling (share = r) or a self-loop (c = r) alike
    for damping in P.DAMPINGS:
        q, D, B = P.constants(1, damping)
        assert q == 1 << 62
        for name in ("empty1", "loop1"):
            rs, _, _ = P.trajectory(*P.graph(name), damping, 1)
            assert int(rs[1][0]) == B + ((D * q) >> 32), (name, damping)
    # all_dangling: every vertex equal, at every iteration
    rs, _, _ = P.trajectory(*P.graph("all_dangling"), 0.85, 5)
    assert all((r == r[0]).all() for r in rs)
    res = P.pagerank(*P.graph("all_dangling"), 0.85, 5)
    assert res["dangling"] == 300 and res["iterations"] == 5 and res["converged"] == 0
    # damping 0: B = q, D = 0, so r_t = q for every t on every graph
    for name in P.GRAPHS:
        rp, ci, n = P.graph(name)
        q, D, B = P.constants(n, 0.0)
        assert D == 0 and B == q
        rs, deltas, _ = P.trajectory(rp, ci, n, 0.0, 3)
        assert all((r == np.uint64(q)).all() for r in rs) and deltas == [0, 0, 0], name
    assert P.constants(7, 1.0)[1] == 1 << 32 and P.constants(7, 0.5000001)[1] == 2147484077
    # max_iter 0 and the empty graph
    res = P.pagerank(*P.graph("empty0"), 0.85, 4)
    assert res["fixed"].size == 0 and res["mass"] == 0 and res["iterations"] == 4 and res["delta"] == 0
    res = P.pagerank(*P.graph("rmat11"), 0.85, 0)
    assert res["iterations"] == 0 and res["delta"] == 0 and (res["fixed"] == np.uint64((1 << 62) // 2011)).all()
    assert P.to_double(np.array([1 << 62, 1 << 61], np.uint64)).tolist() == [1.0, 0.5]


@pytest.mark.parametrize("name", sorted(P.GRAPHS))
def test_mass_stays_under_one_and_only_floors_lose_it(name):
    rp, ci, n = P.graph(name)
    src, _ = P.edges(rp, ci, n)
    for damping in P.DAMPINGS:
        rs, _, _ = P.cached_trajectory(name, damping)
        mass = [int(r.sum(dtype=np.uint64)) for r in rs]
        start = n * P.constants(n, damping)[0]
        assert mass[0] == start <= P.ONE
        # it never grows: sum of s <= the mass before, and n B + D / 2^32 * that <= n q.  An iteration loses less than
        # one unit per floor: c(u), which counts once for every out-edge of u, the share, counted n times, and one
        # each per vertex in B and in r_t
        slack = src.size + 3 * n
        for t, m in enumerate(mass):
            assert m <= start and start - m <= t * slack, (name, damping, t)


def test_deviation_from_the_float64_iteration():
    """the largest relative deviation over all GRAPHS (20 iterations) and over R-MAT scale 14 at 1, 20 and 100 iterations;
    measured at 2.0e-13 at most on R-MAT 14 and 8.2e-13 on hub_chunks, the cap leaves three orders of magnitude and sits five inside Graphalytics' 1e-4"""
    worst = 0.0
    cases = [(name, P.graph(name), (20,)) for name in sorted(P.GRAPHS)]
    cases.append(("rmat14", gen.rmat(14, 16, kcore_ref.SKEW, 5750), (1, 20, 100)))
    for name, (rp, ci, n), its in cases:
        if n == 0:
            continue
        rs, _, _ = P.trajectory(rp, ci, n, 0.85, max(its))
        for it in its:
            f = P.float_iteration(rp, ci, n, 0.85, it)
            dev = float((np.abs(P.to_double(rs[it]) - f) / f).max())
            print("%-18s %3d iterations: largest relative deviation %.3g" % (name, it, dev))
            worst = max(worst, dev)
    print("largest relative deviation overall: %.3g" % worst)
    assert worst <= 1e-9


def test_named_graphs_straddle_what_they_claim():
    for K in P.CAPS:
        d = P.indegree(*P.graph("sink_star_%d" % K))
        for want in (K - 1, K, K + 1):
            assert (d == want).sum() == 1, (K, want)
        out = np.diff(P.canonical(*P.graph("sink_star_%d" % K))[0])
        assert len(set(out.tolist())) >= 4 and (out == 0).sum() == 3
        cls = P.class_vertices(*P.graph("sink_star_%d" % K))
        assert cls[P.CAPS.index(K)] >= 2 and cls[P.CAPS.index(K) + 1] == 1, cls
    rp, ci, n = P.graph("hub_chunks")
    d = P.indegree(rp, ci, n)
    assert d.max() == 3 * P.HUB_CHUNK + 1 and (d > P.GROUP_CAP).sum() == 1 and P.hub_chunks(rp, ci, n) == 4
    assert P.class_vertices(rp, ci, n, 3) == [0, 0, 0, n] and P.hub_chunks(rp, ci, n, 3) == 4 + int((d[1:] > 0).sum())
    assert np.diff(P.canonical(*P.graph("source_star"))[0]).max() == 5000
    rp, ci, n = P.graph("rmat11")
    assert n % 64 and P.edges(rp, ci, n)[0].size % 64 and P.class_vertices(rp, ci, n)[1] > 0
    rp, ci, n = P.graph("symmetric_rmat9")
    assert np.array_equal(P.transposed(rp, ci, n)[1], ci) and np.array_equal(P.transposed(rp, ci, n)[0], rp)
    rp, ci, n = P.graph("n_4097")
    assert n == 4097 and ci.size < 4096 and P.indegree(rp, ci, n)[4096] > 0 and rp[4097] - rp[4096] > 0
    assert P.is_canonical(*P.graph("rmat11")) and P.is_canonical(*P.graph("symmetric_rmat9"))
    for name in ("dups_unsorted", "untidy"):
        rp, ci, n = P.graph(name)
        assert not P.is_canonical(rp, ci, n)
        assert P.edges(rp, ci, n)[0].size < ci.size, name                       # repeats
        assert any(np.any(np.diff(ci[rp[u]:rp[u + 1]]) < 0) for u in range(n)), name
    assert (P.indegree(*P.graph("self_loops")) >= 1).all()
    assert (np.diff(P.graph("path_dangling_end")[0]) == 0).sum() == 1
