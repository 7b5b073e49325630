"""The graph algorithms' arrays in the context's workspace (csrc/ws_layout.hpp): one list of arrays per entry point sizes
the workspace and places the pointers, and the pointers are taken again after anything that may have moved it.

What can go wrong is a pointer taken before the workspace moved, or an array sized differently from where it is placed.
Neither shows in a warm context whose workspace is already large, so every case runs three times and the runs are compared
bit for bit -- every output array and the info: (a) the first call of a fresh context, whose workspace grows inside the
call; (b) the same call again, warm; (c) the same call in a context that larger calls have grown past the need.  Where
tests/*_ref.py has a model, (a) is compared with it as well.

The operands have unsorted rows with a repeated entry, so every call that asks for canonical rows canonicalises mid-way (two
transposes in the workspace), and no AT is passed, so the transpose runs inside the call.  n = 1, 3 and 70: 70 is no
multiple of 4 (the padded array lengths differ from n), above 64 (two waves), and vertex 0 has degree 69.
"""
import functools

import numpy as np
import pytest

import bspgemm
import bc_ref
import bfs_tree_ref
import cc_ref
import cdlp_ref
import color_ref
import dot_ref
import extract_ref
import gen
import kcore_ref
import lcc_ref
import pagerank_ref
import scc_ref

pytestmark = pytest.mark.gpu
SIZES = (1, 3, 70)
SEED = 6100


@functools.lru_cache(maxsize=None)
def _graph(n):
    """(rp, ci, n): vertex 0 points at everybody else (degree n - 1), everybody else at three pseudo-random vertices and back
    at 0 from every third; every row is stored descending and names its first column twice"""
    rng = np.random.default_rng(SEED + n)
    rows = []
    for v in range(n):
        cols = np.arange(1, n) if v == 0 else np.unique(np.concatenate([rng.integers(0, n, size=3), [0] if v % 3 == 0 else []]))
        cols = np.asarray(cols, np.int32)[::-1]
        rows.append(np.concatenate([cols, cols[:1]]) if cols.size else np.asarray([v, v], np.int32))
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    assert not pagerank_ref.is_canonical(rp, ci, n)
    for a in (rp, ci):
        a.setflags(write=False)
    return rp, ci, n


def _lists(n):
    """the row and column lists of the extraction: rows out of order with a repeat, columns out of order"""
    return np.arange(n)[::-1][: max(1, 2 * n // 3)].tolist() + [0], np.arange(n)[::-2].tolist()


def _matrix(M):
    out = M.download()
    M.free()
    return tuple(out)


def _result(R):
    out = tuple(R.download()) + (R.download_values(),)
    R.free()
    return out


def _core(ctx, A, n):
    R, top, rounds = ctx.core_numbers(A)
    return _result(R), {"degeneracy": top, "rounds": rounds}


def _scc(ctx, A, n):
    P, count, rounds, sweeps = ctx.strongly_connected_components(A)
    return _matrix(P), {"components": count, "rounds": rounds, "sweeps": sweeps}


def _cc(ctx, A, n):
    P, count, rounds = ctx.connected_components(A)
    return _matrix(P), {"components": count, "rounds": rounds}


def _color(ctx, A, n):
    P, colors, rounds = ctx.graph_coloring(A, order="largest", seed=SEED)
    return _matrix(P), {"colors": colors, "rounds": rounds}


def _lp(ctx, A, n):
    P, info = ctx.label_propagation(A, max_iter=4)
    return _matrix(P), info


def _lcc(ctx, A, n):
    R, degree, lcc, info = ctx.local_clustering(A, directed=True)
    return _result(R) + (degree, lcc.view(np.uint64)), info


def _bfs_tree(ctx, A, n):
    R, info = ctx.bfs_tree(A, AT=None, source=0, direction="pull")
    return _result(R), info


def _pagerank(ctx, A, n):
    fixed, rank, info = ctx.pagerank(A, AT=None, method=bspgemm.PR_PULL, damping=0.85, max_iter=5)
    return (fixed, rank.view(np.uint64)), info


def _bc(ctx, A, n):
    fixed, bc, info = ctx.betweenness(A, np.arange(min(n, 5)))
    return (fixed, bc.view(np.uint64)), info


def _dot(ctx, A, n):
    R, info = ctx.multiply_masked_dot(A, A, A)
    return _result(R), info


def _extract(ctx, A, n):
    I, J = _lists(n)
    M, info = ctx.extract(A, rows=I, cols=J)
    return _matrix(M), info


def _ref_core(rp, ci, n, arrays, info):
    core, top, rounds = kcore_ref.core_numbers(rp, ci, n)
    assert np.array_equal(arrays[2], core) and info == {"degeneracy": top, "rounds": rounds}


def _ref_scc(rp, ci, n, arrays, info):
    label, count = scc_ref.labels(rp, ci, n)
    assert np.array_equal(arrays[1], label) and info["components"] == count


def _ref_cc(rp, ci, n, arrays, info):
    label, count = cc_ref.labels(rp, ci, n)
    assert np.array_equal(arrays[1], label) and info["components"] == count


def _ref_color(rp, ci, n, arrays, info):
    colour, colors, rounds = color_ref.coloring(rp, ci, n, order="largest", seed=SEED)
    assert np.array_equal(arrays[1], colour) and info == {"colors": colors, "rounds": rounds}


def _ref_lp(rp, ci, n, arrays, info):
    labels, iterations, converged, changed, communities = cdlp_ref.label_propagation(rp, ci, n, 4)
    assert np.array_equal(arrays[1], labels)
    assert (info["iterations"], info["converged"], info["changed"], info["communities"]) == (iterations, converged, changed, communities)


def _ref_lcc(rp, ci, n, arrays, info):
    num, d, lcc, triangles, reciprocal = lcc_ref.local_clustering(rp, ci, n, True)
    assert np.array_equal(arrays[2], num) and np.array_equal(arrays[3], d) and np.array_equal(arrays[4], lcc.view(np.uint64))
    assert (info["triangles"], info["reciprocal"]) == (triangles, reciprocal)


def _ref_bfs_tree(rp, ci, n, arrays, info):
    e_rp, e_parent, e_level = bfs_tree_ref.bfs_tree(rp, ci, n, 0)
    assert all(np.array_equal(g, e) for g, e in zip(arrays, (e_rp, e_parent, e_level)))
    assert info["reached"] == e_parent.size and info["transposed"] == (1 if info["pull_levels"] else 0)


def _ref_pagerank(rp, ci, n, arrays, info):
    e = pagerank_ref.pagerank(rp, ci, n, 0.85, 5)
    assert np.array_equal(arrays[0], e["fixed"]) and np.array_equal(arrays[1], e["rank"].view(np.uint64))
    assert all(info[k] == e[k] for k in ("mass", "delta", "dangling", "iterations", "converged"))
    assert info["transposed"] == 1 and info["canonicalised"] == 1


def _ref_bc(rp, ci, n, arrays, info):
    e = bc_ref.model(rp, ci, n, np.arange(min(n, 5)))
    assert np.array_equal(arrays[0], e["fixed"]) and np.array_equal(arrays[1], e["bc"].view(np.uint64))
    assert all(info[k] == e[k] for k in info if k != "canonicalised") and info["canonicalised"] == 1


def _ref_dot(rp, ci, n, arrays, info):
    e = dot_ref.dot_ref((rp, ci), (rp, ci), (rp, ci), n, n, n, n)
    assert all(np.array_equal(g, x) for g, x in zip(arrays, e))
    assert info["kept"] == e[1].size and info["canonicalised"] == 7


def _ref_extract(rp, ci, n, arrays, info):
    I, J = _lists(n)
    e = extract_ref.model(rp, ci, n, n, I, J)
    assert np.array_equal(arrays[0], e["rp"]) and np.array_equal(arrays[1], e["ci"])
    assert all(info[k] == e[k] for k in ("kept", "scanned", "hub_chunks", "cols_monotone", "sorted_by", "canonicalised"))


CALLS = {
    "core_numbers": (_core, _ref_core),
    "scc": (_scc, _ref_scc),
    "cc": (_cc, _ref_cc),
    "coloring": (_color, _ref_color),
    "label_propagation": (_lp, _ref_lp),
    "lcc": (_lcc, _ref_lcc),
    "bfs_tree": (_bfs_tree, _ref_bfs_tree),
    "pagerank_pull": (_pagerank, _ref_pagerank),
    "betweenness": (_bc, _ref_bc),
    "masked_dot": (_dot, _ref_dot),
    "extract": (_extract, _ref_extract),
}


def _run(ctx, name, n):
    rp, ci, _ = _graph(n)
    A = ctx.upload(rp, ci, n)
    try:
        return CALLS[name][0](ctx, A, n)
    finally:
        A.free()


@pytest.fixture(scope="module")
def grown():
    """a context whose workspaces every entry point has already grown, on an untidy graph of 2000 vertices"""
    ctx = bspgemm.Context(0)
    rp, ci, n = gen.dups_unsorted(2000, 8, SEED)
    A = ctx.upload(rp, ci, n)
    for name in CALLS:
        CALLS[name][0](ctx, A, n)
    A.free()
    yield ctx
    ctx.close()


def _same(x, y):
    return x[1] == y[1] and len(x[0]) == len(y[0]) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(x[0], y[0]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(CALLS))
def test_cold_warm_and_grown_workspaces_agree(grown, name, n):
    ctx = bspgemm.Context(0)
    try:
        cold = _run(ctx, name, n)
        warm = _run(ctx, name, n)
    finally:
        ctx.close()
    past = _run(grown, name, n)
    assert _same(cold, warm), "%s n %d: the warm call differs from the cold one" % (name, n)
    assert _same(cold, past), "%s n %d: the call in a grown workspace differs from the cold one" % (name, n)
    rp, ci, _ = _graph(n)
    CALLS[name][1](rp, ci, n, *cold)
