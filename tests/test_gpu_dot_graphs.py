"""The two loops with a method argument: bspgemm_triangle_count_ex under both methods equals the scipy count,
bspgemm_ktruss_ex(DOT) equals bspgemm_ktruss bit for bit with equal iterations and converged -- on a symmetric graph, on a
non-symmetric one (the transpose branch), for k = 2, with max_iter = 1 and for a k that empties the graph -- and
SpGEMM_hip_ktruss --dot prints what the plain run prints."""
import os
import subprocess

import numpy as np
import pytest

import bspgemm
import gen
import ktruss_ref

pytestmark = pytest.mark.gpu
SKEW = (0.57, 0.19, 0.19, 0.05)
CLI = os.path.join(os.path.dirname(bspgemm.LIB_PATH), "SpGEMM_hip_ktruss")


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def graphs():
    """(row_ptr, col_idx, n): a symmetric R-MAT scale 10 graph, and a directed one with repeats, unsorted rows and a diagonal"""
    rp, ci, n = gen.rmat(10, 8, SKEW, 9101)
    sym = ktruss_ref.symmetrise(rp, ci, n) + (n,)
    d_rp, d_ci, dn = gen.rmat(9, 14, SKEW, 9102)
    rows = np.repeat(np.arange(dn), np.diff(d_rp))
    rng = np.random.default_rng(9103)
    extra = rng.integers(0, d_ci.size, d_ci.size // 5)                # repeats, and every vertex's diagonal entry
    r = np.concatenate([rows, rows[extra], np.arange(dn)])
    c = np.concatenate([d_ci, d_ci[extra], np.arange(dn)])
    order = rng.permutation(r.size)
    order = order[np.argsort(r[order], kind="stable")]                # rows together, entries in random order
    directed = (np.concatenate([[0], np.cumsum(np.bincount(r, minlength=dn))]).astype(np.int32), c[order].astype(np.int32), dn)
    return {"symmetric": sym, "directed": directed}


def _truss(ctx, A, k, max_iter, method):
    T, it, conv = ctx.ktruss(A, k, max_iter, method=method)
    out = T.download()
    T.free()
    return out, it, conv


def _same(ctx, g, k, max_iter=0):
    rp, ci, n = g
    A = ctx.upload(rp, ci, n)
    try:
        p, d = _truss(ctx, A, k, max_iter, "product"), _truss(ctx, A, k, max_iter, "dot")
    finally:
        A.free()
    assert np.array_equal(p[0][0], d[0][0]) and np.array_equal(p[0][1], d[0][1]), "k = %d: the trusses differ" % k
    assert p[1:] == d[1:], "k = %d: (iterations, converged) %r under PRODUCT, %r under DOT" % (k, p[1:], d[1:])
    return d


@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_triangles_under_both_methods(ctx, graphs, kind):
    rp, ci, n = graphs[kind]
    expect = ktruss_ref.triangles_ref(rp, ci, n)
    assert expect > 100
    A = ctx.upload(rp, ci, n)
    assert ctx.triangle_count(A) == expect
    assert ctx.triangle_count(A, method="product") == expect
    assert ctx.triangle_count(A, method="dot") == expect
    A.free()


@pytest.mark.parametrize("k", [3, 4, 5])
def test_ktruss_symmetric(ctx, graphs, k):
    (t_rp, t_ci), it, conv = _same(ctx, graphs["symmetric"], k)
    (e_rp, e_ci), e_it, e_conv = ktruss_ref.ktruss_ref(*graphs["symmetric"], k)
    assert np.array_equal(t_rp, e_rp) and np.array_equal(t_ci, e_ci) and (it, conv) == (e_it, e_conv)
    assert 0 < t_ci.size and it >= 2


def test_ktruss_directed_takes_the_transpose_branch(ctx, graphs):
    rp, ci, n = graphs["directed"]
    s_rp, s_ci = ktruss_ref.dedup_ref(*ktruss_ref.select_ref(rp, ci, "offdiag"), n)
    t_rp, t_ci = ktruss_ref.symmetrise(s_rp, s_ci, n)
    assert t_ci.size > s_ci.size                                      # S0 is not its own transpose
    for k in (3, 4):
        (g_rp, g_ci), it, conv = _same(ctx, graphs["directed"], k)
        (e_rp, e_ci), e_it, e_conv = ktruss_ref.ktruss_ref(rp, ci, n, k)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci) and (it, conv) == (e_it, e_conv), k
        assert it >= 2                                                # a later step transposes its own S


def test_ktruss_edge_cases(ctx, graphs):
    for kind in ("symmetric", "directed"):
        g = graphs[kind]
        (rp2, ci2), it, conv = _same(ctx, g, 2)                       # k = 2: S0 itself, no support counted
        e_rp, e_ci = ktruss_ref.dedup_ref(*ktruss_ref.select_ref(g[0], g[1], "offdiag"), g[2])
        assert (it, conv) == (0, True) and np.array_equal(rp2, e_rp) and np.array_equal(ci2, e_ci)
        _, it, conv = _same(ctx, g, 4, max_iter=1)                    # capped after one step
        assert (it, conv) == (1, False)
        (_, ci_e), it, conv = _same(ctx, g, 100000)                   # a k that empties the graph
        assert ci_e.size == 0 and (it, conv) == (1, True)


def _csv(args):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    fields = r.stdout.strip().split(",")
    assert len(fields) == 8, r.stdout
    return fields[:7]                                                  # (without ms)


def test_cli_dot_flag(golden_dir, tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    src = os.path.join(golden_dir, "validity_test.mtx")
    plain, dot = _csv([src, "3"]), _csv(["--dot", src, "3"])
    assert dot == plain, (plain, dot)
    # with --symmetrize, in either order, and the written truss
    out_p, out_d = str(tmp_path / "p.mtx"), str(tmp_path / "d.mtx")
    sym = _csv(["--symmetrize", src, "3", out_p])
    assert _csv(["--symmetrize", "--dot", src, "3", out_d]) == sym
    assert _csv(["--dot", "--symmetrize", src, "3"]) == sym
    assert open(out_p).read() == open(out_d).read()
    r = subprocess.run([CLI, "--dot", src], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout.startswith("usage: SpGEMM_hip_ktruss")
