"""bspgemm_pagerank on the GPU at every hub-chunk and grid-stride edge of csrc/pagerank.hip: the edge graphs of
pagerank_ref.py (tests/test_pagerank_edges_shapes.py proves without a GPU which kernel edges they reach) give the numpy model's
bits under PULL with AT given, PULL with AT NULL and PUSH, under every PR_MIN_CLASS, from a col_idx off 16-byte alignment,
and under BSPGEMM_PR_TIMING, whose line on stderr carries the model's class sizes, lanes per wave-class row, chunk count and
dangling count.
"""
import os
import re

import numpy as np
import pytest

import bspgemm
import pagerank_ref as P

pytestmark = pytest.mark.gpu
FORMS = (("PULL, AT given", P.PR_PULL, True), ("PULL, AT NULL", P.PR_PULL, False), ("PUSH", P.PR_PUSH, False))
LINE = re.compile(r"\[bspgemm\] bspgemm_pagerank: n (\d+) nnz (\d+) (pull|push) classes (\d+)/(\d+)/(\d+)/(\d+) "
                  r"\((\d+) lanes per wave-class row\) chunks (\d+) dangling (\d+) \| .* \+ (\d+) iterations ")


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def timed():
    """a second context, created under BSPGEMM_PR_TIMING (read once, in bspgemm_create)"""
    os.environ["BSPGEMM_PR_TIMING"] = "1"
    try:
        c = bspgemm.Context(0)
    finally:
        del os.environ["BSPGEMM_PR_TIMING"]
    yield c
    c.close()


def _check(got, exp, method, what):
    fixed, rank, info = got
    assert fixed.dtype == np.uint64 and np.array_equal(fixed, exp["fixed"]), what
    assert rank.tobytes() == exp["rank"].tobytes(), what
    for k in ("mass", "delta", "dangling", "iterations", "converged"):
        assert info[k] == exp[k], (what, k, info[k], exp[k])
    assert info["method"] == method and info["canonicalised"] == 0, what
    return fixed.tobytes()


def _expected(name, damping, at):
    rp, ci, n = P.graph(name)
    rs, deltas, _ = P.cached_trajectory(name, damping, P.EDGE_ITERATIONS[name])
    return P.result(rs, deltas, False, rp, ci, n, at=at)


def _operands(c, name):
    rp, ci, n = P.graph(name)
    A = c.upload(rp, ci, n)
    t_rp, t_ci, _ = P.transposed(rp, ci, n)
    return A, c.upload(t_rp, t_ci, n)


def _run_forms(c, A, AT, name, min_class, damping, it):
    rp, ci, n = P.graph(name)
    exp = _expected(name, damping, it)
    for what, method, give_at in FORMS:
        what = (name, what, "PR_MIN_CLASS %d" % min_class, damping, it)
        _, _, info = got = c.pagerank(A, AT if give_at else None, method, damping, it)
        _check(got, exp, method, what)
        assert info["class_vertices"] == (P.class_vertices(rp, ci, n, min_class) if method == P.PR_PULL else [0, 0, 0, 0]), what
        assert info["transposed"] == (1 if method == P.PR_PULL and not give_at else 0), what


@pytest.mark.parametrize("name", sorted(P.EDGE_GRAPHS))
def test_equals_the_model_in_every_form(ctx, name):
    A, AT = _operands(ctx, name)
    try:
        _run_forms(ctx, A, AT, name, 0, 0.85, P.EDGE_ITERATIONS[name])
    finally:
        AT.free()
        A.free()


def test_hubs_under_every_min_class_damping_and_iteration_count(ctx):
    A, AT = _operands(ctx, "hubs")
    try:
        for min_class in P.EDGE_MIN_CLASSES["hubs"]:
            ctx.set_option("pr_min_class", min_class)
            for damping in (0.85, 1.0):
                for it in (1, 2, 20):
                    _run_forms(ctx, A, AT, "hubs", min_class, damping, it)
    finally:
        ctx.set_option("pr_min_class", 0)
        AT.free()
        A.free()


@pytest.mark.parametrize("name", ["wide", "wave64"])
def test_wide_graphs_under_every_min_class(ctx, name):
    """two iterations: every vertex through the wave kernel, through k_pr_group, and as a hub of at most one chunk"""
    rp, ci, n = P.graph(name)
    A, AT = _operands(ctx, name)
    exp = _expected(name, 0.85, 2)
    try:
        for min_class in (1, 2, 3):
            assert min_class in P.EDGE_MIN_CLASSES[name]
            ctx.set_option("pr_min_class", min_class)
            _, _, info = got = ctx.pagerank(A, AT, P.PR_PULL, 0.85, 2)
            _check(got, exp, P.PR_PULL, (name, min_class))
            assert info["class_vertices"] == P.class_vertices(rp, ci, n, min_class), (name, min_class, info)
    finally:
        ctx.set_option("pr_min_class", 0)
        AT.free()
        A.free()


@pytest.mark.parametrize("name", sorted(P.EDGE_GRAPHS))
def test_push_from_an_unaligned_col_idx(ctx, name):
    """A wrapped from a device buffer 1, 2 and 3 ints off 16-byte alignment: k_pr_push reads it entry by entry"""
    import torch
    rp, ci, n = P.graph(name)
    assert P.is_canonical(rp, ci, n)                           # (else the call would read a canonical copy of its own)
    K = P.EDGE_ITERATIONS[name]
    exp = _expected(name, 0.85, K)
    d_rp = torch.from_numpy(np.array(rp)).cuda()
    seen = set()
    for shift in (0, 1, 2, 3):
        buf = torch.zeros(ci.size + 4, dtype=torch.int32, device="cuda")
        buf[shift:shift + ci.size] = torch.from_numpy(np.array(ci)).cuda()
        torch.cuda.synchronize()
        d_ci = buf[shift:]
        assert d_ci.data_ptr() % 16 == 4 * shift
        W = ctx.wrap_device(n, n, ci.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, buf))
        try:
            seen.add(_check(ctx.pagerank(W, None, P.PR_PUSH, 0.85, K), exp, P.PR_PUSH, (name, "col_idx %d ints off" % shift)))
        finally:
            W.free()
    assert len(seen) == 1


def _timed_line(capfd, call):
    capfd.readouterr()
    got = call()
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "bspgemm_pagerank:" in ln]
    assert len(lines) == 1, lines
    m = LINE.search(lines[0])
    assert m, lines[0]
    f = [int(x) if x.isdigit() else x for x in m.groups()]
    return got, {"n": f[0], "nnz": f[1], "method": f[2], "classes": f[3:7], "lanes": f[7], "chunks": f[8], "dangling": f[9],
                 "iterations": f[10]}


@pytest.mark.parametrize("name", ["hubs", "lanes_at_32", "lanes_above_32"])
def test_timing_mode_gives_the_same_bits_and_reports_the_model(ctx, timed, capfd, name):
    rp, ci, n = P.graph(name)
    K = P.EDGE_ITERATIONS[name]
    exp = _expected(name, 0.85, K)
    A, AT = _operands(ctx, name)
    At, ATt = _operands(timed, name)
    try:
        for min_class in P.EDGE_MIN_CLASSES[name]:
            ctx.set_option("pr_min_class", min_class)
            timed.set_option("pr_min_class", min_class)
            for what, method, give_at in FORMS:
                what = (name, what, min_class)
                capfd.readouterr()
                plain = _check(ctx.pagerank(A, AT if give_at else None, method, 0.85, K), exp, method, what)
                assert "[bspgemm]" not in capfd.readouterr().err, what      # an untimed context writes nothing
                got, line = _timed_line(capfd, lambda: timed.pagerank(At, ATt if give_at else None, method, 0.85, K))
                assert _check(got, exp, method, what) == plain
                pull = method == P.PR_PULL
                assert line == {"n": n, "nnz": ci.size, "method": "pull" if pull else "push",
                                "classes": P.class_vertices(rp, ci, n, min_class) if pull else [0, 0, 0, 0],
                                "lanes": P.wave_lanes(rp, ci, n, min_class) if pull else 64,
                                "chunks": P.hub_chunks(rp, ci, n, min_class) if pull else 0,
                                "dangling": exp["dangling"], "iterations": K}, (what, line)
                if pull:
                    assert got[2]["class_vertices"] == line["classes"]
    finally:
        ctx.set_option("pr_min_class", 0)
        timed.set_option("pr_min_class", 0)
        for h in (ATt, At, AT, A):
            h.free()
    assert "BSPGEMM_PR_TIMING" not in os.environ
