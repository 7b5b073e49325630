"""bspgemm_betweenness on the GPU against the numpy model of its definition (bc_ref.py): the fixed-point sums, the doubles'
bytes and every field of the info are EQUAL to the model's on every named graph, under every BC_LANES, twice in a row and
after other graph calls on the same context, with every output NULL, for every form of the operand; path counts of 2^63 are
refused with the outputs untouched; the multiply statistics stay what they were; every refused argument leaves a usable
context.
"""
import ctypes as C

import numpy as np
import pytest

import bspgemm
import gen
import bc_ref as B

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_OVERFLOW = 1, 5
INFO = ("sigma_max", "reached", "edges_forward", "hub_chunks", "sources", "depth_max", "levels", "canonicalised")


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _check(got, exp, what):
    fixed, bc, info = got
    assert fixed.dtype == np.uint64 and np.array_equal(fixed, exp["fixed"]), what
    assert bc.tobytes() == exp["bc"].tobytes(), what
    for k in INFO:
        assert info[k] == exp[k], (what, k, info[k], exp[k])
    return fixed.tobytes()


@pytest.mark.parametrize("name", sorted(B.GRAPHS))
def test_equals_the_model(ctx, name):
    """every BC_LANES, and the automatic choice twice in a row"""
    rp, ci, n = B.graph(name)
    sources, exp = B.sources_of(name), B.expected(name)
    A = ctx.upload(rp, ci, n)
    try:
        for lanes in B.LANES + (0,):
            ctx.set_option("bc_lanes", lanes)
            _check(ctx.betweenness(A, sources), exp, (name, lanes))
    finally:
        ctx.set_option("bc_lanes", 0)
        A.free()


def test_bc_lanes_option(ctx):
    for bad in (1, 8, 32, 128, -4):
        with pytest.raises(bspgemm.BspgemmError):
            ctx.set_option("bc_lanes", bad)
    assert ctx.get_option("bc_lanes") == 0
    ctx.set_option("bc_lanes", 16)
    assert ctx.get_option("bc_lanes") == 16
    ctx.set_option("bc_lanes", 0)


@pytest.mark.parametrize("name", ["rmat11", "hub_4097", "diamond_ladder"])
def test_sources_in_any_number_and_order(ctx, name):
    rp, ci, n = B.graph(name)
    A = ctx.upload(rp, ci, n)
    first = B.sources_of(name)[:5]
    try:
        for sources in ([], first[:1], first[::-1], np.concatenate([first, first[:2], first])):
            _check(ctx.betweenness(A, sources), B.model(rp, ci, n, sources), (name, list(sources)))
    finally:
        A.free()


def test_workspace_reuse(ctx):
    """a call after other graph calls and after a larger betweenness on the same context"""
    rp, ci, n = B.graph("rmat11")
    sources, exp = B.sources_of("rmat11"), B.expected("rmat11")
    A = ctx.upload(rp, ci, n)
    big = ctx.upload(*B.graph("hub_chunks"))
    try:
        first = _check(ctx.betweenness(A, sources), exp, "first")
        assert _check(ctx.betweenness(A, sources), exp, "second") == first
        _check(ctx.betweenness(big, B.sources_of("hub_chunks")), B.expected("hub_chunks"), "larger")
        tree, _ = ctx.bfs_tree(A, None, int(sources[0]), "push")
        tree.free()
        assert _check(ctx.betweenness(A, sources), exp, "after bfs_tree") == first
        ctx.pagerank(A, None, max_iter=3)
        assert _check(ctx.betweenness(A, sources), exp, "after pagerank") == first
    finally:
        big.free()
        A.free()


def test_null_outputs(ctx):
    L = bspgemm.lib()
    name = "hub_4097"
    rp, ci, n = B.graph(name)
    sources, exp = np.ascontiguousarray(B.sources_of(name)), B.expected(name)
    A = ctx.upload(rp, ci, n)
    try:
        for want_fixed, want_bc, want_info in ((1, 0, 1), (0, 1, 1), (0, 0, 1), (1, 1, 0), (0, 0, 0)):
            fixed, bc, info = np.zeros(n, np.uint64), np.zeros(n, np.float64), bspgemm.BcInfo()
            st = L.bspgemm_betweenness(ctx._h, A._h, sources.size, sources.ctypes.data, fixed.ctypes.data if want_fixed else None,
                                       bc.ctypes.data if want_bc else None, C.byref(info) if want_info else None)
            assert st == 0, L.bspgemm_last_error()
            if want_fixed:
                assert np.array_equal(fixed, exp["fixed"])
            if want_bc:
                assert bc.tobytes() == exp["bc"].tobytes()
            if want_info:
                assert all(getattr(info, k) == exp[k] for k in INFO), info.as_dict()
    finally:
        A.free()


def test_operands_in_every_form(ctx):
    import torch
    name = "rmat11"
    rp, ci, n = B.graph(name)
    sources, exp = B.sources_of(name), B.expected(name)
    A = ctx.upload(rp, ci, n)
    d_rp, d_ci = torch.from_numpy(np.array(rp)).cuda(), torch.from_numpy(np.array(ci)).cuda()
    torch.cuda.synchronize()
    W = ctx.wrap_device(n, n, ci.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci))
    I = ctx.upload(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), n)
    R = ctx.multiply(I, A)
    M = ctx.matrix_from_result(R, n)
    R.free()
    # the same graph with every row reversed and its first entry twice: canonicalised inside the call
    rows = [ci[rp[v]:rp[v + 1]][::-1] for v in range(n)]
    rows = [np.concatenate([r, r[:1]]) for r in rows]
    u_rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    Un = ctx.upload(u_rp, np.concatenate(rows).astype(np.int32), n)
    try:
        seen = set()
        for what, a, canon in (("uploaded", A, 0), ("wrapped", W, 0), ("from a result", M, 0), ("untidy", Un, 1)):
            seen.add(_check(ctx.betweenness(a, sources), dict(exp, canonicalised=canon), what))
        assert len(seen) == 1
    finally:
        for h in (Un, M, I, W, A):
            h.free()


@pytest.mark.parametrize("name", sorted(B.REFUSED))
def test_path_counts_of_2p63_are_refused(ctx, name):
    L = bspgemm.lib()
    rp, ci, n = B.graph(name)
    level = B.REFUSED[name][1]
    A = ctx.upload(rp, ci, n)
    ok = ctx.upload(*B.graph("layers_2p62"))
    sources = np.array([1, 0], np.int32)                       # (vertex 1, of the first layer, passes)
    try:
        for lanes in B.LANES:
            ctx.set_option("bc_lanes", lanes)
            fixed, bc, info = np.full(n, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(n, -7.25), bspgemm.BcInfo()
            C.memset(C.byref(info), 0x5A, C.sizeof(info))
            st = L.bspgemm_betweenness(ctx._h, A._h, 2, sources.ctypes.data, fixed.ctypes.data, bc.ctypes.data, C.byref(info))
            msg = L.bspgemm_last_error().decode()
            assert st == ERR_OVERFLOW, (st, msg)
            assert "bspgemm_betweenness" in msg and "sources[1]" in msg and "level %d" % level in msg, msg
            assert bytes(info) == bytes(C.sizeof(info)), "info is not zeroed"
            assert (fixed == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and (bc == -7.25).all(), "the outputs were written"
            _check(ctx.betweenness(ok, B.sources_of("layers_2p62")), B.expected("layers_2p62"), "accepted, after " + name)
            # the first layer alone stays under 2^63
            _check(ctx.betweenness(A, [1]), B.model(rp, ci, n, [1]), "source 1 of " + name)
    finally:
        ctx.set_option("bc_lanes", 0)
        ok.free()
        A.free()


def test_multiply_statistics_are_untouched(ctx):
    rp, ci, n = B.graph("rmat11")
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    try:
        before = ctx.stats()
        _check(ctx.betweenness(A, B.sources_of("rmat11")), B.expected("rmat11"), "stats")
        assert ctx.stats() == before and before["rows"] == n
    finally:
        R.free()
        A.free()


def test_errors_leave_a_usable_context(ctx):
    import torch
    L = bspgemm.lib()
    name = "rmat11"
    rp, ci, n = B.graph(name)
    sources, exp = np.ascontiguousarray(B.sources_of(name)), B.expected(name)
    A = ctx.upload(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                              # 10 x n
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)
    bad = []
    for at, col in ((ci.size // 2, n), (ci.size - 1, -1), (0, 1 << 30)):
        c = ci.copy()
        c[at] = col
        d_rp, d_ci = torch.from_numpy(rp.copy()).cuda(), torch.from_numpy(c).cuda()
        bad.append(ctx.wrap_device(n, n, c.size, d_rp.data_ptr(), d_ci.data_ptr(), keep=(d_rp, d_ci)))
    torch.cuda.synchronize()

    def call(a, src):
        src = np.ascontiguousarray(src, np.int32)
        info = bspgemm.BcInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        fixed = np.full(n, 77, np.uint64)
        st = L.bspgemm_betweenness(ctx._h, a._h, src.size, src.ctypes.data, fixed.ctypes.data, None, C.byref(info))
        msg = L.bspgemm_last_error().decode()
        assert st != 0 and bytes(info) == bytes(C.sizeof(info)) and "bspgemm_betweenness" in msg, (st, msg)
        assert (fixed == 77).all(), "the outputs were written"
        return st, msg

    try:
        st, msg = call(rect, sources)
        assert st == ERR_INVALID and "square" in msg, msg
        st, msg = call(foreign, sources)
        assert st == ERR_INVALID and "context" in msg, msg
        for W in bad:
            st, msg = call(W, sources)
            assert st == ERR_INVALID and "column" in msg, msg
            _check(ctx.betweenness(A, sources), exp, "after a bad column")
        for src in ([0, n, 1], [n + 5]):
            st, msg = call(A, src)
            assert st == ERR_INVALID and "source %d" % max(src) in msg and "outside" in msg, msg
        st, msg = call(A, [3, -2])
        assert st == ERR_INVALID and "source -2" in msg, msg
        st, msg = call(A, np.zeros((1 << 31) // n + 1, np.int32))
        assert st == ERR_INVALID and "nsources" in msg, msg
        _check(ctx.betweenness(A, np.zeros(3, np.int32)), B.model(rp, ci, n, [0, 0, 0]), "a source three times")
        R = ctx.multiply(A, A)                                              # the context still multiplies correctly
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        _check(ctx.betweenness(A, sources), exp, "after the errors")
    finally:
        for h in bad:
            h.free()
        foreign.free()
        other.close()
        rect.free()
        A.free()
