"""The device-resident shortest paths (bspgemm_weights_*, bspgemm_sssp): the distances and the parents against the heap
Dijkstra and the tight-predecessor pass of sssp_ref.py, and every field of the info against its numpy round model, bit for
bit, under delta = 1, 16, the default and 2^64 - 1 and under lanes 0, 4, 16 and 64.

What can go wrong is the round: the lane stride and its tail (rows of 0 .. 257 entries, W x (steps in flight) +- 1 among
them), the chunk boundaries of a hub (a centre of 4096, 4097, 8192, 8193 entries as the source, reached late, and lowered
twice so that its records are emitted again), a near vertex lowered by another one of the same round (the counters must
not depend on who saw it), repeated entries, self-loops, zero-length edges and cycles, distances past 2^32, long runs of
tiny rounds and of advances (the path), and more candidates in a round than the settle grid covers in one stride.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bspgemm
import sssp_ref
from sssp_ref import INF

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
NAME = "bspgemm_sssp"


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = sssp_ref.GRAPHS[name]()
    for a in (g.rp, g.ci, g.w):
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(dist, parent) by the definition; computed once and read-only"""
    dist, parent = sssp_ref.reference_of(_graph(name))
    dist.setflags(write=False)
    parent.setflags(write=False)
    return dist, parent


@functools.lru_cache(maxsize=None)
def _expected(name, delta):
    """the model's Sssp; computed once and read-only"""
    m = sssp_ref.model_of(_graph(name), delta)
    assert np.array_equal(m.dist, _reference(name)[0]), (name, delta)
    return m


def _on_device(ctx, g):
    A = ctx.upload(g.rp, g.ci, g.n)
    return A, ctx.weights_upload(A, g.w)


def _check(ctx, A, W, name, delta=0, lanes=0, parents=True):
    g, want, (dist, parent) = _graph(name), _expected(name, delta), _reference(name)
    got_dist, got_parent, info = ctx.sssp(A, W, g.source, delta=delta, lanes=lanes, parents=parents)
    what = (name, delta, lanes)
    assert got_dist.dtype == np.uint64 and np.array_equal(got_dist, dist), (what, np.flatnonzero(got_dist != dist)[:8])
    if parents:
        assert got_parent.dtype == np.int32 and np.array_equal(got_parent, parent), (what, np.flatnonzero(got_parent != parent)[:8])
    else:
        assert got_parent is None
    want = want._replace(lanes=lanes or want.lanes)
    for k in sssp_ref.INFO:
        assert info[k] == getattr(want, k), (what, k, info[k], getattr(want, k))
    return info


def _sweep(ctx, name, deltas=sssp_ref.DELTAS, lanes=sssp_ref.LANES):
    A, W = _on_device(ctx, _graph(name))
    try:
        for delta in deltas:
            for w in lanes:
                _check(ctx, A, W, name, delta, w)
        _check(ctx, A, W, name, deltas[-1], parents=False)
    finally:
        W.free()
        A.free()


# ---------------------------------------------------------------- 1. the small graphs -----------------------------------
@pytest.mark.parametrize("name", list(sssp_ref.SMALL))
def test_small_graphs_under_every_delta_and_lanes(ctx, name):
    _sweep(ctx, name)


def test_the_small_graphs_are_what_they_are_built_for():
    m = _expected("snap_rule", INF)                          # the snap rule: c is lowered twice, from b's settled 5 first
    assert (m.rounds, m.improved, m.entries_walked) == (4, 5, 5)
    dist, parent = _reference("untidy")
    assert dist.tolist() == [0, 2, 5, 5, 5, 5, 5, INF, INF] and parent.tolist() == [0, 0, 1, 2, 3, 4, 2, -1, -1]
    assert _reference("heavy_path")[0][-1] == 5 * (2 ** 32 - 1)
    assert [_expected(k, 0).lanes for k in ("row_lengths", "dense16", "dense64")] == [4, 16, 64]
    g = _graph("row_lengths")                                # every listed length is the row of a reached vertex
    assert (np.diff(g.rp)[: len(sssp_ref.ROW_LENGTHS)] == sssp_ref.ROW_LENGTHS).all()
    assert (_reference("row_lengths")[0][: len(sssp_ref.ROW_LENGTHS)] != sssp_ref.NONE).all()
    assert {4 * sssp_ref.DEEP - 1, 16 * sssp_ref.DEEP + 1, 64 * sssp_ref.DEEP - 1, 64 * sssp_ref.DEEP + 1} <= set(sssp_ref.ROW_LENGTHS)


def test_no_vertices(ctx):
    A = ctx.upload(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)
    W = ctx.weights_upload(A, np.zeros(0, np.uint32))
    try:
        dist, parent, info = ctx.sssp(A, W, 0, parents=True)
        assert dist.size == 0 and parent.size == 0 and not any(info.values())
        assert (W.nnz, W.sum) == (0, 0) and W.download().size == 0
    finally:
        W.free()
        A.free()


# ---------------------------------------------------------------- 2. the hub chunks ------------------------------------
@pytest.mark.parametrize("name", list(sssp_ref.HUB_GRAPHS))
def test_hub_chunks(ctx, name):
    d = int(name.rsplit("_", 1)[1])
    k = -(-d // sssp_ref.CHUNK) if d > sssp_ref.CHUNK else 0
    if name.startswith("hub_twice"):                         # walked in rounds 2 and 3 of the one bucket: the records twice
        assert _expected(name, INF).hub_chunks == 2 * k and _expected(name, 1).hub_chunks == k
    elif name.startswith(("star", "late_star")):
        assert [_expected(name, delta).hub_chunks for delta in sssp_ref.DELTAS] == [k] * 4
    else:                                                    # near-stars: the hub is the source and is never lowered again
        assert [_expected(name, delta).hub_chunks for delta in sssp_ref.DELTAS] == [k] * 4
    _sweep(ctx, name)


# ---------------------------------------------------------------- 3. many rounds, many advances --------------------------
def test_path_of_300_twice(ctx):
    assert (_expected("unit_path300", 1).rounds, _expected("unit_path300", 1).buckets) == (300, 300)
    assert (_expected("unit_path300", INF).rounds, _expected("unit_path300", INF).buckets) == (300, 1)
    A, W = _on_device(ctx, _graph("unit_path300"))
    try:
        for _ in range(2):                                   # the repeat: the workspace is the first run's
            for delta in sssp_ref.DELTAS:
                for lanes in sssp_ref.LANES:
                    _check(ctx, A, W, "unit_path300", delta, lanes)
    finally:
        W.free()
        A.free()


@pytest.mark.parametrize("name", list(sssp_ref.RMAT_GRAPHS))
def test_rmat_with_hashed_weights(ctx, name):
    g = _graph(name)
    symmetric = name.endswith("_sym")
    A = ctx.upload(g.rp, g.ci, g.n)
    W = ctx.weights_hashed(A, 7, 1, 255, symmetric=symmetric)
    try:
        assert np.array_equal(W.download(), g.w) and W.sum == int(g.w.sum(dtype=np.uint64)) and W.nnz == g.ci.size
        assert _expected(name, 1).rounds > 200 and _expected(name, INF).buckets == 1
        for delta in sssp_ref.DELTAS:
            for lanes in sssp_ref.LANES:
                _check(ctx, A, W, name, delta, lanes)
    finally:
        W.free()
        A.free()


def test_more_candidates_than_one_stride_of_the_settle(ctx):
    assert _expected("settle_stride", INF).improved > sssp_ref.SETTLE_STRIDE and _expected("settle_stride", INF).rounds == 2
    _sweep(ctx, "settle_stride")


# ---------------------------------------------------------------- 4. the weights ---------------------------------------
def test_weights_round_trip_hash_and_sum(ctx):
    g = _graph("rmat10_sym")
    A = ctx.upload(g.rp, g.ci, g.n)
    made = []
    try:
        big = np.full(g.ci.size, 2 ** 32 - 1, np.uint32)
        big[::3] = 0
        for w in (g.w, big):
            W = ctx.weights_upload(A, w)
            made.append(W)
            assert np.array_equal(W.download(), w) and W.sum == int(w.sum(dtype=np.uint64)) and W.nnz == w.size
        assert made[1].sum > 2 ** 44
        for seed, lo, hi, sym in ((7, 1, 255, False), (7, 1, 255, True), (0xdeadbeef, 0, 2 ** 32 - 1, False), (3, 9, 9, True),
                                  (2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 1, True)):
            W = ctx.weights_hashed(A, seed, lo, hi, symmetric=sym)
            made.append(W)
            want = sssp_ref.weight_hash(g.rp, g.ci, g.n, seed, lo, hi, sym)
            assert np.array_equal(W.download(), want), (seed, lo, hi, sym)
            assert W.sum == int(want.sum(dtype=np.uint64)) and W.nnz == want.size
        with pytest.raises(ValueError):
            ctx.weights_upload(A, g.w[:-1])
    finally:
        for W in made:
            W.free()
        A.free()


# ---------------------------------------------------------------- 5. errors --------------------------------------------
def test_errors_leave_the_outputs_and_a_usable_context(ctx):
    import torch
    L = bspgemm.lib()
    g = _graph("rmat10")
    n = g.n
    A, W = _on_device(ctx, g)
    twin = ctx.upload(g.rp, g.ci, n)                                    # the same graph, another operand
    rect = ctx.upload(g.rp[:11], g.ci[:g.rp[10]], n)                    # 10 x n
    rect_w = ctx.weights_upload(rect, g.w[:g.rp[10]])
    other = bspgemm.Context(0)
    foreign = other.upload(g.rp, g.ci, n)
    foreign_w = other.weights_upload(foreign, g.w)
    trp = torch.from_numpy(np.array(g.rp)).cuda()
    wrapped = []
    for at, col in ((g.ci.size // 2, n), (g.ci.size - 1, -1), (0, 2 ** 31 - 1)):   # checked on the device before it indexes
        c = np.array(g.ci)
        c[at] = col
        tci = torch.from_numpy(c).cuda()
        m = ctx.wrap_device(n, n, c.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, tci))
        wrapped.append((m, ctx.weights_upload(m, g.w)))
    torch.cuda.synchronize()

    def call(a, w, source=g.source, lanes=0, c=ctx):
        info, params = bspgemm.SsspInfo(), bspgemm.SsspParams(0, lanes, 0)
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        dist, parent = np.full(n, 9, np.uint64), np.full(n, 9, np.int32)
        st = L.bspgemm_sssp(c._h, a._h, w._h, source, C.byref(params), dist.ctypes.data, parent.ctypes.data, C.byref(info))
        untouched = bytes(info) == bytes(C.sizeof(info)) and (dist == 9).all() and (parent == 9).all()
        return st, L.bspgemm_last_error().decode(), untouched

    try:
        for args, cause in (((rect, rect_w), "square"), ((foreign, W), "context"), ((A, foreign_w), "another context"),
                            ((twin, W), "not made for this operand"), ((A, W, n), "source %d outside [0, %d)" % (n, n)),
                            ((A, W, 2 ** 31 - 1), "outside"), ((A, W, -1), "negative source"), ((A, W, 0, 8), "lanes")):
            st, msg, untouched = call(*args)
            assert st == ERR_INVALID and NAME in msg and cause in msg and untouched, (cause, st, msg)
            _check(ctx, A, W, "rmat10")                                # the context is as usable as before
        for m, w in wrapped:
            st, msg, untouched = call(m, w)
            assert st == ERR_INVALID and NAME in msg and "column index outside [0, %d)" % n in msg and untouched, (st, msg)
            _check(ctx, A, W, "rmat10", INF, 16)
    finally:
        for m, w in wrapped:
            w.free()
            m.free()
        for h in (foreign_w, foreign, rect_w, rect, twin, W, A):
            h.free()
        other.close()
