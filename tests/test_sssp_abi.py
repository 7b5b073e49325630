"""bspgemm_weights_* and bspgemm_sssp without a GPU: the header and the Python view agree, a C99 caller compiles, the calls
refuse by name before anything is dereferenced, and the reference of the GPU tests is right by itself -- the weight hash
against a vector worked out by hand, the numpy round model against the heap Dijkstra and scipy's on every test graph
under delta = 1, 16, the default and 2^64 - 1, the counts of the hand examples, and the default bucket width.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bspgemm
import sssp_ref
from abi_kit import ROOT, ERR_INVALID, FAKE, SENTINEL, header_code, compile_c99, last_error, dirtied

NAME = "bspgemm_sssp"
SYMBOLS = ("bspgemm_weights_upload", "bspgemm_weights_hashed", "bspgemm_weights_download", "bspgemm_weights_nnz",
           "bspgemm_weights_sum", "bspgemm_weights_free", "bspgemm_sssp")
C99_CALLER = """
#include "bspgemm.h"
int main(void)
{
    bspgemm_sssp_params p = {0, 0, 0};
    bspgemm_sssp_info info;
    bspgemm_weights *W = 0;
    uint64_t dist[4];
    int parent[4];
    bspgemm_status st = bspgemm_weights_hashed(0, 0, 7u, 1u, 255u, BSPGEMM_WEIGHTS_SYMMETRIC, &W);
    if (st == BSPGEMM_OK) st = bspgemm_sssp(0, 0, W, 0, &p, dist, parent, &info);
    bspgemm_weights_free(W);
    return (int)st + (int)(bspgemm_weights_sum(W) + (uint64_t)bspgemm_weights_nnz(W)) + BSPGEMM_SSSP_DELTA_C;
}
"""


def test_header_declares_the_handle_the_structs_and_the_constant():
    code = header_code()
    assert "typedef struct bspgemm_weights bspgemm_weights;" in code
    assert "#define BSPGEMM_WEIGHTS_SYMMETRIC 1u" in code
    assert "typedef struct bspgemm_sssp_params { uint64_t delta; int lanes; int reserved; } bspgemm_sssp_params;" in code
    assert ("typedef struct bspgemm_sssp_info { uint64_t delta; uint64_t dist_max; int64_t reached; int64_t entries_walked; "
            "int64_t improved; int64_t hub_chunks; int rounds; int buckets; int lanes; int reserved; } bspgemm_sssp_info;") in code
    assert "#define BSPGEMM_SSSP_DELTA_C %d " % sssp_ref.DELTA_C in code and bspgemm.SSSP_DELTA_C == sssp_ref.DELTA_C
    assert "BSPGEMM_SSSP_TIMING" in open(os.path.join(ROOT, "include", "bspgemm.h")).read()


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in bspgemm.EXPORTS, name
    assert L.bspgemm_weights_sum.restype is C.c_uint64 and L.bspgemm_weights_nnz.restype is C.c_int64
    assert L.bspgemm_weights_free.restype is None
    assert [f for f, _ in bspgemm.SsspInfo._fields_] == list(sssp_ref.INFO)
    assert C.sizeof(bspgemm.SsspInfo) == 64 and C.sizeof(bspgemm.SsspParams) == 16
    assert bspgemm.SsspInfo(delta=2 ** 64 - 1, rounds=3).as_dict() == dict(dict.fromkeys(sssp_ref.INFO, 0), delta=2 ** 64 - 1, rounds=3)
    assert bspgemm.WEIGHTS_SYMMETRIC == 1
    for method in ("weights_upload", "weights_hashed", "sssp"):
        assert callable(getattr(bspgemm.Context, method))
    assert L.bspgemm_weights_nnz(None) == 0 and L.bspgemm_weights_sum(None) == 0
    L.bspgemm_weights_free(None)


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_the_calls_refuse_by_name_before_anything_is_dereferenced():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the refusal comes first
    sentinel, last = SENTINEL, last_error

    def info7():
        return dirtied(bspgemm.SsspInfo, 7)

    dist, parent = np.full(4, 9, np.uint64), np.full(4, 9, np.int32)

    def sssp(ctx, A, W, source, lanes=0):
        info, params = info7(), bspgemm.SsspParams(0, lanes, 0)
        st = L.bspgemm_sssp(ctx, A, W, source, C.byref(params), dist.ctypes.data, parent.ctypes.data, C.byref(info))
        assert st == ERR_INVALID and NAME in last(), last()
        assert bytes(info) == bytes(C.sizeof(info)) and (dist == 9).all() and (parent == 9).all()
        return last()

    for ctx, A, W in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert "NULL" in sssp(ctx, A, W, 0)
    assert "negative source" in sssp(fake, fake, fake, -1)
    for lanes in (1, 8, 32, 65, -4):
        assert "lanes" in sssp(fake, fake, fake, 0, lanes)
    for fn, args in ((L.bspgemm_weights_upload, ()), (L.bspgemm_weights_hashed, (7, 1, 255, 0))):
        for ctx, A in ((None, fake), (fake, None)):
            out = C.c_void_p(sentinel)
            a = (ctx, A, fake) if not args else (ctx, A) + args
            assert fn(*a, C.byref(out)) == ERR_INVALID and not out.value and "NULL" in last(), last()
        a = (fake, fake, fake) if not args else (fake, fake) + args
        assert fn(*a, None) == ERR_INVALID and "NULL" in last()
    out = C.c_void_p(sentinel)
    assert L.bspgemm_weights_hashed(fake, fake, 7, 256, 255, 0, C.byref(out)) == ERR_INVALID
    assert not out.value and "bspgemm_weights_hashed" in last() and "wmin > wmax" in last(), last()
    out = C.c_void_p(sentinel)
    assert L.bspgemm_weights_hashed(fake, fake, 7, 1, 255, 2, C.byref(out)) == ERR_INVALID
    assert not out.value and "flags" in last(), last()
    assert L.bspgemm_weights_download(None, fake, None) == ERR_INVALID and "bspgemm_weights_download" in last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def _mix(x):
    """mix32 in Python integers, written out again"""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_the_weight_hash_on_a_hand_computed_vector():
    # the entries (0, 1), (1, 0), (2, 2), (3, 0), (3, 7)
    rp, ci, n = np.array([0, 1, 2, 3, 5, 5, 5, 5, 5]), np.array([1, 0, 2, 0, 7]), 8
    assert [_mix(x) for x in (0, 1, 2, 0xFFFFFFFF)] == [0, 1753845952, 3507691905, 1734902346]
    assert sssp_ref.weight_hash(rp, ci, n, 7, 1, 255).tolist() == [80, 165, 127, 213, 201]
    assert sssp_ref.weight_hash(rp, ci, n, 7, 1, 255, symmetric=True).tolist() == [80, 80, 127, 73, 201]
    assert sssp_ref.weight_hash(rp, ci, n, 0xdeadbeef, 0, 2 ** 32 - 1).tolist() == [660479691, 3652640880, 2690581637, 3179573431,
                                                                                  2799599230]
    assert sssp_ref.weight_hash(rp, ci, n, 5, 9, 9).tolist() == [9] * 5
    rows = np.repeat(np.arange(n), np.diff(rp))
    for seed, lo, hi in ((7, 1, 255), (1 << 31, 0, 0), (3, 2 ** 32 - 2, 2 ** 32 - 1)):
        want = [lo + _mix(_mix(r ^ seed) ^ c) % (hi - lo + 1) for r, c in zip(rows.tolist(), ci.tolist())]
        assert sssp_ref.weight_hash(rp, ci, n, seed, lo, hi).tolist() == want
    w = sssp_ref.weight_hash(*sssp_ref.rmat(10, True)[:3], 7, 1, 255, True)
    assert w.min() == 1 and w.max() == 255


def test_the_default_bucket_width():
    d = sssp_ref.default_delta
    assert d(0, 0, 5) == 1 and d(10, 10, 100) == 32 and d(9, 10, 100) == 1            # sum / nnz = 0
    assert d(128 * 4380, 4380, 1024) == 32 * 128 // 4 and d(127 * 100 + 99, 100, 7) == 32 * 127 // 14
    assert d(2 ** 32 * 10, 10, 10, c=1) == 2 ** 32


@functools.lru_cache(maxsize=None)
def _graph(name):
    return sssp_ref.GRAPHS[name]()


@pytest.mark.parametrize("name", [g for g in sssp_ref.GRAPHS if g != "settle_stride"])
def test_model_equals_dijkstra_and_scipy(name):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    g = _graph(name)
    dist = sssp_ref.dijkstra(g.rp, g.ci, g.w, g.n, g.source)
    if g.ci.size and (g.w > 0).all():                        # (scipy takes a stored 0 for no edge; float64 is exact below 2^53)
        rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.rp))
        key = rows * g.n + g.ci
        order = np.lexsort((g.w, key))
        sel = order[np.concatenate([[True], key[order][1:] != key[order][:-1]])]     # the smallest of repeated entries
        M = sp.csr_matrix((g.w[sel].astype(np.float64), (rows[sel], g.ci[sel])), shape=(g.n, g.n))
        ref = dijkstra(M, directed=True, indices=g.source)
        assert dist[dist != sssp_ref.NONE].max() < 2 ** 53
        assert np.array_equal(np.isinf(ref), dist == sssp_ref.NONE)
        assert np.array_equal(ref[~np.isinf(ref)], dist[dist != sssp_ref.NONE].astype(np.float64))
    for delta in sssp_ref.DELTAS:
        m = sssp_ref.model(g.rp, g.ci, g.w, g.n, g.source, delta)
        assert np.array_equal(m.dist, dist), (name, delta)
        assert m.reached == int((dist != sssp_ref.NONE).sum()) and m.dist_max == int(dist[dist != sssp_ref.NONE].max())
        assert m.rounds <= 2 * g.n + 2 and 1 <= m.buckets <= m.rounds and m.improved >= m.reached - 1
    par = sssp_ref.parents(g.rp, g.ci, g.w, g.n, g.source, dist)
    assert par[g.source] == g.source and ((par >= 0) == (dist != sssp_ref.NONE)).all()


def test_model_counts_on_the_hand_examples():
    def run(name, delta):
        g = _graph(name)
        return sssp_ref.model(g.rp, g.ci, g.w, g.n, g.source, delta)

    m = run("snap_rule", sssp_ref.INF)                       # b is walked from its settled 5 while a lowers it to 2
    assert m.dist.tolist() == [0, 1, 2, 3, sssp_ref.INF] and (m.rounds, m.buckets, m.entries_walked, m.improved) == (4, 1, 5, 5)
    m = run("snap_rule", 1)                                  # Dijkstra's order: every vertex is lowered to its distance once ...
    assert (m.rounds, m.buckets, m.entries_walked, m.improved) == (4, 4, 4, 4)      # ... but b, which 5 reaches first
    for d in (sssp_ref.CHUNK + 1, 2 * sssp_ref.CHUNK, 2 * sssp_ref.CHUNK + 1):   # the hub is walked in rounds 2 and 3: its records twice
        k = -(-d // sssp_ref.CHUNK)
        assert k == (3 if d > 2 * sssp_ref.CHUNK else 2)
        m = run("hub_twice_%d" % d, sssp_ref.INF)
        assert (m.rounds, m.hub_chunks, m.improved) == (4, 2 * k, 2 * d + 3)
        assert run("hub_twice_%d" % d, 1).hub_chunks == k
    assert run("hub_twice_%d" % sssp_ref.CHUNK, sssp_ref.INF).hub_chunks == 0
    # the near-star's leaves point back at the hub, which is the source: never lowered, so its records are emitted once
    for d, k in ((sssp_ref.CHUNK, 0), (sssp_ref.CHUNK + 1, 2), (2 * sssp_ref.CHUNK, 2), (2 * sssp_ref.CHUNK + 1, 3)):
        assert [run("near_star_%d" % d, delta).hub_chunks for delta in sssp_ref.DELTAS] == [k] * 4
        assert [run("star_%d" % d, delta).hub_chunks for delta in sssp_ref.DELTAS] == [k] * 4
        assert [run("late_star_%d" % d, delta).hub_chunks for delta in sssp_ref.DELTAS] == [k] * 4
    m = run("unit_path300", 1)
    assert (m.rounds, m.buckets) == (300, 300)               # 299 advances
    m = run("unit_path300", sssp_ref.INF)
    assert (m.rounds, m.buckets) == (300, 1)
    m = run("heavy_path", 0)
    assert m.dist.tolist() == [k * (2 ** 32 - 1) for k in range(6)] and m.dist_max > 2 ** 34
    g = _graph("untidy")
    dist = sssp_ref.dijkstra(g.rp, g.ci, g.w, g.n, g.source)
    assert dist.tolist() == [0, 2, 5, 5, 5, 5, 5, sssp_ref.INF, sssp_ref.INF]
    # 3 has a self-loop of 1 and is tight from 2; the zero-length 2-cycle 4 <-> 5 has 4 tight from 3 and 5 from 4
    assert sssp_ref.parents(g.rp, g.ci, g.w, g.n, g.source, dist).tolist() == [0, 0, 1, 2, 3, 4, 2, -1, -1]
    assert [sssp_ref.model_of(_graph(k)).lanes for k in ("rmat10", "dense16", "dense64")] == [4, 16, 64]
    g = _graph("settle_stride")
    assert g.n - 1 > sssp_ref.SETTLE_STRIDE
