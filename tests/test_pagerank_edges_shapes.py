"""The graphs of tests/test_gpu_pagerank_edges.py, checked without a GPU: the constants that tests/pagerank_ref.py mirrors are
the ones in csrc/pagerank.hip, the runs of the GPU tests together reach every kernel edge ("cell") that pagerank_ref.cells
knows, every graph reaches the cells it is named for, and the numpy model equals the naive one on scaled-down twins that the
same builders make.
"""
import numpy as np
import pytest

import pagerank_ref as P

# every cell, written out: the union over the GPU tests' runs has to be exactly this
ALL_CELLS = [
    "init: one trip", "init: second trip", "lane: one trip", "lane: second trip", "wave16: one trip", "wave16: second trip",
    "wave64: one trip", "wave64: second trip", "group: one trip", "group: second trip", "hub_chunk: one trip",
    "hub_chunk: second trip", "finish: one trip", "finish: second trip", "finish_push: one trip", "finish_push: second trip",
    "mass: one trip", "mass: second trip", "wave16: last wave partly idle", "wave64: last workgroup partly idle",
    "hub: in-degree chunk + 1", "hub: in-degree an exact multiple of the chunk", "hub: in-degree of several chunks otherwise",
    "hub: in-degree within one chunk", "hub: in-degree 0", "hubs: two of several chunks", "hub: dangling", "hub: self-loop",
    "lanes: 16", "lanes: 64", "lanes: mean exactly 32", "lanes: mean just above 32", "push: aligned col_idx",
    "push: unaligned col_idx"]

# what each graph is there for, on its natural classes (PR_MIN_CLASS 0) unless a class is named
NAMED_FOR = {
    ("hubs", 0, P.PR_PULL): ["hub: in-degree chunk + 1", "hub: in-degree an exact multiple of the chunk",
                             "hub: in-degree of several chunks otherwise", "hubs: two of several chunks", "hub: dangling",
                             "hub: self-loop", "hub_chunk: one trip", "finish: one trip", "group: one trip"],
    ("hubs", 3, P.PR_PULL): ["hub: in-degree within one chunk", "hub_chunk: second trip", "hubs: two of several chunks"],
    ("wide", 0, P.PR_PULL): ["init: second trip", "lane: second trip", "wave16: second trip", "wave16: last wave partly idle",
                             "mass: second trip", "lanes: 16"],
    ("wide", 2, P.PR_PULL): ["group: second trip"],
    ("wide", 3, P.PR_PULL): ["finish: second trip", "hub_chunk: second trip", "hub: in-degree 0"],
    ("wide", 0, P.PR_PUSH): ["finish_push: second trip", "init: second trip", "mass: second trip"],
    ("wave64", 0, P.PR_PULL): ["wave64: second trip", "wave64: last workgroup partly idle", "lanes: 64", "lane: one trip"],
    ("lanes_at_32", 0, P.PR_PULL): ["lanes: mean exactly 32", "lanes: 16", "wave16: one trip", "wave16: last wave partly idle"],
    ("lanes_above_32", 0, P.PR_PULL): ["lanes: mean just above 32", "lanes: 64", "wave64: one trip"],
}


def test_constants_are_the_sources():
    src = P.source_constants()
    assert src == {k: getattr(P, k) for k in src}
    assert (P.LANE_CAP, P.WAVE_CAP, P.GROUP_CAP, P.HUB_CHUNK, P.THREADS, P.WAVES, P.MAX_BLOCKS, P.LANES_MEAN) == \
        (8, 256, 4096, 4096, 256, 4, 2048, 32)
    assert P.grid(0, 256) == 1 and P.grid(256, 256) == 1 and P.grid(257, 256) == 2 and P.grid(10**7, 256) == 2048
    assert sorted(ALL_CELLS) == sorted(P.CELLS) and len(set(ALL_CELLS)) == len(ALL_CELLS)


def test_the_runs_reach_every_cell():
    """the runs of tests/test_gpu_pagerank_edges.py: every graph under its PR_MIN_CLASS values with PULL, and with PUSH on an
    aligned and on an unaligned col_idx"""
    seen = set()
    for name, classes in P.EDGE_MIN_CLASSES.items():
        rp, ci, n = P.graph(name)
        for min_class in classes:
            seen |= P.cells(rp, ci, n, min_class, P.PR_PULL)
        for shift in (0, 1):
            seen |= P.cells(rp, ci, n, 0, P.PR_PUSH, shift)
    assert sorted(seen) == sorted(ALL_CELLS), sorted(set(ALL_CELLS) ^ seen)


@pytest.mark.parametrize("name,min_class,method", sorted(NAMED_FOR))
def test_graph_reaches_the_cells_it_is_named_for(name, min_class, method):
    assert name in P.EDGE_GRAPHS and min_class in P.EDGE_MIN_CLASSES[name]
    got = P.cells(*P.graph(name), min_class, method)
    assert set(NAMED_FOR[name, min_class, method]) <= got, sorted(set(NAMED_FOR[name, min_class, method]) - got)


def test_edge_graphs_are_small_and_canonical():
    for name in P.EDGE_GRAPHS:
        rp, ci, n = P.graph(name)
        assert P.is_canonical(rp, ci, n) and ci.size <= 500_000 and n <= 560_000, name    # (PUSH reads A as it is stored)
        assert name not in P.GRAPHS


def test_hubs_graph():
    rp, ci, n = P.graph("hubs")
    C = P.HUB_CHUNK
    d, out = P.indegree(rp, ci, n), np.diff(rp)
    assert 13_000 <= n <= 20_000
    assert d[:4].tolist() == [C + 1, 2 * C, 2 * C + 1, 3 * C] and d[4:-1].max() <= P.WAVE_CAP < d[-1] <= P.GROUP_CAP
    assert out[0] == 0 and out[1:4].min() > 0 and 3 in ci[rp[3]:rp[4]]
    assert P.hub_chunks(rp, ci, n) == 2 + 2 + 3 + 3 and P.class_vertices(rp, ci, n)[3] == 4
    # the feeders of every hub have out-degrees from a few (1 at hub 0) to over 300; the chunks' sums of c(u) = q / outdeg(u) differ by
    # more than a factor of 100 (the chunks of a single entry, and the feeders' spread)
    t_rp, t_ci, _ = P.transposed(rp, ci, n)
    q, sums = P.ONE // n, []
    for h in range(4):
        feed = t_ci[t_rp[h]:t_rp[h + 1]]
        deg = out[feed]
        assert deg.min() <= (1 if h == 0 else 4) and deg.max() >= 300, (h, deg.min(), deg.max())
        sums += [int((q // deg[b:b + C].astype(np.uint64)).sum()) for b in range(0, feed.size, C)]
    assert len(sums) == 10 and max(sums) > 100 * min(sums) > 0


def test_wide_graphs():
    rp, ci, n = P.graph("wide")
    size = P.class_vertices(rp, ci, n)
    assert size[0] > P.THREADS * P.MAX_BLOCKS and size[1] > 16 * P.MAX_BLOCKS and size[1] % 4 != 0 and size[2:] == [0, 0]
    assert n > P.THREADS * P.MAX_BLOCKS and P.wave_lanes(rp, ci, n) == 16
    assert 0 < P.pagerank(rp, ci, n, max_iter=0)["dangling"] < n
    dangling = np.diff(rp) == 0                            # in the lane class, and every fifth vertex of the wave class:
    assert dangling[:size[0]].any() and dangling[size[0]::5].all()   # whatever the list's order, every trip holds some
    rp, ci, n = P.graph("wave64")
    size = P.class_vertices(rp, ci, n)
    d = P.indegree(rp, ci, n)
    assert size[1] > P.WAVES * P.MAX_BLOCKS and size[1] % P.WAVES != 0 and size[2:] == [0, 0] and P.wave_lanes(rp, ci, n) == 64
    assert d[d > P.LANE_CAP].sum() > P.LANES_MEAN * size[1]


def test_lanes_boundary_graphs():
    for name, entries, lanes in (("lanes_at_32", 32 * 5, 16), ("lanes_above_32", 32 * 5 + 1, 64)):
        rp, ci, n = P.graph(name)
        d = P.indegree(rp, ci, n)
        assert P.class_vertices(rp, ci, n) == [n - 5, 5, 0, 0] and d[d > P.LANE_CAP].sum() == entries
        assert P.wave_lanes(rp, ci, n) == lanes
    assert P.wave_lanes(*P.graph("lanes_at_32"), 1) == 16 and P.wave_lanes(*P.graph("all_dangling")) == 64


TWINS = {
    "hubs": lambda: P.hubs_graph(16),
    "wide": lambda: P.wide_graph(lane=300, wave=37),
    "wave64": lambda: P.wave64_graph(wave=21, feeders=101),
    "lanes_at_32": lambda: P.lanes_graph(0),
    "lanes_above_32": lambda: P.lanes_graph(1),
}


@pytest.mark.parametrize("name", sorted(TWINS))
def test_model_equals_the_naive_one_on_a_twin(name):
    """the same builder at a size the naive model walks: the same structure (read off naively), the same bits"""
    assert sorted(TWINS) == sorted(P.EDGE_GRAPHS)
    rp, ci, n = TWINS[name]()
    assert n <= 400
    rows = [set(ci[rp[u]:rp[u + 1]].tolist()) for u in range(n)]
    indeg = [sum(v in r for r in rows) for v in range(n)]
    assert indeg == P.indegree(rp, ci, n).tolist()
    if name == "hubs":
        assert indeg[:4] == [17, 32, 33, 48] and not rows[0] and 3 in rows[3] and max(indeg[4:]) <= 16
        assert min(len(rows[u]) for u in range(4, n)) == 1 and max(len(rows[u]) for u in range(4, n)) > 2 * 16
    if name == "wide":
        assert sorted(set(indeg[300:])) == [9, 10] and max(indeg[:300]) <= 8 and any(not r for r in rows)
    if name == "wave64":
        assert set(indeg[101:]) == {40} and max(indeg[:101]) <= 8
    for damping in (0.85, 1.0):
        rs, deltas, _ = P.trajectory(rp, ci, n, damping, 3)
        r, nd, _ = P.naive(rp, ci, n, damping, 3)
        assert rs[-1].tolist() == r and deltas == nd
