"""The graphs of tests/test_gpu_bc_edges.py, checked without a GPU: the constants that tests/bc_ref.py mirrors are the ones in
csrc/betweenness.hip, the graphs and sources of the GPU tests together reach every edge of the hub code ("cell") that
bc_ref.cells knows, every graph reaches the cells it is named for, and twins with a chunk of 16 that the same builders make
reach the same cells and give the naive model's bits.
"""
import os
import re

import numpy as np
import pytest

import bc_ref as B

# every cell, written out: the union over the GPU tests' graphs has to be exactly this
ALL_CELLS = [
    "source is a hub", "source hub of more than 256 records", "two hubs in one level", "hub level with a non-zero chunk offset",
    "hub length chunk + 1", "hub length an exact multiple of the chunk", "hub length otherwise", "hub in the last level",
    "hub with a self-loop", "hub entry to the source", "hub entry to an earlier level", "hub entry to the same level",
    "hub with backward sum 0", "hub reached from two sources in a row", "stored row over the chunk, distinct row not",
    "stored and distinct row over the chunk", "hub successor with sigma > 1 fed from two chunks"]

NAMED_FOR = {
    "hub_levels": ["source is a hub", "two hubs in one level", "hub level with a non-zero chunk offset", "hub length chunk + 1",
                   "hub length an exact multiple of the chunk", "hub length otherwise", "hub in the last level",
                   "hub with a self-loop", "hub entry to the source", "hub entry to an earlier level",
                   "hub entry to the same level", "hub with backward sum 0", "hub reached from two sources in a row",
                   "hub successor with sigma > 1 fed from two chunks"],
    "hub_258_records": ["source is a hub", "source hub of more than 256 records"],
    "stored_5000_of_4000": ["stored row over the chunk, distinct row not"],
    "stored_9000_of_4097": ["stored and distinct row over the chunk", "hub length chunk + 1", "source is a hub"],
}
# the same builders with a chunk of 16: (graph, sources)
TWINS = {
    "hub_levels": lambda: (B.hub_levels(16), B.hub_levels_sources(16)),
    "hub_258_records": lambda: (B.hub((B.THREADS + 1) * 16 + 1), B.EDGE_SOURCES["hub_258_records"]),
    "stored_5000_of_4000": lambda: (B.hub_stored(20, 15), B.EDGE_SOURCES["stored_5000_of_4000"]),
    "stored_9000_of_4097": lambda: (B.hub_stored(35, 17), B.EDGE_SOURCES["stored_9000_of_4097"]),
}


def test_constants_are_the_sources():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "binary-spgemm_amd", "csrc", "betweenness.hip")) as f:
        src = f.read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (const("kBcHubChunk"), const("kBcThreads")) == (B.HUB_CHUNK, B.THREADS) == (4096, 256)
    assert "for (int j = threadIdx.x; j < k && j < chunk_cap; j += kBcThreads) chunk[j] = make_int2(src, j);" in src
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "binary-spgemm_amd", "csrc", "hub_chunks.hpp")) as f:
        hub = f.read()
    assert "return len > CHUNK ? hub_chunks_of<CHUNK>(len) : 0;" in hub     # hub_chunks_over<CHUNK>, which betweenness.hip calls
    assert "hub_chunks_over<kBcHubChunk>(len)" in src
    assert sorted(ALL_CELLS) == sorted(B.CELLS) and len(set(ALL_CELLS)) == len(ALL_CELLS)


def test_the_graphs_reach_every_cell():
    """the graphs of tests/test_gpu_bc_edges.py from their sources, hub_levels also with the sources backwards"""
    seen = set()
    for name in B.EDGE_GRAPHS:
        seen |= B.edge_cells(name)
    seen |= B.cells(*B.graph("hub_levels"), B.EDGE_SOURCES["hub_levels"][::-1])
    assert sorted(seen) == sorted(ALL_CELLS), sorted(set(ALL_CELLS) ^ seen)


@pytest.mark.parametrize("name", sorted(B.EDGE_GRAPHS))
def test_graph_reaches_the_cells_it_is_named_for(name):
    rp, ci, n = B.graph(name)
    assert name not in B.GRAPHS and sorted(NAMED_FOR) == sorted(B.EDGE_GRAPHS) == sorted(B.EDGE_SOURCES)
    got = B.edge_cells(name)
    assert set(NAMED_FOR[name]) <= got, sorted(set(NAMED_FOR[name]) - got)
    assert B.is_canonical(rp, ci, n) == (not name.startswith("stored"))
    if name == "stored_5000_of_4000":                      # not one record: the canonical row fits a group of lanes
        assert got == {"stored row over the chunk, distinct row not"} and B.edge_expected(name)[1]["hub_chunks"] == 0


def test_hub_levels_by_hand():
    """the sweep from vertex 0, level by level: sizes, hubs, chunk offsets, and the counts the library reports"""
    C = B.HUB_CHUNK
    rp, ci, n = B.graph("hub_levels")
    g, p, fresh, X, Y, Z = B.hub_levels_names()
    lens = np.diff(rp)
    assert 18_000 <= n <= 30_000 and n == Z + 1
    assert lens[[1, 2, 3, g, X, Z]].tolist() == [C + 1, 2 * C, C, 2 * C + 1, C + 1, C + 1] and (np.delete(lens, [1, 2, g, X, Z]) <= C).all()
    assert {g, 0, 2, p} <= set(ci[rp[g]:rp[g + 1]].tolist())
    trace = []
    info = B.model(rp, ci, n, [0], trace)
    fronts, level, sigma, delta = (trace[0][k] for k in ("fronts", "level", "sigma", "delta"))
    assert [f.size for f in fronts] == [1, 3, 5 * C // 2, 2, 2 * C - 3, 1]
    assert [level[v] for v in (1, 2, 3, g, p, X, Y, Z)] == [1, 1, 1, 3, 3, 4, 4, 5]
    leaves = 4 + np.arange(5 * C // 2)
    assert sorted(set(sigma[leaves].tolist())) == [1, 2, 3] and sigma[leaves[C]] == 3 and sigma[leaves[C // 2]] == 2
    assert delta[X] == 0 and delta[Z] == 0 and delta[g] > 0 and delta[Y] > 0
    # records: vertices 1 and 2 at offset 0 (2 + 2), g at 4 (3), X at 7 (2), Z at 9 (2); all but Z's are read again backwards
    assert (info["hub_chunks"], info["levels"], info["depth_max"], info["reached"]) == (11 + 9, 6, 5, n)
    # from the first leaf: g alone in level 1, vertices 2 and X in level 2
    trace = []
    B.model(rp, ci, n, [4], trace)
    assert trace[0]["fronts"][1].tolist() == [g] and {2, X} <= set(trace[0]["fronts"][2].tolist())
    # the chunk array never overflows: csrc/betweenness.hip chunk_cap
    assert 11 <= 2 * (ci.size // C) + 2


@pytest.mark.parametrize("name", sorted(TWINS))
def test_twin_reaches_the_same_cells_and_the_naive_bits(name):
    (rp, ci, n), sources = TWINS[name]()
    assert n <= 4200
    assert B.cells(rp, ci, n, sources, chunk=16) == B.edge_cells(name)
    assert B.model(rp, ci, n, sources)["fixed"].tolist() == B.naive(rp, ci, n, sources)
    if name == "hub_levels":
        assert B.model(rp, ci, n, sources[::-1])["fixed"].tolist() == B.naive(rp, ci, n, sources[::-1])
