"""bspgemm_betweenness on the GPU at every edge of the hub code of csrc/betweenness.hip: the edge graphs of bc_ref.py
(tests/test_bc_edges_shapes.py proves without a GPU which edges they reach: several hubs in a level, chunk records behind those
of earlier levels, a hub as the source, in the last level, with a sum of 0, with entries that are not one level down, a
source of 258 records, stored rows longer than their distinct entries) give the numpy model's bits and counts, under every
BC_LANES and source order, and under BSPGEMM_BC_TIMING, whose line on stderr carries the model's counts.
"""
import os
import re

import numpy as np
import pytest

import bspgemm
import bc_ref as B

pytestmark = pytest.mark.gpu
INFO = ("sigma_max", "reached", "edges_forward", "hub_chunks", "sources", "depth_max", "levels", "canonicalised")
LINE = re.compile(r"\[bspgemm\] bspgemm_betweenness: n (\d+) nnz (\d+) sources (\d+) reached (\d+) depth (\d+) levels (\d+) "
                  r"hub chunks (\d+) \((\d+) lanes\) \| ")


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def timed():
    """a second context, created under BSPGEMM_BC_TIMING (read once, in bspgemm_create)"""
    os.environ["BSPGEMM_BC_TIMING"] = "1"
    try:
        c = bspgemm.Context(0)
    finally:
        del os.environ["BSPGEMM_BC_TIMING"]
    yield c
    c.close()


def _check(got, exp, what):
    fixed, bc, info = got
    assert fixed.dtype == np.uint64 and np.array_equal(fixed, exp["fixed"]), what
    assert bc.tobytes() == exp["bc"].tobytes(), what
    for k in INFO:
        assert info[k] == exp[k], (what, k, info[k], exp[k])
    return fixed.tobytes()


@pytest.mark.parametrize("name", ["hub_levels", "stored_5000_of_4000", "stored_9000_of_4097"])
def test_equals_the_model_under_every_lanes_and_order(ctx, name):
    rp, ci, n = B.graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for lanes in B.LANES:
            ctx.set_option("bc_lanes", lanes)
            for backwards in (False, True):
                sources, exp = B.edge_expected(name, backwards)
                _check(ctx.betweenness(A, sources), exp, (name, lanes, sources.tolist()))
    finally:
        ctx.set_option("bc_lanes", 0)
        A.free()


def test_hub_levels_source_by_source(ctx):
    """every source alone, and the first-generation hub three times in a row: delta[hub] starts from 0 every time"""
    rp, ci, n = B.graph("hub_levels")
    g, p, fresh, X, Y, Z = B.hub_levels_names()
    A = ctx.upload(rp, ci, n)
    try:
        for sources in ([0], [2], [4], [g], [X], [Z], [2, 2, 2], [g, 1, g]):
            _check(ctx.betweenness(A, sources), B.model(rp, ci, n, sources), sources)
    finally:
        A.free()


def test_source_of_258_chunk_records(ctx):
    """k_bc_source's loop over the records goes round twice; once, under the automatic lanes"""
    name = "hub_258_records"
    rp, ci, n = B.graph(name)
    sources, exp = B.edge_expected(name)
    assert (np.diff(rp)[sources[0]] + B.HUB_CHUNK - 1) // B.HUB_CHUNK == B.THREADS + 2
    A = ctx.upload(rp, ci, n)
    try:
        _check(ctx.betweenness(A, sources), exp, name)
    finally:
        A.free()


def test_timing_mode_gives_the_same_bits_and_reports_the_model(ctx, timed, capfd):
    name = "hub_levels"
    rp, ci, n = B.graph(name)
    A, At = ctx.upload(rp, ci, n), timed.upload(rp, ci, n)
    try:
        for lanes in (0, 64):
            ctx.set_option("bc_lanes", lanes)
            timed.set_option("bc_lanes", lanes)
            for backwards in (False, True):
                sources, exp = B.edge_expected(name, backwards)
                capfd.readouterr()
                plain = _check(ctx.betweenness(A, sources), exp, (name, lanes))
                assert "[bspgemm]" not in capfd.readouterr().err          # an untimed context writes nothing
                got = timed.betweenness(At, sources)
                lines = [ln for ln in capfd.readouterr().err.splitlines() if "bspgemm_betweenness:" in ln]
                assert len(lines) == 1, lines
                assert _check(got, exp, (name, lanes, "timed")) == plain
                m = LINE.search(lines[0])
                assert m, lines[0]
                assert [int(x) for x in m.groups()] == [n, ci.size, sources.size, exp["reached"], exp["depth_max"], exp["levels"],
                                                        exp["hub_chunks"], lanes], lines[0]
    finally:
        ctx.set_option("bc_lanes", 0)
        timed.set_option("bc_lanes", 0)
        At.free()
        A.free()
    assert "BSPGEMM_BC_TIMING" not in os.environ
