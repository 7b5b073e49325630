"""The graph algorithms' arrays in the context's workspace (csrc/ws_layout.hpp): one list of arrays per entry point sizes
the workspace and places the pointers, and the pointers are taken again after anything that may have moved it.

What can go wrong is a pointer taken before the workspace moved, or an array sized differently from where it is placed.
Neither shows in a warm context whose workspace is already large, so every case runs three times and the runs are compared
bit for bit -- every output array and the info: (a) the first call of a fresh context, whose workspace grows inside the
call; (b) the same call again, warm; (c) the same call in a context that larger calls have grown past the need.  Where
tests/*_ref.py has a model, (a) is compared with it as well.  The calls and their references are the table of
tests/state_cases.py: every case there that takes any square graph runs here.

The operands have unsorted rows with a repeated entry, so every call that asks for canonical rows canonicalises mid-way (two
transposes in the workspace), and no AT is passed, so the transpose runs inside the call.  n = 1, 3 and 70: 70 is no
multiple of 4 (the padded array lengths differ from n), above 64 (two waves), and vertex 0 has degree 69.
"""
import functools

import pytest

import bspgemm
import gen
import state_cases
from state_cases import SEED

pytestmark = pytest.mark.gpu
SIZES = (1, 3, 70)
CALLS = state_cases.GRAPH_CASES          # every case of the table that takes any square graph (tests/state_cases.py)


@functools.lru_cache(maxsize=None)
def _graph(n):
    """the operands of size n (state_cases.small_graph: vertex 0 of degree n - 1, rows descending with a repeated entry)"""
    return state_cases.graph_ops("layout%d" % n, *state_cases.small_graph(n))


def _run(ctx, name, n):
    g = state_cases.Ops(_graph(n).key, _graph(n).host).upload(ctx)
    try:
        return state_cases.run_case(ctx, name, g)
    finally:
        g.free()


@pytest.fixture(scope="module")
def grown():
    """a context whose workspaces every entry point has already grown, on an untidy graph of 2000 vertices"""
    ctx = bspgemm.Context(0)
    g = state_cases.graph_ops("grown", *gen.dups_unsorted(2000, 8, SEED)).upload(ctx)
    for name in CALLS:
        state_cases.run_case(ctx, name, g)
    g.free()
    yield ctx
    ctx.close()


_same = state_cases.same


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
    state_cases.check_case(name, _graph(n), *cold)
