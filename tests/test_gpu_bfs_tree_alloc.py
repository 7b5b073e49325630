"""Every branch of bspgemm_bfs_tree that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *tree == NULL, a zeroed info block and a message; the same
call, unarmed, on the same context returns the exact tree; after freeing every handle and destroying the context the gate's
live count and live bytes are back where they were.  The sweep runs twice: with AT == NULL under PULL, so that the
transpose's allocations are inside the call, and with AT given under AUTO.

One request cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's workspace (ensure_tmp), which after an
out-of-memory answer drops the cache of freed results and asks again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The call grows the workspace once, before anything else, so that is k = 1: the armed
call returns BSPGEMM_OK.  The test accepts BSPGEMM_OK from an armed call only at k = 1, only with the exact tree and with
exactly one request more than a cold call makes (the failed one, repeated); every other k must end in BSPGEMM_ERR_ALLOC.
The result's three buffers are asked for once each (csrc/bfs_tree.hip: tree_buffer), so they end in BSPGEMM_ERR_ALLOC too.

A cold call with AT == NULL makes 8 device allocations (measured on an MI355X; the sweep prints it, ALLOCSWEEP): the
workspace, the tile rows of the operand check, the transpose's row_ptr, col_idx and row-length bytes, and the result's
row_ptr, col_idx and values: ERR_ALLOC at k = 2 .. 8, retried at k = 1.  With AT given it makes 4: the transpose that the
test ran beforehand has left a workspace that is large enough, so no k is retried and k = 1 .. 4 end in ERR_ALLOC.  A cold
call that makes more than twice the count fails the test before the sweep (tests/alloc_sweep.py).
"""
import ctypes as C

import pytest

import bfs_tree_ref as ref
import bspgemm
from alloc_sweep import OK, VP, Case, L, call_to_handle, fields, last_error, sweep

pytestmark = pytest.mark.gpu

NAME = "rmat12_directed"
AUTO, PULL = 0, 2


def bfs_tree_case(with_at, direction, cold_expected):
    rp, ci, n, source = ref.graph(NAME)
    model = ref.model(rp, ci, n, source, direction="pull" if direction == PULL else "auto")
    info_keys = sorted(model) + ["transposed", "canonicalised"]

    def setup(env):
        inp = dict(A=env.upload(rp, ci, n), AT=None)
        if with_at:
            inp["AT"] = env.mat(VP())
            assert L().bspgemm_matrix_transpose(env.ctx, inp["A"], C.byref(inp["AT"])) == OK, last_error()
        return inp

    def call(env, inp, tree, info):
        return L().bspgemm_bfs_tree(env.ctx, inp["A"], inp["AT"], source, direction, 0, tree, info)

    def expect():
        exp = ref.expected(NAME)
        assert model["pull_levels"] > 0 and exp[1].size > 1000
        return tuple(exp) + tuple(model[k] for k in sorted(model)) + (int(not with_at), 0)

    def read(env, inp, out):
        return env.result(out.handles["tree"][1], values=True) + fields(out.structs["info"], info_keys)

    return Case("bfs_tree, AT %s" % ("given" if with_at else "NULL"), setup,
                call_to_handle("r", "tree", call, structs={"info": bspgemm.BfsTreeInfo}), read, expect, zeroed=("info",),
                cap=2 * cold_expected, min_failed=lambda cold: cold - 1, max_retried=1, retried_only_at=1, strict_requests=True)


@pytest.mark.parametrize("with_at,direction,cold_expected", [(False, PULL, 8), (True, AUTO, 4)])
def test_every_allocation_failure_of_the_call(with_at, direction, cold_expected):
    sweep(bfs_tree_case(with_at, direction, cold_expected))
