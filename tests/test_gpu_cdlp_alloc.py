"""Every branch of bspgemm_label_propagation that follows a failed device allocation, taken one at a time through
bspgemm_debug_fail_alloc: in a fresh context the k-th device allocation of the call fails, k = 1, 2, ... until the hook no
longer fires.  An armed call returns BSPGEMM_ERR_ALLOC with *P == NULL, a zeroed info and a message; the same call, unarmed,
on the same context returns the exact labels; after freeing every handle and destroying the context the gate's live count
and live bytes are back where they were.

The graph is a star of 5000 leaves: its hub is longer than a workgroup's row (cdlp_ref.GROUP_CAP), so the call needs a hub
table, and in a fresh context the growth of the values workspace that holds it is one of the requests.

Two requests cannot end in BSPGEMM_ERR_ALLOC under a one-shot hook: the context's two workspaces (ensure_tmp: the call's
state and the symmetrize's scratch, grown once before anything else; ensure_tmpv: the hub tables), which after an
out-of-memory answer drop the cache of freed results and ask again -- "a new request, which may succeed", as
include/bspgemm.h says of the hook.  The test accepts BSPGEMM_OK from an armed call only with the exact labels and with
exactly one request more than a cold call makes (the failed one, repeated), and from at most two k; every other k must end
in BSPGEMM_ERR_ALLOC.

A cold call makes 15 device allocations (measured on an MI355X: the retries were k = 1 and k = 14): the workspace's request,
the ten of bspgemm_matrix_symmetrize (the tile rows of the context and three arrays each for the select's, the transpose's
and the union's operand), P.row_ptr and P.col_idx, the hub tables and the row-length bytes of P; the sweep prints the count
(ALLOCSWEEP), and a cold call that makes more than CAP fails the test before it (tests/alloc_sweep.py).
"""
import numpy as np
import pytest

import bspgemm
import cdlp_ref
from alloc_sweep import Case, L, call_to_handle, fields, sweep

pytestmark = pytest.mark.gpu

CAP = 40
MAX_ITER = 3
INFO = ("iterations", "converged", "changed", "communities")


def cdlp_case():
    rp, ci, n = cdlp_ref.GRAPHS["star_hub_last"]()
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)

    def call(env, inp, P, info):
        return L().bspgemm_label_propagation(env.ctx, inp["A"], None, MAX_ITER, P, info)

    def expect():
        e_labels, e_iterations, e_converged, e_changed, e_communities = cdlp_ref.label_propagation(rp, ci, n, MAX_ITER)
        e_classes = cdlp_ref.class_vertices(rp, ci, n)
        assert e_classes == [n - 1, 0, 0, 1] and (e_iterations, e_converged, e_changed) == (MAX_ITER, 0, n)
        return np.arange(n + 1), e_labels, e_iterations, e_converged, e_changed, e_communities, e_classes

    def read(env, inp, out):
        info = out.structs["info"]
        return env.matrix(out.handles["P"][1]) + fields(info, INFO) + (list(info.class_vertices),)   # a hub: the call needed a table

    return Case("label_propagation", lambda env: dict(A=env.upload(rp, ci, n)),
                call_to_handle("m", "P", call, structs={"info": bspgemm.LpInfo}), read, expect, zeroed=("info",),
                cap=CAP, min_failed=lambda cold: cold - 2, max_retried=2, strict_requests=True)


def test_every_allocation_failure_of_the_call():
    sweep(cdlp_case())
