"""The kernel edges of the operand transpose (csrc/transpose.hip), each at the smallest shape that holds it: the vector
and scalar tails of load_items and an exact tile end (the entry counts), the largest staged row_ptr window of
k_tr_scatter<true> and the first two unstaged ones (alone, with empty rows around, and behind a staged tile), no digit
bit at all and one, three passes whose keys differ in one digit only, runs of equal pairs that straddle a thread, a wave
and a tile of the dedup kernels, threads and tiles that keep nothing, every length of a run of empty AT rows around the
narrow / wide switch of fill_rows (leading, inner, trailing, several wide ones in one wave, one across a tile seam), and
a hub column through three tiles.

Every case is compared completely -- rows, cols, nnz, row_ptr, col_idx -- with tests/transpose_ref.py, then transposed
a second time and compared with the canonical form of the input.  All of it is integer and bit for bit.
tests/test_transpose_shapes.py proves without a GPU that every case holds the edge it is named for.
"""
import numpy as np
import pytest

import bspgemm
import transpose_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _same(M, shape, exp, what):
    """every difference in one message: the shape and nnz, row_ptr, col_idx"""
    e_rp, e_ci = exp
    bad = []
    if (M.rows, M.cols, M.nnz) != shape + (e_ci.size,):
        bad.append("%d x %d with %d entries, expected %d x %d with %d" % ((M.rows, M.cols, M.nnz) + shape + (e_ci.size,)))
    for name, g, e in zip(("row_ptr", "col_idx"), M.download(), exp):
        if g.shape != e.shape:
            bad.append("%s has %d entries, expected %d" % (name, g.size, e.size))
        elif not np.array_equal(g, e):
            k = int(np.flatnonzero(g != e)[0])
            bad.append("%s differs first at %d: got %d, expected %d (%d differ)" % (name, k, g[k], e[k], int((g != e).sum())))
    assert not bad, "%s: %s" % (what, "; ".join(bad))


@pytest.mark.parametrize("name", list(T.TRANSPOSE_CASES))
def test_transpose_edge(ctx, name):
    c = T.transpose_case(name)
    e_at, e_canon = T.transpose_expected(name)
    A = ctx.upload(c["rp"], c["ci"], c["cols"])
    AT = ATT = None
    try:
        AT = ctx.transpose(A)
        _same(AT, (c["cols"], c["rows"]), e_at, name + ": AT")
        ATT = ctx.transpose(AT)
        _same(ATT, (c["rows"], c["cols"]), e_canon, name + ": (AT)T")
    finally:
        for h in (ATT, AT, A):
            if h is not None:
                h.free()
