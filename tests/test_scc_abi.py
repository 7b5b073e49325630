"""The device-resident strongly connected components (bspgemm_strongly_connected_components) at the ABI level, without a
GPU: the header declares it with the agreed argument list between bspgemm_kcore and bspgemm_closure, the library exports
it, the Python view has it, a C99 caller compiles cleanly, NULL arguments are refused by name -- and the tests' own
reference (scc_ref.py) agrees with a hand example, and its builders have the properties the GPU tests rely on.
"""
import ctypes as C

import numpy as np

import bspgemm
import cc_ref
import scc_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, header_text, compile_c99, last_error

NAME = "bspgemm_strongly_connected_components"

DECLARATION = ("bspgemm_status bspgemm_strongly_connected_components(bspgemm_context *ctx, const bspgemm_matrix *A, "
               "bspgemm_matrix **P, int *ncomponents, int *rounds, int *sweeps);")


def test_header_declares_it_between_kcore_and_closure():
    code = header_code()
    assert DECLARATION in code, "include/bspgemm.h does not declare %s as agreed" % NAME
    assert code.index("bspgemm_kcore(") < code.index(NAME + "(") < code.index("bspgemm_closure(")
    assert "bspgemm_readCOO" in header_text().split(NAME + "(")[0].rsplit("/*", 1)[1]    # the transposition remark


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, NAME), "%s is not exported by libbspgemm.so" % NAME
    assert NAME in bspgemm.EXPORTS
    assert len(getattr(L, NAME).argtypes) == 6
    assert callable(getattr(bspgemm.Context, "strongly_connected_components", None)), "Context.strongly_connected_components"


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the size of the largest strongly connected component; *count = how many there are */
int largest_component(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int *count)
{
    bspgemm_matrix *P = 0, *members = 0;
    int rounds = 0, sweeps = 0, largest = 0, c;
    int *row_ptr;
    if (bspgemm_strongly_connected_components(ctx, A, &P, count, &rounds, &sweeps) != BSPGEMM_OK) return -1;
    if (bspgemm_matrix_transpose(ctx, P, &members) != BSPGEMM_OK) { bspgemm_matrix_free(P); return -1; }
    row_ptr = malloc(((size_t)n + 1) * sizeof(int));
    if (row_ptr && bspgemm_matrix_download(ctx, members, row_ptr, 0) == BSPGEMM_OK)
        for (c = 0; c < n; c++)
            if (row_ptr[c + 1] - row_ptr[c] > largest) largest = row_ptr[c + 1] - row_ptr[c];
    free(row_ptr);
    bspgemm_matrix_free(members);
    bspgemm_matrix_free(P);
    if (bspgemm_strongly_connected_components(ctx, A, &P, 0, 0, 0) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(P);
    return largest + (rounds > sweeps);
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fn = getattr(L, NAME)
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    for ctx, A in ((None, fake), (fake, None)):
        out, count, rounds, sweeps = C.c_void_p(sentinel), C.c_int(7), C.c_int(7), C.c_int(7)
        assert fn(ctx, A, C.byref(out), C.byref(count), C.byref(rounds), C.byref(sweeps)) == ERR_INVALID
        assert not out.value and NAME in last() and "NULL" in last(), last()
        assert (count.value, rounds.value, sweeps.value) == (0, 0, 0)
    assert fn(fake, fake, None, None, None, None) == ERR_INVALID
    assert NAME in last() and "NULL" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def test_scc_ref_on_a_hand_example():
    # 0 -> 1 -> 2 -> 0 (row 1 repeats its entry), 2 -> 3, 3 -> 4 and 4 -> 3 (row 4 unsorted: 6, 3), 4 -> 6, 5 -> 5, 7 alone
    rp = np.array([0, 1, 3, 5, 6, 8, 9, 9, 9], np.int32)
    ci = np.array([1, 2, 2, 3, 0, 4, 6, 3, 5], np.int32)
    label, count = scc_ref.labels(rp, ci, 8)
    assert label.dtype == np.int32 and label.tolist() == [0, 0, 0, 3, 3, 5, 6, 7] and count == 5
    assert scc_ref.largest(label) == 3
    m_rp, m_ci = scc_ref.members(label)
    assert m_rp.tolist() == [0, 3, 3, 3, 5, 5, 6, 7, 8] and m_ci.tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    t_rp, t_ci, _ = scc_ref.transposed(rp, ci, 8)
    assert t_rp.tolist() == [0, 1, 2, 4, 6, 7, 8, 9, 9] and t_ci.tolist() == [2, 0, 1, 1, 2, 4, 3, 5, 4]
    assert np.array_equal(scc_ref.labels(t_rp, t_ci, 8)[0], label)      # a graph and its transpose: the same components
    assert scc_ref.labels(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)[1] == 0
    assert scc_ref.labels(np.zeros(4, np.int32), np.zeros(0, np.int32), 3)[0].tolist() == [0, 1, 2]


def _shape(g):
    """(entries, components, largest component) of a builder's graph"""
    rp, ci, n = g[:3]
    label, count = scc_ref.labels(rp, ci, n)
    return ci.size, count, scc_ref.largest(label)


def test_builders_have_the_shapes_they_promise():
    assert _shape(scc_ref.cycle(200)) == (200, 1, 200) == _shape(scc_ref.cycle_reversed(200))
    rp, ci, n = scc_ref.cycle_reversed(200)
    assert ci[0] == 199 and np.array_equal(ci[1:], np.arange(199))
    assert _shape(scc_ref.path(200)) == (199, 200, 1) and _shape(scc_ref.path_permuted(4099, 5410)) == (4098, 4099, 1)
    for entry in ("down", "up"):
        rp, ci, n = scc_ref.two_cycles(50, entry)
        assert _shape((rp, ci, n)) == (101, 2, 50) and np.array_equal(scc_ref.labels(rp, ci, n)[0], np.arange(100) // 50 * 50)
        u = int(np.flatnonzero(np.diff(rp) == 2)[0])                        # the one row with two entries holds the joint
        assert (u < 50) == (entry == "down") and (ci[rp[u]:rp[u + 1]] // 50 != u // 50).sum() == 1
        rp, ci, n = scc_ref.ladder(100, entry)
        assert _shape((rp, ci, n)) == (299, 100, 2) and np.array_equal(scc_ref.labels(rp, ci, n)[0], np.arange(200) // 2 * 2)
        rows = np.repeat(np.arange(n), np.diff(rp))
        cross = rows // 2 != ci // 2
        assert cross.sum() == 99 and ((ci[cross] > rows[cross]) == (entry == "down")).all()
    rp, ci, n = scc_ref.tails()
    label, count = scc_ref.labels(rp, ci, n)
    assert (n, ci.size, count, scc_ref.largest(label)) == (71, 72, 42, 30)
    assert ci[rp[70]:rp[71]].tolist() == [70] and (ci == 70).sum() == 2      # a self-loop and one in-edge, nothing else
    for entries in (4095, 4096, 4097, 8195):
        rp, ci, n, lengths = scc_ref.four_cycles(entries, 5600 + entries)
        label, count = scc_ref.labels(rp, ci, n)
        assert ci.size == entries and n % 4 != 0 and min(lengths) >= 2 and not (np.repeat(np.arange(n), np.diff(rp)) == ci).any()
        assert count == len(lengths) + n - entries and np.array_equal(np.sort(np.bincount(label)[np.bincount(label) > 1]),
                                                                      np.sort(lengths))
    for hub in (5000, 2500):
        rp, ci, n = scc_ref.star(5001, hub, "hub")                           # out-edges only: a DAG
        assert _shape((rp, ci, n)) == (5000, 5001, 1) and int(np.diff(rp).max()) == 5000 > scc_ref.K_SEL_TILE
        rp, ci, n = scc_ref.star_both(5001, hub)
        assert _shape((rp, ci, n)) == (10000, 1, 5001) and int(np.diff(rp).max()) == 5000
    rp, ci, n = scc_ref.sparse_far_rows(20000, 250, 12, 5420)
    first = np.searchsorted(rp, 0, side="right") - 1, np.searchsorted(rp, scc_ref.K_SEL_TILE, side="right") - 1
    assert ci.size == 6000 and first[1] - first[0] + 1 > scc_ref.K_SEL_STAGE   # the first tile's window is not staged
    rp, ci, n = scc_ref.untidy(300, 5440)
    rows = np.repeat(np.arange(n), np.diff(rp))
    keys = rows.astype(np.int64) * n + ci
    label, count = scc_ref.labels(rp, ci, n)
    assert (rows == ci).sum() >= 60 and np.unique(keys).size < keys.size and scc_ref.largest(label) >= 10 and count > 10
    assert any((np.diff(ci[rp[r]:rp[r + 1]]) < 0).any() for r in range(n))   # unsorted rows
    assert _shape(cc_ref.untidy(300, 5440))[1:] == (300, 1)                  # the weak components' untidy graph: singletons
    for n in (257, 1023, 4099):
        rp, ci, _ = scc_ref.three_cycles(n)
        label, count = scc_ref.labels(rp, ci, n)
        assert n % 4 and n % 64 and n % 256 and ci.size == n
        assert count == 3 and np.array_equal(label, np.arange(n) % 3)
