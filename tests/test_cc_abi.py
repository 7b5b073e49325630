"""The device-resident connected components (bspgemm_connected_components) at the ABI level, without a GPU: the header
declares it with the agreed argument list between bspgemm_bfs and bspgemm_closure, the library exports it, the Python view
has it, a C99 caller compiles cleanly, NULL arguments are refused by name -- and the tests' own reference (cc_ref.py)
agrees with a hand example.
"""
import ctypes as C

import numpy as np

import bspgemm
import cc_ref
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, compile_c99, last_error


DECLARATION = ("bspgemm_status bspgemm_connected_components(bspgemm_context *ctx, const bspgemm_matrix *A, "
               "bspgemm_matrix **P, int *ncomponents, int *rounds);")


def test_header_declares_it_between_bfs_and_closure():
    code = header_code()
    assert DECLARATION in code, "include/bspgemm.h does not declare bspgemm_connected_components as agreed"
    assert code.index("bspgemm_bfs(") < code.index("bspgemm_connected_components(") < code.index("bspgemm_closure(")


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, "bspgemm_connected_components"), "bspgemm_connected_components is not exported by libbspgemm.so"
    assert "bspgemm_connected_components" in bspgemm.EXPORTS
    assert len(L.bspgemm_connected_components.argtypes) == 5
    assert callable(getattr(bspgemm.Context, "connected_components", None)), "Context.connected_components"


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the size of the largest component; *count = how many there are */
int largest_component(bspgemm_context *ctx, const bspgemm_matrix *A, int n, int *count)
{
    bspgemm_matrix *P = 0, *members = 0;
    int rounds = 0, largest = 0, c;
    int *row_ptr;
    if (bspgemm_connected_components(ctx, A, &P, count, &rounds) != BSPGEMM_OK) return -1;
    if (bspgemm_matrix_transpose(ctx, P, &members) != BSPGEMM_OK) { bspgemm_matrix_free(P); return -1; }
    row_ptr = malloc(((size_t)n + 1) * sizeof(int));
    if (row_ptr && bspgemm_matrix_download(ctx, members, row_ptr, 0) == BSPGEMM_OK)
        for (c = 0; c < n; c++)
            if (row_ptr[c + 1] - row_ptr[c] > largest) largest = row_ptr[c + 1] - row_ptr[c];
    free(row_ptr);
    bspgemm_matrix_free(members);
    bspgemm_matrix_free(P);
    if (bspgemm_connected_components(ctx, A, &P, 0, 0) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(P);
    return largest;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    for ctx, A in ((None, fake), (fake, None)):
        out, count, rounds = C.c_void_p(sentinel), C.c_int(7), C.c_int(7)
        assert L.bspgemm_connected_components(ctx, A, C.byref(out), C.byref(count), C.byref(rounds)) == ERR_INVALID
        assert not out.value and "bspgemm_connected_components" in last() and "NULL" in last(), last()
    assert L.bspgemm_connected_components(fake, fake, None, None, None) == ERR_INVALID
    assert "bspgemm_connected_components" in last() and "NULL" in last(), last()


# ---------------------------------------------------------------- the reference itself -------------------------------
def test_cc_ref_on_a_hand_example():
    # 3 -> 1 and 1 -> 3 twice, 5 -> 3, 2 -> 6, 6 -> 6, 4 -> 0; 7 alone.  Row 1 is unsorted and repeats an entry.
    rp = np.array([0, 0, 2, 3, 4, 5, 6, 7, 7], np.int32)
    ci = np.array([3, 3, 6, 1, 0, 3, 6], np.int32)
    label, count = cc_ref.labels(rp, ci, 8)
    assert label.dtype == np.int32 and label.tolist() == [0, 1, 2, 1, 0, 1, 2, 7] and count == 4
    m_rp, m_ci = cc_ref.members(label)
    assert m_rp.tolist() == [0, 2, 5, 7, 7, 7, 7, 7, 8] and m_ci.tolist() == [0, 4, 1, 3, 5, 2, 6, 7]
    assert cc_ref.labels(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)[1] == 0
    assert cc_ref.labels(np.zeros(4, np.int32), np.zeros(0, np.int32), 3)[0].tolist() == [0, 1, 2]


def test_builders_have_the_shapes_they_promise():
    for entries in (4095, 4096, 4097, 8195):
        rp, ci, n = cc_ref.short_paths(entries, 5500 + entries)
        label, count = cc_ref.labels(rp, ci, n)
        assert ci.size == entries and n % 4 != 0 and count == n - entries and count > entries // 4
    rp, ci, n = cc_ref.path_permuted(4099, 5410)
    assert ci.size == 4098 and cc_ref.labels(rp, ci, n)[1] == 1 and int(np.diff(rp).max()) == 1
    for hub, stored in ((5000, "hub"), (2500, "hub"), (5000, "leaves")):
        rp, ci, n = cc_ref.star(5001, hub, stored)
        assert ci.size == 5000 and int(np.diff(rp).max()) == (5000 if stored == "hub" else 1)
        assert not cc_ref.labels(rp, ci, n)[0].any()
    rp, ci, n = cc_ref.sparse_far_rows(20000, 250, 12, 5420)
    first = np.searchsorted(rp, 0, side="right") - 1, np.searchsorted(rp, cc_ref.K_SEL_TILE, side="right") - 1
    assert ci.size == 6000 and first[1] - first[0] + 1 > cc_ref.K_SEL_STAGE       # the first tile's window is not staged
    label, count = cc_ref.labels(rp, ci, n)
    assert int((np.bincount(label, minlength=n) == 1).sum()) > n // 2               # isolated vertices: the majority
    for side in ("first", "second"):
        rp, ci, n, (u, v) = cc_ref.two_halves(150, 5430, side)
        assert cc_ref.labels(rp, ci, n)[1] == 1
        row, col = (u, v) if side == "first" else (v, u)
        at = rp[row] + int(np.flatnonzero(ci[rp[row]:rp[row + 1]] == col)[0])
        cut_rp = rp - (np.arange(rp.size) > row)
        assert cc_ref.labels(cut_rp, np.delete(ci, at), n)[1] == 2                  # the one entry joins the halves
        rows = np.repeat(np.arange(n), np.diff(rp))
        assert not ((rows == col) & (ci == row)).any()                              # and is not stored the other way
    rp, ci, n = cc_ref.untidy(300, 5440)
    rows = np.repeat(np.arange(n), np.diff(rp))
    keys = rows.astype(np.int64) * n + ci
    assert (rows == ci).sum() == 60 and np.unique(keys).size < keys.size and cc_ref.labels(rp, ci, n)[1] > 3
    assert any((np.diff(ci[rp[r]:rp[r + 1]]) < 0).any() for r in range(n))          # unsorted rows
