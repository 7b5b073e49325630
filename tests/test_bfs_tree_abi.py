"""The single-source BFS tree (bspgemm_bfs_tree, bspgemm_bfs_direction, bspgemm_bfs_tree_info, the three BFS options) at
the ABI level, without a GPU: the header declares them with the agreed argument list between bspgemm_bfs and
bspgemm_connected_components, the library exports the function, the Python view has it, a C99 caller compiles cleanly, NULL
arguments are refused by name -- and the tests' own reference (bfs_tree_ref.py) agrees with scipy's shortest paths on every
named graph, passes the tree check and a hand example with two candidate parents, the graph builders have the shapes they
promise, and the host model of the direction rule really changes direction twice on one of them.
"""
import ctypes as C
import re

import numpy as np
import pytest

import bfs_ref
import bfs_tree_ref as ref
import bspgemm
from abi_kit import ERR_INVALID, FAKE, SENTINEL, header_code, header_text, compile_c99, last_error, dirtied


DECLARATION = ("bspgemm_status bspgemm_bfs_tree(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT, "
               "int source, bspgemm_bfs_direction direction, int max_depth, bspgemm_result **tree, "
               "bspgemm_bfs_tree_info *info);")
ENUM = ("typedef enum bspgemm_bfs_direction { BSPGEMM_BFS_AUTO = 0, BSPGEMM_BFS_PUSH = 1, BSPGEMM_BFS_PULL = 2 } "
        "bspgemm_bfs_direction;")
STRUCT = ("typedef struct bspgemm_bfs_tree_info { int64_t reached; int64_t edges_pushed; uint64_t pull_mask; int depth; "
          "int complete; int push_levels, pull_levels; int transposed; int canonicalised; } bspgemm_bfs_tree_info;")


def test_header_declares_them_between_bfs_and_components():
    code = header_code()
    for what in (DECLARATION, ENUM, STRUCT):
        assert what in code, "include/bspgemm.h does not declare as agreed: %s" % what
    assert code.index("bspgemm_bfs(") < code.index(ENUM) < code.index(STRUCT) < code.index("bspgemm_bfs_tree(")
    assert code.index("bspgemm_bfs_tree(") < code.index("bspgemm_connected_components(")
    for name, value in (("BFS_ALPHA", 8), ("BFS_BETA", 9), ("BFS_PUSH_LANES", 10)):
        assert re.search(r"BSPGEMM_OPT_%s\s*=\s*%d\b" % (name, value), code), name
    text = header_text()
    for word in ("bit for bit", "m_f * alpha > m_u", "n_f * beta < n", "BSPGEMM_BFS_TREE_TIMING"):
        assert word in text, word


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    assert hasattr(L, "bspgemm_bfs_tree"), "bspgemm_bfs_tree is not exported by libbspgemm.so"
    assert "bspgemm_bfs_tree" in bspgemm.EXPORTS
    assert len(L.bspgemm_bfs_tree.argtypes) == 8
    assert (bspgemm.OPTIONS["bfs_alpha"], bspgemm.OPTIONS["bfs_beta"], bspgemm.OPTIONS["bfs_push_lanes"]) == (8, 9, 10)
    assert callable(getattr(bspgemm.Context, "bfs_tree", None)), "Context.bfs_tree"
    assert C.sizeof(bspgemm.BfsTreeInfo) == 48


C99_CALLER = r"""
#include <stdlib.h>
#include "bspgemm.h"
/* the children lists of the BFS tree from `source`; *depth = its height, or -1 */
bspgemm_matrix *children(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *AT, int n, int source, int *depth)
{
    bspgemm_result *tree = 0;
    bspgemm_matrix *up = 0, *down = 0;
    bspgemm_bfs_tree_info info;
    *depth = -1;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_BFS_ALPHA, 15) != BSPGEMM_OK) return 0;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_BFS_BETA, 18) != BSPGEMM_OK) return 0;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_BFS_PUSH_LANES, 0) != BSPGEMM_OK) return 0;
    if (bspgemm_bfs_tree(ctx, A, AT, source, BSPGEMM_BFS_AUTO, 0, &tree, &info) != BSPGEMM_OK) return 0;
    if (info.complete && (info.pull_mask & 1u) == 0 && info.push_levels + info.pull_levels > 0) *depth = info.depth;
    bspgemm_result_free(tree);
    if (bspgemm_bfs_tree(ctx, A, 0, source, BSPGEMM_BFS_PUSH, 3, &tree, 0) != BSPGEMM_OK) return 0;
    bspgemm_result_free(tree);
    if (bspgemm_bfs_tree(ctx, A, AT, source, BSPGEMM_BFS_PULL, 0, &tree, &info) != BSPGEMM_OK) return 0;
    if (bspgemm_matrix_from_result(ctx, tree, n, &up) == BSPGEMM_OK) bspgemm_matrix_transpose(ctx, up, &down);
    bspgemm_matrix_free(up);
    bspgemm_result_free(tree);
    return down;
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the NULL argument is refused first
    sentinel, last = SENTINEL, last_error

    def dirty():
        return dirtied(bspgemm.BfsTreeInfo, 0x5A)

    for ctx, A in ((None, fake), (fake, None)):
        out, info = C.c_void_p(sentinel), dirty()
        assert L.bspgemm_bfs_tree(ctx, A, None, 0, 0, 0, C.byref(out), C.byref(info)) == ERR_INVALID
        assert not out.value and "bspgemm_bfs_tree" in last() and "NULL" in last(), last()
        assert not any(info.as_dict().values()) and bytes(info) == bytes(C.sizeof(info))
    info = dirty()
    assert L.bspgemm_bfs_tree(fake, fake, fake, 0, 0, 0, None, C.byref(info)) == ERR_INVALID
    assert "bspgemm_bfs_tree" in last() and "NULL" in last(), last()
    assert bytes(info) == bytes(C.sizeof(info))
    out = C.c_void_p(sentinel)
    assert L.bspgemm_bfs_tree(None, None, None, 0, 0, 0, C.byref(out), None) == ERR_INVALID and not out.value
    for direction in (-1, 3):        # refused before either operand is looked at
        out, info = C.c_void_p(sentinel), dirty()
        assert L.bspgemm_bfs_tree(fake, fake, None, 0, direction, 0, C.byref(out), C.byref(info)) == ERR_INVALID
        assert not out.value and "bspgemm_bfs_tree" in last() and "direction" in last(), last()
        assert bytes(info) == bytes(C.sizeof(info))


# ---------------------------------------------------------------- the reference itself -------------------------------
def _full(name):
    rp, ci, n, source = ref.graph(name)
    return ref.search(rp, ci, n, source)


@pytest.mark.parametrize("name", list(ref.GRAPHS))
def test_reference_levels_equal_scipy_and_parents_pass_the_tree_check(name):
    rp, ci, n, source = ref.graph(name)
    level, parent, frontiers, left = _full(name)
    assert np.array_equal(level, bfs_ref.distances(rp, ci, n, [source])[0])
    assert left == 0 and len(frontiers) == int(level.max()) + 1           # the last, empty level was attempted
    assert sum(f[0] for f in frontiers) == int((level >= 0).sum())
    t_rp, t_parent, t_level = ref.expected(name)
    assert (t_rp.dtype, t_parent.dtype, t_level.dtype) == (np.int64, np.int32, np.int32)
    ref.tree_check(rp, ci, n, source, t_rp, t_parent, t_level)
    # the smallest candidate: no stored (u, v) with level(u) == level(v) - 1 and u < parent(v)
    rows = np.repeat(np.arange(n), np.diff(rp))
    up = (level[rows] >= 0) & (level[ci] == level[rows] + 1)
    assert (rows[up] >= parent[ci[up]]).all()


def test_reference_on_a_hand_example():
    # 0 -> {3, 2}; 3 -> {1, 4}; 2 -> {1, 4, 0}; 1 -> 5; 4 -> {5, 4}; 6 -> 0 is never walked.  1 and 4 have the candidate
    # parents 2 and 3: the smaller one wins whatever the order of the rows' entries.  5 has the candidates 1 and 4.
    rp = np.array([0, 2, 3, 6, 8, 10, 10, 11], np.int32)
    ci = np.array([3, 2, 5, 1, 4, 0, 1, 4, 5, 4, 0], np.int32)
    level, parent, frontiers, left = ref.search(rp, ci, 7, 0)
    assert level.tolist() == [0, 2, 1, 1, 2, 3, -1] and parent.tolist() == [0, 2, 0, 0, 2, 1, -1]
    assert frontiers == [(1, 2), (2, 5), (2, 3), (1, 0)] and left == 0
    t_rp, t_parent, t_level = ref.bfs_tree(rp, ci, 7, 0)
    assert t_rp.tolist() == [0, 1, 2, 3, 4, 5, 6, 6] and t_parent.tolist() == [0, 2, 0, 0, 2, 1]
    assert t_level.tolist() == [0, 2, 1, 1, 2, 3]
    t_rp, t_parent, t_level = ref.bfs_tree(rp, ci, 7, 0, max_depth=1)
    assert t_rp.tolist() == [0, 1, 1, 2, 3, 3, 3, 3] and t_parent.tolist() == [0, 0, 0] and t_level.tolist() == [0, 1, 1]
    m = ref.model(rp, ci, 7, 0, "push")
    assert m == {"reached": 6, "edges_pushed": 10, "pull_mask": 0, "depth": 3, "complete": 1, "push_levels": 4, "pull_levels": 0}
    assert ref.model(rp, ci, 7, 0, "pull")["pull_mask"] == 0b1111
    assert ref.model(rp, ci, 7, 0, "push", max_depth=2) == {"reached": 5, "edges_pushed": 7, "pull_mask": 0, "depth": 2,
                                                            "complete": 0, "push_levels": 2, "pull_levels": 0}
    with pytest.raises(AssertionError):                                  # a parent that is not one level up
        ref.tree_check(rp, ci, 7, 0, np.array([0, 1, 2, 3, 4, 5, 6, 6]), np.array([0, 2, 0, 0, 2, 2]), np.array([0, 2, 1, 1, 2, 3]))


def test_builders_have_the_shapes_they_promise():
    for m in (63, 64, 65, 5000):
        rp, ci, n, source = ref.graph("star_out%d" % m)
        level, parent, frontiers, _ = _full("star_out%d" % m)
        assert n == m + 1 and frontiers == [(1, m), (m, 0)] and (parent == 0).all()
        level, parent, frontiers, _ = _full("star_in%d" % m)
        assert frontiers == [(1, m), (m, m), (1, 0)] and parent[m + 1] == 1 and level[m + 1] == 2
    for W in (4, 16, 64):
        rp, ci, n, source = ref.graph("rows_around%d" % W)
        assert sorted(set(np.diff(rp)[1:13].tolist())) == [W - 1, W, W + 1]
        assert (np.diff(ci[rp[1]:rp[2]]) < 0).any()                      # the rows are not sorted
        level, parent, frontiers, _ = _full("rows_around%d" % W)
        targets = np.flatnonzero(level == 2)
        assert frontiers[1] == (12, 12 * W) and targets.size > 2 * W and np.unique(parent[targets]).size > 3
        incoming = np.bincount(ci[rp[1]:rp[13]], minlength=n)[targets]
        assert (incoming > 1).sum() > W                                  # several candidate parents
    level, parent, frontiers, _ = _full("layered")
    assert [f[0] for f in frontiers] == [1, 6, 40, 300, 700, 150, 20] and int((level < 0).sum()) == 60
    L = ref.K_PULL_LIGHT
    for length in (L - 1, L, L + 1, 5000):
        for where, a in (("first", 1), ("last", length), ("absent", length + 1)):
            rp, ci, n, source = ref.graph("in_row%d_%s" % (length, where))
            level, parent, _, _ = _full("in_row%d_%s" % (length, where))
            t = length + 2
            assert n == length + 3 and int((ci == t).sum()) == length and level[a] == 1
            assert int((level >= 0).sum()) == (2 if where == "absent" else 3)
            assert (level[t], parent[t]) == ((-1, -1) if where == "absent" else (2, a))
    for n in (257, 1023, 4099):
        level = _full("sparse%d" % n)[0]
        words = (n + 63) // 64
        per_word = np.bincount(np.flatnonzero(level >= 0) // 64, minlength=words)
        assert n % 4 and n % 64 and 64 < (level >= 0).sum() < n and (per_word > 0).all() and (per_word < 64).any()
    level, parent, frontiers, _ = _full("path300")
    assert level.tolist() == list(range(300)) and len(frontiers) == 300
    assert [ref.model(*ref.graph("path300"), max_depth=d)["complete"] for d in (1, 150, 400)] == [0, 0, 1]
    assert [ref.model(*ref.graph("path300"), max_depth=d)["depth"] for d in (1, 150, 400)] == [1, 150, 299]
    for name, reached in (("sink_source", 1), ("single", 1), ("no_edges", 1), ("self_loop_alone", 1), ("self_loop_source", 3)):
        assert int((_full(name)[0] >= 0).sum()) == reached, name
    rp, ci, n, source = ref.graph("untidy300")
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert (rows == ci).any() and np.unique(rows * n + ci).size < ci.size
    for name in ("rmat12_directed", "rmat12", "powerlaw"):
        level = _full(name)[0]
        assert (level >= 0).sum() > 1000, name


def test_the_default_rule_pulls_between_two_push_levels():
    """so that the GPU test of the direction cannot pass vacuously"""
    m = ref.model(*ref.graph("rmat12"))
    levels = m["push_levels"] + m["pull_levels"]
    kinds = [(m["pull_mask"] >> d) & 1 for d in range(levels)]
    assert kinds[0] == 0 and kinds[-1] == 0 and m["pull_levels"] >= 1, kinds
    first = kinds.index(1)
    assert 0 in kinds[first:], kinds                                     # push, ..., pull, ..., push
    # the extreme knobs differ from the defaults: alpha = 1 enters PULL late and beta = 1 leaves it at once; alpha = 2^20
    # enters it at level 1 and beta = 2^20 never leaves it
    assert ref.model(*ref.graph("rmat12"), alpha=1, beta=1)["pull_mask"] != m["pull_mask"]
    assert ref.model(*ref.graph("rmat12"), alpha=2**20, beta=2**20)["pull_mask"] != m["pull_mask"]
