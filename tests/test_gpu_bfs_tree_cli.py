"""SpGEMM_hip_bfs_tree, the command-line driver of bspgemm_bfs_tree: on a Matrix Market file written here entry by entry,
`i j` for the edge i -> j, of a graph that is not symmetric, its two lines equal what the numpy reference gives -- which
fixes the orientation -- under every direction flag; --symmetric on a file that holds every edge both ways; and a bad
source ends it with a message.
"""
import os

import numpy as np
import pytest

import bfs_tree_ref as ref
import cc_ref
from cli_kit import cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_bfs_tree")


def _expect(name, source, direction):
    rp, ci, n, _ = ref.graph(name)
    t_rp, parent, level = ref.bfs_tree(rp, ci, n, source)
    m = ref.model(rp, ci, n, source, direction=direction)
    first = [source, parent.size, m["depth"], int(level.sum(dtype=np.int64)), int(parent.sum(dtype=np.int64))]
    return first, [n, ci.size, m["push_levels"], m["pull_levels"]]


@pytest.mark.parametrize("name,flags,direction", [("rmat12_directed", [], "auto"), ("rmat12_directed", ["--push"], "push"),
                                                  ("rmat12_directed", ["--pull"], "pull"), ("rmat12", ["--symmetric"], "auto"),
                                                  ("rmat12", ["--symmetric", "--pull"], "pull")])
def test_cli_matches_the_reference(tmp_path, name, flags, direction):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n, _ = ref.graph(name)
    source = 5
    if name == "rmat12_directed":                     # the graph must tell an edge from its reverse
        back = cc_ref.csr(ci, np.repeat(np.arange(n), np.diff(rp)), n)
        assert not np.array_equal(ref.search(rp, ci, n, source)[0], ref.search(back[0], back[1], n, source)[0])
    src = str(tmp_path / "graph.mtx")
    write_edges(src, rp, ci, n)
    r = run(CLI, [src, str(source)] + flags)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2, r.stdout
    first, second = _expect(name, source, direction)
    assert first[1] > 1000 and first[2] >= 3
    assert [int(x) for x in lines[0].split(",")] == first, lines[0]
    last = lines[1].split(",")
    assert len(last) == 5 and [int(x) for x in last[:4]] == second and float(last[4]) > 0, lines[1]


@pytest.mark.parametrize("bad", ["4096", "-1", "seven"])
def test_cli_refuses_a_bad_source(tmp_path, bad):
    rp, ci, n, _ = ref.graph("rmat12_directed")
    src = str(tmp_path / "graph.mtx")
    write_edges(src, rp, ci, n)
    r = run(CLI, [src, bad])
    assert r.returncode != 0 and not r.stdout.strip()
    assert ("source" in r.stderr and "bspgemm_bfs_tree" in r.stderr) if bad != "seven" else "not a vertex id" in r.stderr, r.stderr


def test_cli_refuses_an_unknown_flag(tmp_path):
    r = run(CLI, [str(tmp_path / "none.mtx"), "0", "--sideways"])
    assert r.returncode != 0 and "usage" in r.stdout
