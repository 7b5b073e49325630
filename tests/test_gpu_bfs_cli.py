"""SpGEMM_hip_bfs, the command-line driver of bspgemm_bfs: on a Matrix Market file written here entry by entry, `i j` for
the edge i -> j, of a graph that is not symmetric, its lines equal what Context.bfs and the scipy reference give -- which
fixes the orientation -- and a bad source ends it with a message.
"""
import os

import numpy as np
import pytest

import bfs_ref
import bspgemm
import gen
from cli_kit import cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_bfs")


def test_cli_matches_the_api_and_the_reference(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 7601)
    sources = [int(x) for x in np.random.default_rng(3).choice(n, size=5, replace=False)] + [0]
    dist = bfs_ref.distances(rp, ci, n, sources)
    back = bfs_ref.distances(*gen._csr_from_pairs(ci, np.repeat(np.arange(n), np.diff(rp)), n), n, sources)
    assert not np.array_equal(dist, back), "the graph must tell an edge from its reverse"
    src = str(tmp_path / "graph.mtx")
    write_edges(src, rp, ci, n)
    r = run(CLI, [src] + [str(s) for s in sources])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(sources) + 1, r.stdout
    (e_rp, e_ci, e_v), e_depth, e_complete = bfs_ref.bfs_ref(rp, ci, n, sources)
    ctx = bspgemm.Context(0)
    try:
        A = ctx.upload(rp, ci, n)
        R, depth, complete = ctx.bfs(A, sources)
        g_rp, g_ci = R.download()
        g_v = R.download_values()
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci) and np.array_equal(g_v, e_v)
        assert (depth, int(complete)) == (e_depth, e_complete)
        R.free()
        A.free()
    finally:
        ctx.close()
    for s, line in enumerate(lines[:-1]):
        v = e_v[e_rp[s]:e_rp[s + 1]].astype(np.int64)
        assert [int(x) for x in line.split(",")] == [sources[s], v.size, int(v.max()), int(v.sum())], line
    last = lines[-1].split(",")
    assert len(last) == 6 and [int(x) for x in last[:5]] == [n, ci.size, len(sources), e_depth, e_complete], lines[-1]
    assert float(last[5]) > 0 and e_depth >= 3


@pytest.mark.parametrize("bad", ["1024", "-1", "seven"])
def test_cli_refuses_a_bad_source(tmp_path, bad):
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 7601)
    src = str(tmp_path / "graph.mtx")
    write_edges(src, rp, ci, n)
    r = run(CLI, [src, "3", bad])
    assert r.returncode != 0 and not r.stdout.strip()
    assert ("sources[1]" in r.stderr and "bspgemm_bfs" in r.stderr) if bad != "seven" else "not a vertex id" in r.stderr, r.stderr
