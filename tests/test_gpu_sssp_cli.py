"""SpGEMM_hip_sssp, the command-line driver of bspgemm_weights_hashed and bspgemm_sssp: on a Matrix Market file written here
entry by entry its line and its --out file equal what the model and the definition give on the loader's orientation (the
transpose of the file's) under the hashed lengths; bad arguments, a bad source and bad input end it like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import sssp_ref
from cli_kit import assert_missing_file, assert_not_square, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_sssp")
USAGE = "usage: SpGEMM_hip_sssp"


def test_cli_matches_the_model(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    g = sssp_ref.rmat(10, False)
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "dist.txt")
    write_edges(src, g.rp, g.ci, g.n, g.n)
    rp, ci, _, _ = bspgemm.readCOO(src)                                 # what the driver uploads
    source = int(np.argmax(np.diff(rp)))
    for args, (seed, lo, hi), sym, delta, lanes in (
            ([], (0, 1, 255), False, 0, 0),
            (["--weights", "9:0:1000", "--symmetric", "--delta", "16", "--lanes", "16"], (9, 0, 1000), True, 16, 16),
            (["--delta", "18446744073709551615", "--weights", "16:5:5"], (16, 5, 5), False, sssp_ref.INF, 0)):
        w = sssp_ref.weight_hash(rp, ci, g.n, seed, lo, hi, sym)
        m = sssp_ref.model(rp, ci, w, g.n, source, delta, lanes)
        parent = sssp_ref.parents(rp, ci, w, g.n, source, m.dist)
        assert np.array_equal(m.dist, sssp_ref.dijkstra(rp, ci, w, g.n, source)) and m.reached > g.n // 2
        want = [g.n, ci.size, source, m.delta, m.reached, m.dist_max, m.rounds, m.buckets, m.entries_walked, m.improved, m.hub_chunks]
        for extra in ([], ["--out", out]):
            p = run(CLI, [src, "--source", str(source)] + args + extra)
            assert p.returncode == 0, p.stderr
            f = p.stdout.strip().split(",")
            assert len(f) == 12, p.stdout
            assert [int(x) for x in f[:11]] == want, (args, p.stdout)
            assert float(f[11]) > 0, p.stdout
        v = np.flatnonzero(m.dist != sssp_ref.NONE)
        rows = [ln.split() for ln in open(out).read().splitlines()]
        assert [[int(x) for x in r] for r in rows] == [[int(a), int(m.dist[a]), int(parent[a])] for a in v], args


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    write_edges(src, np.array([0, 1, 2, 2]), np.array([1, 2]), 3, 3)    # the file's 0 -> 1 -> 2 is the loader's 2 -> 1 -> 0
    for bad in ([], [src], [src, "--out", "x"], [src, "--source"], [src, "--source", "x"], [src, "--source", "-1"],
                [src, "--source", "0", "--lanes", "8"], [src, "--source", "0", "--weights", "1:9:2"],
                [src, "--source", "0", "--weights", "1:2"], [src, "--source", "0", "--delta"], [src, "--source", "0", "--delta", "18446744073709551616"], [src, "--source", "0", "--paths", "y"]):
        assert_usage(run(CLI, bad), USAGE, bad)
    r = run(CLI, [src, "--source", "2", "--weights", "0:3:3"])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:8] == ["3", "2", "2", "96", "3", "6", "3", "1"], r.stdout
    r = run(CLI, [src, "--source", "3"])                                    # a bad source: no vertex of the graph
    assert r.returncode == 1 and r.stdout == "" and "source 3 is not a vertex of a graph of 3" in r.stderr, (r.stdout, r.stderr)
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx"), "--source", "0"]))
    rect = str(tmp_path / "rect.mtx")
    write_edges(rect, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    assert_not_square(run(CLI, [rect, "--source", "0"]), "shortest paths")
