"""SpGEMM_hip_match, the command-line driver of bspgemm_maximal_matching: on a Matrix Market file written here entry by entry
its line and its --out file equal what the model gives on the loader's orientation (the transpose of the file's, which is
the same undirected graph), for the three orders; bad arguments and bad input end it like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import match_ref
from cli_kit import assert_missing_file, assert_not_square, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_match")
USAGE = "usage: SpGEMM_hip_match"


def test_cli_matches_the_model(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = match_ref.GRAPHS["untidy300"]()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "pairs.txt")
    write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    for args, order, seed in ((["--order", "light", "--seed", "7"], "light", 7), (["--order", "natural"], "natural", 0),
                              ([], "random", 0)):
        r = match_ref.matching(l_rp, l_ci, n, order, seed)
        assert np.array_equal(r.mate, match_ref.matching(rp, ci, n, order, seed).mate) and r.pairs > 2
        for extra in ([], ["--out", out]):
            p = run(CLI, [src] + args + extra)
            assert p.returncode == 0, p.stderr
            f = p.stdout.strip().split(",")
            assert len(f) == 5, p.stdout
            assert [int(x) for x in f[:4]] == [n, ci.size, r.pairs, r.rounds], (order, p.stdout)
            assert float(f[4]) > 0, p.stdout
        v = np.flatnonzero(r.mate > np.arange(n))
        assert np.array_equal(np.loadtxt(out, dtype=np.int64).reshape(-1, 2), np.stack([v, r.mate[v]], axis=1)), order


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    write_edges(src, np.array([0, 1, 2, 2]), np.array([1, 2]), 3, 3)
    for bad in ([], [src, "--out"], [src, "--order", "heavy"], [src, "--seed", "x"], [src, "--mates", "y"], [src, "--order"]):
        assert_usage(run(CLI, bad), USAGE, bad)
    r = run(CLI, [src, "--order", "natural", "--seed", "0x10"])            # the path 0 - 1 - 2: the pair (0, 1), then 2 retires
    assert r.returncode == 0 and r.stdout.strip().split(",")[:4] == ["3", "2", "1", "2"], r.stdout
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
    rect = str(tmp_path / "rect.mtx")
    write_edges(rect, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    assert_not_square(run(CLI, [rect]), "matching")
