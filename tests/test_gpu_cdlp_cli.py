"""SpGEMM_hip_cdlp, the command-line driver of bspgemm_label_propagation: on a Matrix Market file written here entry by
entry its line and its --labels file equal what the model gives on the loader's orientation (the transpose of the file's,
which is the same undirected graph), for the default and for given iteration counts; bad arguments and bad input end it
like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import cdlp_ref
from cli_kit import assert_missing_file, assert_not_square, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_cdlp")
USAGE = "usage: SpGEMM_hip_cdlp"


def test_cli_matches_the_model(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = cdlp_ref.GRAPHS["untidy300"]()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "labels.txt")
    write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    for args, max_iter in (([], 10), (["--iterations", "3"], 3), (["--iterations", "0"], 0)):
        labels, iterations, converged, _, communities = cdlp_ref.label_propagation(l_rp, l_ci, n, max_iter)
        assert np.array_equal(labels, cdlp_ref.label_propagation(rp, ci, n, max_iter)[0]) and 2 < communities <= n
        for extra in ([], ["--labels", out]):
            r = run(CLI, [src] + args + extra)
            assert r.returncode == 0, r.stderr
            f = r.stdout.strip().split(",")
            assert len(f) == 7, r.stdout
            assert [int(x) for x in f[:6]] == [n, ci.size, communities, int(np.bincount(labels).max()), iterations, converged], \
                (max_iter, r.stdout)
            assert float(f[6]) > 0, r.stdout
        assert np.array_equal(np.loadtxt(out, dtype=np.int64), labels), max_iter
    # a graph that converges: two triangles
    tri = str(tmp_path / "triangles.mtx")
    write_edges(tri, np.array([0, 2, 3, 3, 5, 6, 6]), np.array([1, 2, 2, 4, 5, 5]), 6, 6)
    r = run(CLI, [tri, "--labels", out])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:6] == ["6", "6", "2", "3", "3", "1"], r.stdout
    assert np.loadtxt(out, dtype=np.int64).tolist() == [0, 0, 0, 3, 3, 3]


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    write_edges(src, np.array([0, 1, 2, 2]), np.array([1, 2]), 3, 3)
    for bad in ([], [src, "--labels"], [src, "--iterations", "x"], [src, "--iterations", "-1"], [src, "--colors", "y"],
                [src, "--iterations"]):
        assert_usage(run(CLI, bad), USAGE, bad)
    r = run(CLI, [src, "--iterations", "0x2"])                          # the path 0 - 1 - 2 after two iterations
    assert r.returncode == 0 and r.stdout.strip().split(",")[:6] == ["3", "2", "2", "2", "2", "0"], r.stdout
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
    rect = str(tmp_path / "rect.mtx")
    write_edges(rect, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    assert_not_square(run(CLI, [rect]), "label propagation")
