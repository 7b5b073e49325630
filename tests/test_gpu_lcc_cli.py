"""SpGEMM_hip_lcc, the command-line driver of bspgemm_local_clustering: on tests/golden/loader_case.mtx its line and its
--out file equal what the model gives on bspgemm_readCOO's output (the transpose of the file's orientation: the same
undirected graph, and the directed count does not see the difference), with and without --directed; bad arguments and bad
input end it like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import lcc_ref
from cli_kit import assert_missing_file, assert_not_square, assert_usage, cli_path, run

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_lcc")
USAGE = "usage: SpGEMM_hip_lcc"


def _write_edges(path, pairs, rows, cols):
    """(its own: the pairs are written in the order given, which is not row order, so no CSR says it)"""
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate pattern general\n%d %d %d\n" % (rows, cols, len(pairs)))
        f.write("".join("%d %d\n" % (a + 1, b + 1) for a, b in pairs))


def _read_out(path, n):
    """the --out file: (vertex ids, coefficients as the doubles that %.17g round-trips)"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == n + 1
    return [int(x.split(" ")[0]) for x in lines[:-1]], np.array([float(x.split(" ")[1]) for x in lines[:-1]])


def test_cli_matches_the_model_on_the_loader_fixture(tmp_path, golden_dir):
    assert os.path.exists(CLI), "%s is not built" % CLI
    src, out = os.path.join(golden_dir, "loader_case.mtx"), str(tmp_path / "lcc.txt")
    rp, ci, m, n = bspgemm.readCOO(src)                                  # what the driver uploads
    assert m == n == 40
    for args, directed in (([], False), (["--directed"], True)):
        num, d, lcc, triangles, _ = lcc_ref.local_clustering(rp, ci, n, directed)
        for extra in ([], ["--out", out]):
            r = run(CLI, [src] + args + extra)
            assert r.returncode == 0, r.stderr
            f = r.stdout.strip().split(",")
            assert len(f) == 6, r.stdout
            assert [int(f[0]), int(f[1]), int(f[2]), int(f[4])] == [n, ci.size, triangles, int(d.max())], (directed, r.stdout)
            mean = 0.0
            for x in lcc.tolist():                                       # the driver's sum, in its order
                mean += x
            assert float(f[3]) == mean / n and float(f[5]) > 0, (directed, r.stdout)
        ids, got = _read_out(out, n)
        assert ids == list(range(n)) and got.tobytes() == lcc.tobytes(), directed
    und, dire = lcc_ref.local_clustering(rp, ci, n)[0], lcc_ref.local_clustering(rp, ci, n, True)[0]
    assert und.any() and not np.array_equal(und, dire)                   # the fixture has triangles, and one-way edges
    # the file's own orientation gives the same answers
    t_rp, t_ci, _ = lcc_ref.transposed(rp, ci, n)
    assert np.array_equal(lcc_ref.local_clustering(t_rp, t_ci, n, True)[0], dire)


def test_cli_on_hand_examples(tmp_path):
    out = str(tmp_path / "lcc.txt")
    cyc = str(tmp_path / "cycle.mtx")
    _write_edges(cyc, [(0, 1), (1, 2), (2, 0), (1, 0)], 3, 3)           # a directed 3-cycle with one reciprocal edge
    r = run(CLI, [cyc, "--out", out])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:5] == ["3", "4", "1", "1", "2"], r.stdout
    assert _read_out(out, 3)[1].tolist() == [1.0, 1.0, 1.0]
    r = run(CLI, [cyc, "--out", out, "--directed"])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:5] == ["3", "4", "1", "%.17g" % ((0.5 + 0.5 + 1.0) / 3), "2"], r.stdout
    assert _read_out(out, 3)[1].tolist() == [0.5, 0.5, 1.0]
    star = str(tmp_path / "star.mtx")
    _write_edges(star, [(0, 1), (0, 2), (0, 3), (3, 3)], 4, 4)
    r = run(CLI, [star])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:5] == ["4", "4", "0", "0", "3"], r.stdout


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    _write_edges(src, [(0, 1), (1, 2)], 3, 3)
    for bad in ([], [src, "--out"], [src, "--undirected"], [src, "--directed", "x"], [src, "--out", "a", "--out"]):
        assert_usage(run(CLI, bad), USAGE, bad)
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
    rect = str(tmp_path / "rect.mtx")
    _write_edges(rect, [(0, 2), (1, 0)], 2, 3)
    assert_not_square(run(CLI, [rect]), "the clustering coefficient")
