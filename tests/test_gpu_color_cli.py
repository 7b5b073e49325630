"""SpGEMM_hip_color, the command-line driver of bspgemm_graph_coloring: on a Matrix Market file written here entry by entry
its line and its --colors file equal what the model gives on the loader's orientation (the transpose of the file's, which
is the same undirected graph), for two orders; bad arguments and bad input end it like the other drivers.
"""
import os
import subprocess

import numpy as np
import pytest

import bspgemm
import color_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(bspgemm.LIB_PATH), "SpGEMM_hip_color")
USAGE = "usage: SpGEMM_hip_color"


def _write_edges(path, rp, ci, rows, cols):
    r = np.repeat(np.arange(rows), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate pattern general\n%d %d %d\n" % (rows, cols, ci.size))
        f.write("".join("%d %d\n" % (a + 1, b + 1) for a, b in zip(r.tolist(), ci.tolist())))


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def test_cli_matches_the_model(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = color_ref.GRAPHS["untidy300"]()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "colors.txt")
    _write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    for args, order, seed in ((["--order", "largest", "--seed", "7"], "largest", 7), (["--order", "natural"], "natural", 0),
                              ([], "random", 0)):
        colour, ncolors, rounds = color_ref.coloring(l_rp, l_ci, n, order, seed)
        assert np.array_equal(colour, color_ref.coloring(rp, ci, n, order, seed)[0]) and ncolors > 2
        for extra in ([], ["--colors", out]):
            r = _run([src] + args + extra)
            assert r.returncode == 0, r.stderr
            f = r.stdout.strip().split(",")
            assert len(f) == 6, r.stdout
            assert [int(x) for x in f[:5]] == [n, ci.size, ncolors, int(np.bincount(colour).max()), rounds], (order, r.stdout)
            assert float(f[5]) > 0, r.stdout
        assert np.array_equal(np.loadtxt(out, dtype=np.int64), colour), order


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    _write_edges(src, np.array([0, 1, 2, 2]), np.array([1, 2]), 3, 3)
    for bad in ([], [src, "--colors"], [src, "--order", "smallest"], [src, "--seed", "x"], [src, "--labels", "y"],
                [src, "--order"]):
        r = _run(bad)
        assert r.returncode == 1 and r.stdout.startswith(USAGE), (bad, r.stdout)
    r = _run([src, "--order", "natural", "--seed", "0x10"])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:5] == ["3", "2", "2", "2", "3"], r.stdout
    r = _run([str(tmp_path / "missing.mtx")])
    assert r.returncode == 1 and r.stdout == ""
    rect = str(tmp_path / "rect.mtx")
    _write_edges(rect, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    r = _run([rect])
    assert r.returncode == 1 and r.stdout == "" and "colouring needs a square matrix (2x3)" in r.stderr, (r.stdout, r.stderr)
    banner = str(tmp_path / "banner.mtx")
    with open(banner, "w") as f:
        f.write("not a matrix market file\n1 1 1\n1 1\n")
    r = _run([banner])
    assert r.returncode == 1 and "Could not process Matrix Market banner." in r.stdout
