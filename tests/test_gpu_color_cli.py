"""SpGEMM_hip_color, the command-line driver of bspgemm_graph_coloring: on a Matrix Market file written here entry by entry
its line and its --colors file equal what the model gives on the loader's orientation (the transpose of the file's, which
is the same undirected graph), for two orders; bad arguments and bad input end it like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import color_ref
from cli_kit import assert_missing_file, assert_not_square, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_color")
USAGE = "usage: SpGEMM_hip_color"


def test_cli_matches_the_model(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = color_ref.GRAPHS["untidy300"]()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "colors.txt")
    write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    for args, order, seed in ((["--order", "largest", "--seed", "7"], "largest", 7), (["--order", "natural"], "natural", 0),
                              ([], "random", 0)):
        colour, ncolors, rounds = color_ref.coloring(l_rp, l_ci, n, order, seed)
        assert np.array_equal(colour, color_ref.coloring(rp, ci, n, order, seed)[0]) and ncolors > 2
        for extra in ([], ["--colors", out]):
            r = run(CLI, [src] + args + extra)
            assert r.returncode == 0, r.stderr
            f = r.stdout.strip().split(",")
            assert len(f) == 6, r.stdout
            assert [int(x) for x in f[:5]] == [n, ci.size, ncolors, int(np.bincount(colour).max()), rounds], (order, r.stdout)
            assert float(f[5]) > 0, r.stdout
        assert np.array_equal(np.loadtxt(out, dtype=np.int64), colour), order


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    write_edges(src, np.array([0, 1, 2, 2]), np.array([1, 2]), 3, 3)
    for bad in ([], [src, "--colors"], [src, "--order", "smallest"], [src, "--seed", "x"], [src, "--labels", "y"],
                [src, "--order"]):
        assert_usage(run(CLI, bad), USAGE, bad)
    r = run(CLI, [src, "--order", "natural", "--seed", "0x10"])
    assert r.returncode == 0 and r.stdout.strip().split(",")[:5] == ["3", "2", "2", "2", "3"], r.stdout
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
    rect = str(tmp_path / "rect.mtx")
    write_edges(rect, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    assert_not_square(run(CLI, [rect]), "colouring")
    banner = str(tmp_path / "banner.mtx")
    with open(banner, "w") as f:
        f.write("not a matrix market file\n1 1 1\n1 1\n")
    r = run(CLI, [banner])
    assert r.returncode == 1 and "Could not process Matrix Market banner." in r.stdout
