"""SpGEMM_hip_match, the command-line driver of bspgemm_maximal_matching: on a Matrix Market file written here entry by entry
its line and its --out file equal what the model gives on the loader's orientation (the transpose of the file's, which is
the same undirected graph), for the three orders; bad arguments and bad input end it like the other drivers.
"""
import os
import subprocess

import numpy as np
import pytest

import bspgemm
import match_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(bspgemm.LIB_PATH), "SpGEMM_hip_match")
USAGE = "usage: SpGEMM_hip_match"


def _write_edges(path, rp, ci, rows, cols):
    r = np.repeat(np.arange(rows), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate pattern general\n%d %d %d\n" % (rows, cols, ci.size))
        f.write("".join("%d %d\n" % (a + 1, b + 1) for a, b in zip(r.tolist(), ci.tolist())))


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def test_cli_matches_the_model(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = match_ref.GRAPHS["untidy300"]()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "pairs.txt")
    _write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    for args, order, seed in ((["--order", "light", "--seed", "7"], "light", 7), (["--order", "natural"], "natural", 0),
                              ([], "random", 0)):
        r = match_ref.matching(l_rp, l_ci, n, order, seed)
        assert np.array_equal(r.mate, match_ref.matching(rp, ci, n, order, seed).mate) and r.pairs > 2
        for extra in ([], ["--out", out]):
            p = _run([src] + args + extra)
            assert p.returncode == 0, p.stderr
            f = p.stdout.strip().split(",")
            assert len(f) == 5, p.stdout
            assert [int(x) for x in f[:4]] == [n, ci.size, r.pairs, r.rounds], (order, p.stdout)
            assert float(f[4]) > 0, p.stdout
        v = np.flatnonzero(r.mate > np.arange(n))
        assert np.array_equal(np.loadtxt(out, dtype=np.int64).reshape(-1, 2), np.stack([v, r.mate[v]], axis=1)), order


def test_cli_usage_and_bad_input(tmp_path):
    src = str(tmp_path / "graph.mtx")
    _write_edges(src, np.array([0, 1, 2, 2]), np.array([1, 2]), 3, 3)
    for bad in ([], [src, "--out"], [src, "--order", "heavy"], [src, "--seed", "x"], [src, "--mates", "y"], [src, "--order"]):
        r = _run(bad)
        assert r.returncode == 1 and r.stdout.startswith(USAGE), (bad, r.stdout)
    r = _run([src, "--order", "natural", "--seed", "0x10"])            # the path 0 - 1 - 2: the pair (0, 1), then 2 retires
    assert r.returncode == 0 and r.stdout.strip().split(",")[:4] == ["3", "2", "1", "2"], r.stdout
    r = _run([str(tmp_path / "missing.mtx")])
    assert r.returncode == 1 and r.stdout == ""
    rect = str(tmp_path / "rect.mtx")
    _write_edges(rect, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    r = _run([rect])
    assert r.returncode == 1 and r.stdout == "" and "matching needs a square matrix (2x3)" in r.stderr, (r.stdout, r.stderr)
