"""SpGEMM_hip_scc, the command-line driver of bspgemm_strongly_connected_components: on Matrix Market files written here
entry by entry its line and its --labels file equal what the scipy reference gives on the loader's orientation (the
transpose of the file's, which has the same components); bad input ends it like the other drivers.
"""
import os
import subprocess

import numpy as np
import pytest

import bspgemm
import scc_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(bspgemm.LIB_PATH), "SpGEMM_hip_scc")


def _write_edges(path, rp, ci, rows, cols):
    r = np.repeat(np.arange(rows), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate pattern general\n%d %d %d\n" % (rows, cols, ci.size))
        f.write("".join("%d %d\n" % (a + 1, b + 1) for a, b in zip(r.tolist(), ci.tolist())))


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def test_cli_matches_the_reference(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = scc_ref.tails()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "labels.txt")
    _write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    t_rp, t_ci, _ = scc_ref.transposed(rp, ci, n)
    assert np.array_equal(l_rp, t_rp) and np.array_equal(np.sort(l_ci), np.sort(t_ci))
    label, count = scc_ref.labels(l_rp, l_ci, n)
    assert np.array_equal(label, scc_ref.labels(rp, ci, n)[0]) and (count, scc_ref.largest(label)) == (42, 30)
    for extra in ([], ["--labels", out]):
        r = _run([src] + extra)
        assert r.returncode == 0, r.stderr
        f = r.stdout.strip().split(",")
        assert len(f) == 7 and [int(x) for x in f[:5]] == [n, ci.size, 42, 30, 1], r.stdout
        assert 3 <= int(f[5]) <= 4 * (n + 2) and float(f[6]) > 0, r.stdout
    assert np.array_equal(np.loadtxt(out, dtype=np.int64), label)


def test_cli_on_a_one_line_file(tmp_path):
    """one entry 2 -> 1 among three vertices: a DAG, no colouring round, one sweep"""
    src, out = str(tmp_path / "one.mtx"), str(tmp_path / "labels.txt")
    _write_edges(src, np.array([0, 0, 1, 1]), np.array([0]), 3, 3)
    r = _run([src, "--labels", out])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().split(",")[:6] == ["3", "1", "3", "1", "0", "1"], r.stdout
    assert np.loadtxt(out, dtype=np.int64).tolist() == [0, 1, 2]


def test_cli_usage_and_bad_input(tmp_path):
    r = _run([])
    assert r.returncode == 1 and r.stdout.startswith("usage: SpGEMM_hip_scc")
    r = _run([str(tmp_path / "graph.mtx"), "--labels"])
    assert r.returncode == 1 and r.stdout.startswith("usage: SpGEMM_hip_scc")
    r = _run([str(tmp_path / "missing.mtx")])
    assert r.returncode == 1 and r.stdout == ""
    src = str(tmp_path / "rect.mtx")
    _write_edges(src, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    r = _run([src])
    assert r.returncode == 1 and r.stdout == "" and "scc needs a square matrix (2x3)" in r.stderr, (r.stdout, r.stderr)
    src = str(tmp_path / "banner.mtx")
    with open(src, "w") as f:
        f.write("not a matrix market file\n1 1 1\n1 1\n")
    r = _run([src])
    assert r.returncode == 1 and "Could not process Matrix Market banner." in r.stdout
