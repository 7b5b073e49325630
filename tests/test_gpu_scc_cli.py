"""SpGEMM_hip_scc, the command-line driver of bspgemm_strongly_connected_components: on Matrix Market files written here
entry by entry its line and its --labels file equal what the scipy reference gives on the loader's orientation (the
transpose of the file's, which has the same components); bad input ends it like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import scc_ref
from cli_kit import assert_missing_file, assert_not_square, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_scc")


def test_cli_matches_the_reference(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = scc_ref.tails()
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "labels.txt")
    write_edges(src, rp, ci, n, n)
    l_rp, l_ci, _, _ = bspgemm.readCOO(src)                             # what the driver uploads
    t_rp, t_ci, _ = scc_ref.transposed(rp, ci, n)
    assert np.array_equal(l_rp, t_rp) and np.array_equal(np.sort(l_ci), np.sort(t_ci))
    label, count = scc_ref.labels(l_rp, l_ci, n)
    assert np.array_equal(label, scc_ref.labels(rp, ci, n)[0]) and (count, scc_ref.largest(label)) == (42, 30)
    for extra in ([], ["--labels", out]):
        r = run(CLI, [src] + extra)
        assert r.returncode == 0, r.stderr
        f = r.stdout.strip().split(",")
        assert len(f) == 7 and [int(x) for x in f[:5]] == [n, ci.size, 42, 30, 1], r.stdout
        assert 3 <= int(f[5]) <= 4 * (n + 2) and float(f[6]) > 0, r.stdout
    assert np.array_equal(np.loadtxt(out, dtype=np.int64), label)


def test_cli_on_a_one_line_file(tmp_path):
    """one entry 2 -> 1 among three vertices: a DAG, no colouring round, one sweep"""
    src, out = str(tmp_path / "one.mtx"), str(tmp_path / "labels.txt")
    write_edges(src, np.array([0, 0, 1, 1]), np.array([0]), 3, 3)
    r = run(CLI, [src, "--labels", out])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().split(",")[:6] == ["3", "1", "3", "1", "0", "1"], r.stdout
    assert np.loadtxt(out, dtype=np.int64).tolist() == [0, 1, 2]


def test_cli_usage_and_bad_input(tmp_path):
    assert_usage(run(CLI, []), "usage: SpGEMM_hip_scc")
    assert_usage(run(CLI, [str(tmp_path / "graph.mtx"), "--labels"]), "usage: SpGEMM_hip_scc")
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
    src = str(tmp_path / "rect.mtx")
    write_edges(src, np.array([0, 1, 2]), np.array([2, 0]), 2, 3)
    assert_not_square(run(CLI, [src]), "scc")
    src = str(tmp_path / "banner.mtx")
    with open(src, "w") as f:
        f.write("not a matrix market file\n1 1 1\n1 1\n")
    r = run(CLI, [src])
    assert r.returncode == 1 and "Could not process Matrix Market banner." in r.stdout
