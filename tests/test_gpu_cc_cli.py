"""SpGEMM_hip_cc, the command-line driver of bspgemm_connected_components: on a Matrix Market file written here entry by
entry, its line and its --labels file equal what the scipy reference gives; a missing file ends it like the other drivers.
"""
import os

import numpy as np
import pytest

import cc_ref
import gen
from cli_kit import assert_missing_file, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_cc")


def test_cli_matches_the_reference(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = gen.rmat(10, 6, (0.57, 0.19, 0.19, 0.05), 7601)
    label, count = cc_ref.labels(rp, ci, n)
    largest = int(np.bincount(label).max())
    assert 1 < count < n and 1 < largest < n
    src, out = str(tmp_path / "graph.mtx"), str(tmp_path / "labels.txt")
    write_edges(src, rp, ci, n)
    for extra in ([], ["--labels", out]):
        r = run(CLI, [src] + extra)
        assert r.returncode == 0, r.stderr
        f = r.stdout.strip().split(",")
        assert len(f) == 6 and [int(x) for x in f[:4]] == [n, ci.size, count, largest], r.stdout
        assert 1 <= int(f[4]) <= n + 1 and float(f[5]) > 0, r.stdout
    assert np.array_equal(np.loadtxt(out, dtype=np.int64), label)


def test_cli_usage_and_missing_file(tmp_path):
    assert_usage(run(CLI, []), "usage: SpGEMM_hip_cc")
    assert_usage(run(CLI, [str(tmp_path / "graph.mtx"), "--labels"]), "usage: SpGEMM_hip_cc")
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
