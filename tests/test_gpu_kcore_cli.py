"""SpGEMM_hip_kcore, the command-line driver of bspgemm_core_numbers and bspgemm_kcore: on a Matrix Market file written here
entry by entry as a `general` file, its line, its --numbers file and its --k --out file equal what the numpy reference
gives; usage and a missing file end it like the other drivers.
"""
import os

import numpy as np
import pytest

import bspgemm
import kcore_ref
from cli_kit import assert_missing_file, assert_usage, cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_kcore")


def test_cli_matches_the_reference(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = kcore_ref.GRAPHS["rmat10"]()
    core, top, rounds = kcore_ref.core_numbers(rp, ci, n)
    at_top = int((core == top).sum())
    assert top > 3 and 0 < at_top < n
    src, numbers, out = str(tmp_path / "graph.mtx"), str(tmp_path / "numbers.txt"), str(tmp_path / "core.mtx")
    write_edges(src, rp, ci, n)
    for extra in ([], ["--numbers", numbers], ["--k", "3", "--out", out], ["--k", "3", "--out", out, "--numbers", numbers]):
        r = run(CLI, [src] + extra)
        assert r.returncode == 0, r.stderr
        f = r.stdout.strip().split(",")
        assert len(f) == 6 and [int(x) for x in f[:4]] == [n, ci.size, top, at_top], r.stdout
        assert int(f[4]) == rounds and float(f[5]) > 0, r.stdout
    assert np.array_equal(np.loadtxt(numbers, dtype=np.int64), core)
    # the loader hands back the transpose of the file's matrix; the k-core is symmetric, so that is the k-core itself
    t_rp, t_ci, M, N = bspgemm.readCOO(out)
    e_rp, e_ci = kcore_ref.kcore(rp, ci, n, 3)
    assert (M, N) == (n, n) and 0 < e_ci.size < kcore_ref.simple(rp, ci, n)[1].size
    from scipy.sparse import csr_matrix
    T = csr_matrix((np.ones(t_ci.size, np.int8), t_ci, t_rp), shape=(n, n))
    T.sort_indices()
    assert np.array_equal(T.indptr, e_rp) and np.array_equal(T.indices, e_ci)


def test_cli_usage_and_missing_file(tmp_path):
    assert_usage(run(CLI, []), "usage: SpGEMM_hip_kcore")
    for extra in (["--numbers"], ["--k", "3"], ["--out", str(tmp_path / "core.mtx")], ["--labels", "x"]):
        assert_usage(run(CLI, [str(tmp_path / "graph.mtx")] + extra), "usage: SpGEMM_hip_kcore", extra)
    assert_missing_file(run(CLI, [str(tmp_path / "missing.mtx")]))
