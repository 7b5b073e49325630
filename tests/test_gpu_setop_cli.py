"""SpGEMM_hip_ktruss --symmetrize: a `general` Matrix Market file of a directed graph gives the triangle count and the truss
of its underlying undirected graph; without the flag the driver does what it did before.
"""
import os

import numpy as np
import pytest

import bspgemm
import gen
import ktruss_ref
from cli_kit import assert_usage, cli_path, run

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_ktruss")


def test_symmetrize_flag(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = gen.rmat(7, 10, (0.57, 0.19, 0.19, 0.05), 11001)
    src, dst = str(tmp_path / "directed.mtx"), str(tmp_path / "truss.mtx")
    bspgemm.write_mtx(src, rp, ci)
    assert "general" in open(src).readline()
    s_rp, s_ci = ktruss_ref.symmetrise(rp, ci, n)
    assert s_ci.size > ci.size                                # the file's graph is directed
    k = 4
    r = run(CLI, ["--symmetrize", src, str(k), dst])
    assert r.returncode == 0, r.stderr
    fields = r.stdout.strip().split(",")
    assert len(fields) == 8, r.stdout
    (t_rp, t_ci), it, conv = ktruss_ref.ktruss_ref(s_rp, s_ci, n, k)
    tri = ktruss_ref.triangles_ref(s_rp, s_ci, n)
    assert [int(x) for x in fields[:7]] == [n, ci.size, tri, k, t_ci.size, it, int(conv)]
    assert tri > 0 and 0 < t_ci.size < s_ci.size
    w_rp, w_ci, wm, _ = bspgemm.readCOO(dst)
    assert wm == n and np.array_equal(w_rp, t_rp) and np.array_equal(w_ci, t_ci)

    # without the flag: the line of the API on the operand as loaded
    r2 = run(CLI, [src, str(k)])
    assert r2.returncode == 0, r2.stderr
    plain = r2.stdout.strip().split(",")
    ctx = bspgemm.Context(0)
    try:
        l_rp, l_ci, m, _ = bspgemm.readCOO(src, expand_symmetric=True)
        A = ctx.upload(l_rp, l_ci, m)
        T, a_it, a_conv = ctx.ktruss(A, k)
        assert [int(x) for x in plain[:7]] == [n, ci.size, ctx.triangle_count(A), k, T.nnz, a_it, int(a_conv)]
        assert plain[:7] != fields[:7]
    finally:
        ctx.close()
    # the flag does not change the usage check
    assert_usage(run(CLI, ["--symmetrize", src]), "usage: SpGEMM_hip_ktruss")
