"""SpGEMM_hip_ktruss, the command-line driver of bspgemm_triangle_count and bspgemm_ktruss: its CSV line equals what the
Python view computes, and the truss it writes reads back as that truss.
"""
import os

import numpy as np
import pytest

import bspgemm
import gen
from cli_kit import cli_path, run
from ktruss_ref import symmetrise

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_ktruss")


def test_cli_matches_the_api(tmp_path):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = gen.rmat(11, 12, (0.57, 0.19, 0.19, 0.05), 7501)
    s_rp, s_ci = symmetrise(rp, ci, n)
    src, dst = str(tmp_path / "graph.mtx"), str(tmp_path / "truss.mtx")
    bspgemm.write_mtx(src, s_rp, s_ci)
    k = 5
    r = run(CLI, [src, str(k), dst])
    assert r.returncode == 0, r.stderr
    fields = r.stdout.strip().split(",")
    assert len(fields) == 8, r.stdout
    ctx = bspgemm.Context(0)
    try:
        # the loader hands back the file's matrix transposed; the pattern is symmetric, so as a set it is the graph
        l_rp, l_ci, m, _ = bspgemm.readCOO(src, expand_symmetric=True)
        A = ctx.upload(l_rp, l_ci, m)
        tri = ctx.triangle_count(A)
        T, it, conv = ctx.ktruss(A, k)
        t_rp, t_ci = T.download()
        assert [int(x) for x in fields[:7]] == [n, s_ci.size, tri, k, T.nnz, it, int(conv)]
        assert float(fields[7]) > 0 and tri > 0 and 0 < T.nnz < s_ci.size
        w_rp, w_ci, wm, _ = bspgemm.readCOO(dst)
        assert wm == n and np.array_equal(w_rp, t_rp) and np.array_equal(w_ci, t_ci)
        A.free()
        T.free()
    finally:
        ctx.close()
    # without the output path nothing is written and the line is the same up to the time
    os.remove(dst)
    r2 = run(CLI, [src, str(k)])
    assert r2.returncode == 0 and r2.stdout.strip().split(",")[:7] == fields[:7] and not os.path.exists(dst)
