"""The C command-line drivers on a real GPU: same positionals, messages and CSV fields as the
reference's binaries (final/SpGEMM_mpi_omp.c:294-366, final/SpGEMM_mpi_omp_validity.c:308-375)."""
import os
import subprocess

import pytest

from cli_kit import assert_missing_file, assert_usage

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "binary-spgemm_amd")
MTX = os.path.join(ROOT, "tests", "golden", "validity_test.mtx")


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=300, **kw)


def test_validity_driver_prints_the_reference_message():
    """`make test` of the reference: mpirun -n 4 SpGEMM_mpi_omp_validity validity_test.mtx 6250 2"""
    r = _run([os.path.join(PKG, "SpGEMM_hip_validity"), MTX, "6250", "2"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "Results of serial and multricore are the same!"


def test_bench_driver_csv_line():
    r = _run([os.path.join(PKG, "SpGEMM_hip"), MTX, "6250", "2", "5"])
    assert r.returncode == 0, r.stderr
    f = r.stdout.strip().split(",")
    # tasks,threads,tasks*threads,tBlock,path,n,nnz(A),nnz(C),mean,median,fastest + 5 extra columns
    assert len(f) == 16
    assert f[:4] == ["1", "2", "2", "6250"] and f[4] == MTX
    assert f[5:8] == ["50000", "25000", "12502"]
    assert all(float(x) > 0 for x in f[8:11]) and float(f[10]) <= float(f[9])


def test_bench_driver_usage_and_bad_file(tmp_path):
    assert_usage(_run([os.path.join(PKG, "SpGEMM_hip")]), "usage: mpirun  -n  numtasks  SpGEMM_mpi_omp")
    bad = tmp_path / "bad.mtx"
    bad.write_text("%MatrixMarket matrix coordinate pattern general\n1 1 1\n1 1\n")
    r = _run([os.path.join(PKG, "SpGEMM_hip"), str(bad), "1", "1", "1"])
    assert r.returncode == 1 and "Could not process Matrix Market banner." in r.stdout
    assert_missing_file(_run([os.path.join(PKG, "SpGEMM_hip"), str(tmp_path / "missing.mtx"), "1", "1", "1"]))
    # a good banner with a bad size line: the reference exits 1 WITHOUT a message (final/utils.c:60-61)
    bad.write_text("%%MatrixMarket matrix coordinate pattern general\n% a comment\nthree by three\n")
    for exe, extra in (("SpGEMM_hip", ["1", "1", "1"]), ("SpGEMM_hip_validity", ["1", "1"])):
        r = _run([os.path.join(PKG, exe), str(bad)] + extra)
        assert r.returncode == 1 and r.stdout == "", (exe, r.stdout, r.stderr)


MPIRUN = "/opt/conda/bin/mpirun"


def _mpirun(n, args):
    env = dict(os.environ, PATH="/opt/conda/bin:" + os.environ.get("PATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    return _run([MPIRUN, "-n", str(n)] + args, env=env)


def _need_mpirun(exe):
    if not (os.path.exists(exe) and os.path.exists(MPIRUN)):
        pytest.skip("MPI not available")
    r = _mpirun(2, ["/bin/true"])
    if r.returncode != 0:
        pytest.skip("mpirun cannot start processes on this box: " + r.stderr[-200:])


def test_validity_mpi_four_ranks_is_make_test():
    """the reference's `make test` itself (final/Makefile:11-12): mpirun -n 4 <validity binary>
    validity_test.mtx 6250 2.  Four ranks on the box's one GPU: SpGEMM_hip_multi over the MPI host
    transport (equal-work shards, all-gathered row lengths, col_idx gathered on rank 0), compared on
    rank 0 with the whole product (final/SpGEMM_mpi_omp_validity.c:331-343)."""
    exe = os.path.join(PKG, "SpGEMM_hip_validity_mpi")
    _need_mpirun(exe)
    r = _mpirun(4, [exe, MTX, "6250", "2"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "Results of serial and multricore are the same!", r.stdout + r.stderr
    # one rank: the RCCL transport (a communicator of one) runs the same calls
    r = _mpirun(1, [exe, MTX, "6250", "2"])
    assert r.returncode == 0 and r.stdout.strip() == "Results of serial and multricore are the same!", r.stdout + r.stderr


def test_mpi_driver_three_ranks_host_transport(tmp_path):
    """the bench driver under mpirun -n 3 on one GPU: three ragged equal-work shards, C.row_ptr
    stitched through bspgemm_comm_stitch_row_ptr (lengths all-gathered by MPI_Allgather); the total
    nnz it prints is the product's"""
    import bspgemm
    import gen
    from oracle import oracle as O
    exe = os.path.join(PKG, "SpGEMM_hip_mpi")
    _need_mpirun(exe)
    rp, ci, n = gen.rmat(12, 8, (0.57, 0.19, 0.19, 0.05), seed=77)          # skewed: shards differ in rows
    p = str(tmp_path / "g.mtx")
    bspgemm.write_mtx(p, rp, ci)
    erp, _ = O.spgemm(rp, ci, rp, ci, n)
    r = _mpirun(3, [exe, p, "64", "1", "2"])
    assert r.returncode == 0, r.stderr
    f = r.stdout.strip().split(",")
    assert f[0] == "3" and int(f[7]) == int(erp[-1]), r.stdout


def test_mpi_driver_single_rank():
    """the MPI+RCCL build, one rank (singleton init, no mpirun needed)"""
    exe = os.path.join(PKG, "SpGEMM_hip_mpi")
    if not os.path.exists(exe):
        pytest.skip("MPI not available at build time")
    r = _run([exe, MTX, "6250", "2", "3"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().split(",")[7] == "12502"


def test_bench_driver_a_times_b_with_output(tmp_path):
    """optional positionals: file-orientation A*B of rectangular files, C written"""
    import numpy as np
    import scipy.sparse as sp
    import bspgemm
    rng = np.random.default_rng(3)
    A = sp.random(120, 80, density=0.05, random_state=rng, format="csr")
    B = sp.random(80, 200, density=0.04, random_state=rng, format="csr")
    for name, M in (("a.mtx", A), ("b.mtx", B)):
        T = M.T.tocsr()                      # write_mtx takes the loader's (transposed) CSR
        T.sort_indices()
        bspgemm.write_mtx(str(tmp_path / name), T.indptr, T.indices, cols=M.shape[0])
    out = str(tmp_path / "c.mtx")
    r = _run([os.path.join(PKG, "SpGEMM_hip"), str(tmp_path / "a.mtx"), "1", "1", "2", str(tmp_path / "b.mtx"), out])
    assert r.returncode == 0, r.stderr
    Cref = ((A != 0).astype(np.int32) @ (B != 0).astype(np.int32)).tocsr()
    assert int(r.stdout.strip().split(",")[7]) == Cref.nnz
    rp, ci, m, n = bspgemm.readCOO(out)      # loader view = C^T as CSR
    assert (m, n) == (120, 200)
    CT = Cref.T.tocsr()
    CT.sort_indices()
    assert np.array_equal(rp, CT.indptr) and np.array_equal(ci, CT.indices)


def test_closure_driver(tmp_path):
    import numpy as np
    import bspgemm
    n = 500
    rng = np.random.default_rng(8)
    # a ring plus a few chords: the closure is the full matrix, reached in ~log2(n) squarings
    rows = np.concatenate([np.arange(n), rng.integers(0, n, 20)])
    cols = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, 20)])
    import gen
    rp, ci = gen._csr_from_pairs(rows, cols, n)
    bspgemm.write_mtx(str(tmp_path / "g.mtx"), rp, ci)
    r = _run([os.path.join(PKG, "SpGEMM_hip_closure"), str(tmp_path / "g.mtx"), str(tmp_path / "t.mtx")])
    assert r.returncode == 0, r.stderr
    f = r.stdout.strip().split(",")
    assert int(f[1]) == n and int(f[4]) == n * n and 1 <= int(f[3]) <= 12
    trp, tci, _, _ = bspgemm.readCOO(str(tmp_path / "t.mtx"))
    assert trp[-1] == n * n and np.array_equal(tci[:n], np.arange(n))


def test_reference_validity_driver_certifies_the_dropin():
    """The REFERENCE's own validity program on top of the library (VERDICT r3 missing #2): oracle/Makefile pipes the
    untouched final/SpGEMM_mpi_omp_validity.c through the one-token substitution of INTEGRATION.md 1a (`SpGEMM_omp(` at
    :171 -> `SpGEMM_hip(`; nothing of the source is stored) and links libbspgemm.so + MPICH into
    oracle/_ref/SpGEMM_mpi_omp_validity_hip.  Under the reference's `make test` command line (final/Makefile:11-12)
    every MPI rank computes its row block on the GPU through the int32 drop-in, the reference's own MPI gathers and
    rebase (:178-223) assemble C, and then the reference's own serial CPU kernel (SpGEMM_bigslice, :337) and its own
    comparator (SpGEMM_valid, :290-302) decide.  Built only where /root/reference exists; travels to the GPU box as a
    binary like the rest of oracle/_ref."""
    exe = os.path.join(ROOT, "oracle", "_ref", "SpGEMM_mpi_omp_validity_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/SpGEMM_mpi_omp_validity_hip not built (no reference checkout where this tree was built)")
    _need_mpirun(exe)
    for ranks, tblock in ((4, "6250"), (2, "5000"), (1, "50000")):
        r = _mpirun(ranks, [exe, MTX, tblock, "2"])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Results of serial and multricore are the same!" in r.stdout, (ranks, r.stdout + r.stderr)
        assert "dont match" not in r.stdout
