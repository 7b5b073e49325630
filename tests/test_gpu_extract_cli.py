"""The C command-line driver SpGEMM_hip_extract on a real GPU: the written file, read back by the loader, equals the model
of extract_ref.py, the two printed lines carry the shape, `kept` and the info fields, and a bad index ends the program with
a non-zero status and the library's message."""
import os

import numpy as np
import pytest

import bspgemm
import extract_ref as X
from cli_kit import assert_usage, cli_path, run

pytestmark = pytest.mark.gpu
EXE = cli_path("SpGEMM_hip_extract")
MTX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validity_test.mtx")


def _run(args):
    return run(EXE, args, timeout=300)


def _write(path, values):
    path.write_text("".join("%d\n" % v for v in values))
    return str(path)


@pytest.mark.parametrize("keep", [False, True])
def test_written_file_equals_the_model(tmp_path, keep):
    rp, ci, n, _ = bspgemm.readCOO(MTX)
    rng = np.random.default_rng(61)
    I, J = rng.integers(0, n, 9000), rng.permutation(n)[:20000]
    out = tmp_path / "out.mtx"
    r = _run([MTX, "--rows", _write(tmp_path / "rows.txt", I), "--cols", _write(tmp_path / "cols.txt", J)]
             + (["--keep-shape"] if keep else []) + ["-o", str(out)])
    assert r.returncode == 0, r.stderr
    m = X.model(rp, ci, n, n, I, J, keep)
    shape, info = [ln.split(",") for ln in r.stdout.strip().splitlines()]
    assert [int(x) for x in shape[:3]] == [m["shape"][0], m["shape"][1], m["kept"]] and float(shape[3]) > 0
    assert [int(x) for x in info[:2] + info[3:]] == [m[k] for k in ("scanned", "hub_chunks", "cols_monotone", "sorted_by",
                                                                    "canonicalised")]
    assert int(info[2]) in (4, 16, 64)
    assert m["kept"] > 0 and m["sorted_by"] == (0 if keep else 1)
    grp, gci, grows, gcols = bspgemm.readCOO(str(out))
    assert (grows, gcols) == (m["shape"][1], m["shape"][0])      # the file is the transposed operand: cols x rows
    rows = m["shape"][0]
    assert np.array_equal(np.asarray(grp[:rows + 1]), m["rp"]) and np.array_equal(np.asarray(gci), m["ci"])


def test_no_lists_and_a_bad_index(tmp_path):
    rp, ci, n, _ = bspgemm.readCOO(MTX)
    r = _run([MTX])
    assert r.returncode == 0, r.stderr
    m = X.model(rp, ci, n, n)
    assert r.stdout.splitlines()[0].split(",")[:3] == [str(n), str(n), str(m["kept"])]
    r = _run([MTX, "--rows", _write(tmp_path / "rows.txt", [0, n, 2])])
    assert r.returncode != 0 and "bspgemm_matrix_extract" in r.stderr and "I[1]" in r.stderr and "row list I" in r.stderr, r.stderr
    r = _run([MTX, "--cols", _write(tmp_path / "cols.txt", [4, 7, 4])])
    assert r.returncode != 0 and "twice" in r.stderr, r.stderr
    assert_usage(_run([MTX, "--rows"]), "usage: SpGEMM_hip_extract")
