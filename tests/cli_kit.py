"""What the tests of the command-line drivers (test_gpu_*cli.py) share (no tests in here): where a driver is, how it is
run, the Matrix Market pattern file they feed it, and the three endings that every driver has: the usage line, a missing
file, and a matrix that is not square.
"""
import os
import subprocess

import numpy as np

import bspgemm


def cli_path(name):
    """the driver `name` ("SpGEMM_hip_cc"), next to the library"""
    return os.path.join(os.path.dirname(bspgemm.LIB_PATH), name)


def run(exe, args, timeout=120):
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=timeout)


def write_edges(path, rp, ci, rows, cols=None):
    """the CSR (rp, ci) of rows x cols (cols: rows when None) as a `general` pattern file, entry by entry, 1-based"""
    r = np.repeat(np.arange(rows), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate pattern general\n%d %d %d\n" % (rows, rows if cols is None else cols, ci.size))
        f.write("".join("%d %d\n" % (a + 1, b + 1) for a, b in zip(r.tolist(), ci.tolist())))


def assert_usage(r, usage, what=None):
    """the usage line starts stdout, exit status 1; what: the arguments, for the message"""
    assert r.returncode == 1 and r.stdout.startswith(usage), (what, r.stdout)


def assert_missing_file(r):
    """the loader's silent exit(1)"""
    assert r.returncode == 1 and r.stdout == ""


def assert_not_square(r, word, shape="2x3"):
    """word: the driver's word for itself, as it passes it to cli_need_square"""
    assert r.returncode == 1 and r.stdout == "" and "%s needs a square matrix (%s)" % (word, shape) in r.stderr, (r.stdout, r.stderr)
