"""What the tools/*_time.py share: the import order, the one definition of "time a call", the line that reports it, the capture
of the library's timing lines, the second context that prints them, and the host baseline beside a device call.
    import timing_common            (first; the script's directory is on sys.path when a tool is run as documented)
Importing it puts binary-spgemm_amd/ and tests/ on sys.path and imports torch before bspgemm: one HIP runtime in the process."""
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-spgemm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (first: one HIP runtime in the process)
import numpy as np  # noqa: E402
import bspgemm  # noqa: E402


def wall_ms(ctx, fn, reps, warm=1):
    """wall times in ms of `reps` calls of fn(), each between two synchronisations of ctx; the first call is the warm-up
    (warm = 0: none).  What fn() returns, if anything, is the handles to free outside the timed window."""
    out = []
    for i in range(1 - warm, reps + 1):
        ctx.synchronize()
        t = time.perf_counter()
        hs = fn()
        ctx.synchronize()
        if i:
            out.append((time.perf_counter() - t) * 1e3)
        for h in hs or ():
            h.free()
    return out


def line(name, ms, extra=""):
    return "%-60s min %10.3f ms  median %10.3f ms%s" % (name, min(ms), statistics.median(ms), extra)


def show(name, ms, extra=""):
    """prints the label, the minimum and the median of the times, and `extra` behind them; returns the minimum"""
    print(line(name, ms, extra), flush=True)
    return min(ms)


def stderr_of(fn):
    """what fn() writes to file descriptor 2 (the library's timing lines)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def timed_context(env_name, value="1"):
    """a second context created under the environment variable `env_name` (a BSPGEMM_*_TIMING switch: read once, in
    bspgemm_create, so it holds for this context alone)"""
    os.environ[env_name] = value
    try:
        return bspgemm.Context(0)
    finally:
        del os.environ[env_name]


def host_baseline(label, fn, limit, nnz, whole, got=None, indent="      ", check_label=None):
    """One host baseline beside a device call that took `whole` ms: fn() runs once and is timed, unless the operand has more
    than `limit` stored entries.  got (under --check): what the device gave, compared with what fn() returns -- an array, or
    a function of fn()'s result that says whether they agree.  Returns False if they were compared and differ."""
    if nnz > limit:
        print("%sbaseline: download + %s: not run (more than %d stored entries)" % (indent, label, limit), flush=True)
        return True
    t = time.perf_counter()
    exp = fn()
    ms = (time.perf_counter() - t) * 1e3
    print("%s%-50s     %10.3f ms  (once): %.0f x the whole call" % (indent, "baseline: download + " + label, ms, ms / whole),
          flush=True)
    if got is None:
        return True
    same = bool(got(exp) if callable(got) else np.array_equal(got, exp))
    print("%scheck against %s: %s" % (indent, check_label or label, "equal" if same else "DIFFERENT"), flush=True)
    return same
