"""bench.py's two kinds of run on its default one-GPU workload: a plain run prints the headline and what its timed
steps recorded, and spends little time outside them; --full adds the extras (roofline on two class-timed steps,
the drop-in) to the same line."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 2, 3
PLAIN_OUTSIDE_STEPS_S = 30.0                         # what a plain run may spend outside its warm-up and timed steps


def _bench(*extra):
    """one bench.py process: (its JSON line, its wall time from start to exit in seconds)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
           "--warmup", str(WARMUP)] + list(extra)
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout                 # ONE JSON line on stdout
    return json.loads(lines[0]), wall


def test_plain_run_leaves_the_extras_to_full(tmp_path):
    plain, wall = _bench("--dump-outputs", str(tmp_path / "plain"))
    outside = wall - (STEPS + WARMUP) * plain["ms_per_step"] * 1e-3
    assert outside < PLAIN_OUTSIDE_STEPS_S, "a plain run spent %.1f s outside its steps" % outside
    full, _ = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for r in (plain, full):
        assert (r["metric"], r["unit"], r["higher_is_better"], r["dtype"]) == ("output nnz/sec (GNZ/s)", "GNZ/s", True, "int32")
        assert r["value"] > 0 and r["ms_per_step"] > 0 and (r["steps"], r["warmup"]) == (STEPS, WARMUP)
        assert r["whole_job"]["rank0_ms"]["total"] > 0
    assert plain["config"] == dict(full["config"], full=False) and full["config"]["full"] is True

    assert not {"roofline", "dropin_e2e", "cpu_baseline"} & set(plain)
    assert not {"rank0_ms_per_bin", "pmc_step_traffic_bytes"} & set(plain["whole_job"])

    assert "error" not in full["roofline"] and full["roofline"]["instances"], full["roofline"]
    assert len(full["whole_job"]["rank0_ms_per_bin"]) == len(full["whole_job"]["bin_cap"])
    assert full["dropin_e2e"]["nnz_c"] == full["config"]["nnz_c"], full["dropin_e2e"]
    assert "cpu_baseline" not in full                # --no-cpu-baseline still holds under --full

    for name in ("C_row_ptr.npy", "C_col_idx.npy", "C_col_idx_index.npy"):   # both kinds dump the same C
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "full" / name).read_bytes()
