"""SpGEMM_hip_bc, the command-line driver of bspgemm_betweenness: on a small Matrix Market file of tests/golden (written from
gen.uniform(97, 3, 5950), `i j` for the edge i -> j) its lines equal what the numpy model gives on the FILE's orientation,
from seeded sources, from all of them and on the symmetrized graph; --out writes every vertex's fixed value; and the usage
line on bad arguments.
"""
import os

import numpy as np
import pytest

import gen
import bc_ref as B
from cli_kit import cli_path, run

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_bc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc_uniform97.mtx")


def _top(res, k):
    order = sorted(range(res["fixed"].size), key=lambda v: (-int(res["fixed"][v]), v))
    return [(v, int(res["fixed"][v]), float(res["bc"][v])) for v in order[:k]]


def _symmetrized(rp, ci, n):
    src, dst = B.edges(rp, ci, n)
    return B.canonical(*B.cc_ref.csr(np.concatenate([src, dst]), np.concatenate([dst, src]), n))


def test_the_golden_file_is_the_generated_graph():
    rp, ci, n = gen.uniform(97, 3, 5950)
    lines = open(GOLDEN).read().split("\n")
    assert lines[1] == "%d %d %d" % (n, n, ci.size)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert lines[2:2 + ci.size] == ["%d %d" % (r + 1, c + 1) for r, c in zip(rows.tolist(), ci.tolist())]


@pytest.mark.parametrize("args,symmetrize,sources,k", [
    ([], False, ("seeded", 8, 1), 10),
    (["--sources", "5", "--seed", "42", "--top", "4"], False, ("seeded", 5, 42), 4),
    (["--all", "--top", "97"], False, ("all",), 97),
    (["--all", "--symmetrize", "--top", "3"], True, ("all",), 3),
    (["--sources", "0"], False, ("seeded", 0, 1), 10),
])
def test_cli_matches_the_model(tmp_path, args, symmetrize, sources, k):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = gen.uniform(97, 3, 5950)
    if symmetrize:
        rp, ci, n = _symmetrized(rp, ci, n)
    else:                                             # the graph must tell an edge from its reverse
        back = B.model(*B.P.transposed(rp, ci, n), np.arange(n))
        assert not np.array_equal(back["fixed"], B.model(rp, ci, n, np.arange(n))["fixed"])
    src = np.arange(n) if sources[0] == "all" else B.cli_sources(n, sources[1], sources[2])
    res = B.model(rp, ci, n, src)
    out = str(tmp_path / "fixed.txt")
    r = run(CLI, [GOLDEN] + args + ["--out", out])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 + k, r.stdout
    head = lines[0].split(",")
    assert len(head) == 11 and float(head[10]) > 0, lines[0]
    nnz = B.edges(rp, ci, n)[0].size
    assert [int(x) for x in head[:10]] == [n, nnz, res["sources"], res["reached"], res["edges_forward"], res["hub_chunks"],
                                           res["depth_max"], res["levels"], res["sigma_max"], 0], lines[0]
    got = [(int(v), int(f), float(d)) for v, f, d in (ln.split(",") for ln in lines[1:])]
    assert got == _top(res, k), (got, _top(res, k))
    assert [int(x) for x in open(out).read().split()] == [int(x) for x in res["fixed"]]
    if src.size:
        assert res["fixed"].any()


@pytest.mark.parametrize("args", [[], ["--all"], ["g.mtx", "--sideways"], ["g.mtx", "--sources", "-3"], ["g.mtx", "--sources"],
                                  ["g.mtx", "--all", "--sources", "4"], ["g.mtx", "--top", "many"], ["g.mtx", "7"]])
def test_cli_prints_the_usage_line_on_bad_arguments(tmp_path, args):
    r = run(CLI, [a.replace("g.mtx", str(tmp_path / "none.mtx")) for a in args])
    assert r.returncode != 0 and "usage: SpGEMM_hip_bc" in r.stdout
