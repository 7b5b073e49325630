"""SpGEMM_hip_pagerank, the command-line driver of bspgemm_pagerank: on a Matrix Market file written here entry by entry,
`i j` for the edge i -> j, of a graph where the direction matters (stars into one vertex), its lines equal what the numpy
model gives on the FILE's orientation under --pull and --push; --symmetric on a file that holds every edge both ways; a
tolerance; and the usage line on bad arguments.
"""
import os

import pytest

import pagerank_ref as P
from cli_kit import cli_path, run, write_edges

pytestmark = pytest.mark.gpu
CLI = cli_path("SpGEMM_hip_pagerank")


def _top(res, k):
    order = sorted(range(res["fixed"].size), key=lambda v: (-int(res["fixed"][v]), v))
    return [(v, int(res["fixed"][v]), float(res["rank"][v])) for v in order[:k]]


@pytest.mark.parametrize("name,args,iterations,damping,tolerance,k", [
    ("sink_star_256", ["--pull"], 20, 0.85, 0.0, 10),
    ("sink_star_256", ["--push"], 20, 0.85, 0.0, 10),
    ("sink_star_256", ["7", "0.5", "--top", "4"], 7, 0.5, 0.0, 4),
    ("sink_star_256", ["100", "--tolerance", "1e-9", "--push"], 100, 0.85, 1e-9, 10),
    ("symmetric_rmat9", ["--symmetric"], 20, 0.85, 0.0, 10),
    ("symmetric_rmat9", ["--symmetric", "--push", "--top", "3"], 20, 0.85, 0.0, 3),
])
def test_cli_matches_the_model(tmp_path, name, args, iterations, damping, tolerance, k):
    assert os.path.exists(CLI), "%s is not built" % CLI
    rp, ci, n = P.graph(name)
    res = P.pagerank(rp, ci, n, damping, iterations, tolerance)
    if name == "sink_star_256":                       # the graph must tell an edge from its reverse
        back = P.pagerank(*P.transposed(rp, ci, n), damping, iterations, tolerance)
        assert [t[0] for t in _top(back, k)] != [t[0] for t in _top(res, k)]
    src = str(tmp_path / "graph.mtx")
    write_edges(src, rp, ci, n)
    r = run(CLI, [src] + args)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 + k, r.stdout
    head = lines[0].split(",")
    assert len(head) == 7 and float(head[6]) > 0, lines[0]
    assert [int(x) for x in head[:6]] == [n, ci.size, res["dangling"], res["iterations"], res["delta"], res["mass"]], lines[0]
    if tolerance:
        assert 1 < res["iterations"] < iterations
    got = [(int(v), int(f), float(d)) for v, f, d in (ln.split(",") for ln in lines[1:])]
    assert got == _top(res, k), (got, _top(res, k))


@pytest.mark.parametrize("args", [[], ["g.mtx", "--sideways"], ["g.mtx", "-3"], ["g.mtx", "20", "1.5"], ["g.mtx", "20", "0.85", "9"],
                                  ["g.mtx", "--tolerance"], ["g.mtx", "--top", "many"], ["g.mtx", "2.5"]])
def test_cli_prints_the_usage_line_on_bad_arguments(tmp_path, args):
    r = run(CLI, [a.replace("g.mtx", str(tmp_path / "none.mtx")) for a in args])
    assert r.returncode != 0 and "usage: SpGEMM_hip_pagerank" in r.stdout
