"""The tests' model of the submatrix extraction (extract_ref.py) against a naive model of the definition on hand-worked
examples, and the edge graphs of test_gpu_extract.py against what they claim to reach: row lengths, kept counts, chunk
counts, the sort class of every out row and the idle lanes of the last workgroup, all computed from the model.  No GPU.
"""
import numpy as np
import pytest

import gen
import extract_ref as X


def _same(rp, ci, rows, cols, I=None, J=None, keep_shape=False):
    m = X.model(rp, ci, rows, cols, I, J, keep_shape)
    nrp, nci = X.naive(rp, ci, rows, cols, I, J, keep_shape)
    assert m["rp"].tolist() == nrp and m["ci"].tolist() == nci, (I, J, keep_shape)
    assert m["kept"] == len(nci)
    return m


# A = [[0 1 1 0], [1 0 0 1], [0 0 1 0]], worked by hand
HAND = (np.array([0, 2, 4, 5], np.int32), np.array([1, 2, 0, 3, 2], np.int32), 3, 4)


def test_hand_worked_examples():
    rp, ci, rows, cols = HAND
    m = _same(rp, ci, rows, cols, I=[2, 0, 0], J=[2, 1])       # repeated and unsorted I, an unsorted J
    assert m["rp"].tolist() == [0, 1, 3, 5] and m["ci"].tolist() == [0, 0, 1, 0, 1] and m["shape"] == (3, 2)
    assert (m["scanned"], m["cols_monotone"], m["sorted_by"], m["hub_chunks"], m["canonicalised"]) == (5, 0, 1, 0, 0)
    m = _same(rp, ci, rows, cols, J=[3, 2, 1, 0])               # reversed J
    assert m["rp"].tolist() == [0, 2, 4, 5] and m["ci"].tolist() == [1, 2, 0, 3, 1] and m["sorted_by"] == 1
    m = _same(rp, ci, rows, cols)                               # both NULL
    assert m["rp"].tolist() == rp.tolist() and m["ci"].tolist() == ci.tolist() and m["cols_monotone"] == 1
    assert (m["scanned"], m["kept"], m["sorted_by"]) == (5, 5, 0)
    m = _same(rp, ci, rows, cols, I=[], J=[1, 2])               # an empty list
    assert m["shape"] == (0, 2) and m["kept"] == 0 and m["scanned"] == 0 and m["rp"].tolist() == [0]
    m = _same(rp, ci, rows, cols, I=[0, 1], J=[])
    assert m["shape"] == (2, 0) and m["kept"] == 0 and m["scanned"] == 4
    m = _same(rp, ci, rows, cols, I=[1, 1, 0], J=[3, 0, 0], keep_shape=True)     # repeats are harmless
    assert m["rp"].tolist() == [0, 0, 2, 2] and m["ci"].tolist() == [0, 3] and m["shape"] == (3, 4)
    assert (m["scanned"], m["cols_monotone"], m["sorted_by"]) == (4, 1, 0)


def test_rectangular_and_untidy_operands():
    rp, ci = gen.uniform_rect(300, 200, 5, seed=3)
    rng = np.random.default_rng(4)
    I, J = rng.integers(0, 300, 120), rng.permutation(200)[:77]
    for keep in (False, True):
        m = _same(rp, ci, 300, 200, I, J, keep)
        assert m["canonicalised"] == 0 and m["shape"] == ((300, 200) if keep else (120, 77))
    rp, ci, n = gen.dups_unsorted(96, 6, seed=9)
    assert not X.is_canonical(rp, ci)
    crp, cci = X.canonical(rp, ci, n, n)
    assert X.is_canonical(crp, cci) and cci.size < ci.size
    p = rng.permutation(n)
    for keep in (False, True):
        m = _same(rp, ci, n, n, p, p, keep)
        assert m["canonicalised"] == 1
        assert m["scanned"] == cci.size                         # the lengths of the canonical rows
    m = _same(rp, ci, n, n)
    assert m["rp"].tolist() == crp.tolist() and m["ci"].tolist() == cci.tolist()


def test_lane_graph_reaches_its_edges():
    rp, ci, rows, cols, I, J = X.lane_case()
    assert X.is_canonical(rp, ci) and ci.max() < cols and rows == len(X.LANE_LENGTHS) * len(X.LANE_PATTERNS)
    m = _same(rp, ci, rows, cols, I, J)
    lens = np.diff(rp)
    for W in (4, 16, 64):
        for n in (0, 1, W - 1, W, W + 1, 63, 64, 65):
            assert n in lens, (W, n)
    kept = m["kept_rows"][:rows].reshape(len(X.LANE_LENGTHS), len(X.LANE_PATTERNS))
    for a, n in enumerate(X.LANE_LENGTHS):
        assert kept[a].tolist() == [0, n, min(n, 1), min(n, 1), (n + 1) // 2], n
    first = m["ci"][m["rp"][:-1][m["kept_rows"] > 0]]
    assert 0 in first and first.max() == 64                     # "last only" of the 65-entry row: the kept entry is the last
    assert I.size == X.LANE_NI and m["hub_chunks"] == 0 and m["cols_monotone"] == 1
    for W in (4, 16, 64):
        tail = (X.LANE_NI * W) % X.THREADS                      # threads of the last workgroup that have a row
        assert 0 < tail <= X.THREADS - 64, (W, "the last workgroup has no idle wave")
        if W < 64:
            assert tail % 64 != 0, (W, "the last busy wave has no idle group")
    assert X.lanes_auto(m["scanned"], I.size) in (4, 16)


def test_hub_graph_reaches_its_edges():
    rp, ci, rows, cols, I, J = X.hub_case()
    assert X.is_canonical(rp, ci) and ci.max() < cols <= 21000 and np.unique(J).size == J.size
    lens = np.diff(rp)
    C = X.HUB_CHUNK
    assert lens[:4].tolist() == [C, C + 1, 2 * C, 2 * C + 1] and X.chunks_of(lens[:4]).tolist() == [0, 2, 2, 3]
    m = _same(rp, ci, rows, cols, I, J)
    assert m["hub_chunks"] == int(X.chunks_of(lens[I]).sum()) == 2 + 2 + 3 + 2 + 3 + 3 + 2
    assert np.count_nonzero(I == 3) == 2 and X.chunks_of(lens[I[-1]]) > 0                  # a hub twice, a hub last
    jset = np.zeros(cols, bool)
    jset[J] = True

    def chunk_kept(r):
        flags = jset[ci[rp[r]:rp[r + 1]]]
        return [int(flags[b:b + C].sum()) for b in range(0, flags.size, C)], flags

    per, flags = chunk_kept(X.HUB_ROWS["len8193"])
    assert flags[C - 6:C + 6].all() and flags[2 * C - 6:2 * C + 1].all()                   # kept runs across both borders
    assert per[2] == 1                                                                   # the one-entry last chunk is kept
    assert chunk_kept(X.HUB_ROWS["nothing_kept"])[0] == [0, 0] and m["kept_rows"][4] == 0
    per, _ = chunk_kept(X.HUB_ROWS["empty_middle_chunk"])
    assert per[0] > 0 and per[1] == 0 and per[2] > 0
    assert m["kept_rows"][7] == m["kept_rows"][3] > 0                                      # the hub named twice: two copies
    k = _same(rp, ci, rows, cols, I, J, keep_shape=True)
    assert k["hub_chunks"] == m["hub_chunks"] - 3 and k["scanned"] == m["scanned"] - lens[3]  # a row counts once
    assert k["cols_monotone"] == 1 and k["sorted_by"] == 0


def test_sort_graph_reaches_its_classes():
    rng = np.random.default_rng(11)
    for fallback in (False, True):
        rp, ci, rows, cols = X.sort_case(fallback)
        assert X.is_canonical(rp, ci)
        for J in (np.arange(cols)[::-1], rng.permutation(cols)):
            m = X.model(rp, ci, rows, cols, None, J)
            assert m["kept_rows"].tolist() == list(X.SORT_KEPT) + ([X.SORT_BLOCK + 1] if fallback else [])
            assert [X.sort_class(k) for k in m["kept_rows"]] == [0, 1, 1, 1, 2, 2, 2] + ([3] if fallback else [])
            assert m["cols_monotone"] == 0 and m["sorted_by"] == (2 if fallback else 1)
            assert X.is_canonical(m["rp"], m["ci"])
        lens = np.diff(rp)
        assert (X.chunks_of(lens) > 0).tolist() == [False] * 7 + ([True] if fallback else [])   # 4096 is no hub, 4097 is
        m = X.model(rp, ci, rows, cols, None, np.arange(0, cols, 7))
        assert m["cols_monotone"] == 1 and m["sorted_by"] == 0 and 0 < m["kept"] < ci.size // 5
    rp, ci, rows, cols = X.sort_case()
    nrp, nci = X.naive(rp[:5], ci[:rp[4]], 4, cols, None, np.arange(cols)[::-1])
    m = X.model(rp[:5], ci[:rp[4]], 4, cols, None, np.arange(cols)[::-1])
    assert m["rp"].tolist() == nrp and m["ci"].tolist() == nci


@pytest.mark.parametrize("scanned,rows,lanes", [(0, 0, 4), (16 * 70, 70, 4), (16 * 70 + 1, 70, 16), (64 * 70, 70, 16),
                                                (64 * 70 + 1, 70, 64)])
def test_automatic_lanes_rule(scanned, rows, lanes):
    assert X.lanes_auto(scanned, rows) == lanes
