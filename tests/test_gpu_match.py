"""The device-resident maximal matching (bspgemm_maximal_matching): the mates (through mate_host and through P), the labels
and every field of the info against the numpy model of match_ref.py, bit for bit, under all three orders.

What can go wrong is the round: the wave-aggregated appends of the pair launch (the spiders: 63, 65 and 257 vertices kept at
once), 4999 retirements in one launch and 5000 candidates that point at one vertex (the stars), long runs of tiny rounds
and vertex counts that are no multiple of 4, 64 or 256 (the paths and the chains), the groups of 4, 16 and 64 lanes on rows
of W - 1, W and W + 1 entries (the cliques, under every BSPGEMM_OPT_MATCH_LANES), and the hub chunks: a row of exactly the
chunk size and one more, the winner in the first, a middle and the last chunk (whose only entry it is), two adjacent hubs,
and a hub that stays live for three rounds -- each at the smallest size that still has the property.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bspgemm
import cc_ref
import gen
import match_ref
import scc_ref

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
SEED = 11
NAME = "bspgemm_maximal_matching"
INFO = ("pairs", "entries_walked", "hub_chunks", "rounds", "lanes")


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(rp, ci, n) of the named graph; computed once"""
    return (match_ref.GRAPHS.get(name) or match_ref.GROUP_GRAPHS.get(name) or match_ref.HUB_GRAPHS[name])()


@functools.lru_cache(maxsize=None)
def _expected(name, order, seed=SEED):
    """the model's Matching; computed once and read-only"""
    r = match_ref.matching(*_graph(name), order=order, seed=seed)
    r.mate.setflags(write=False)
    r.labels.setflags(write=False)
    return r


def _check(ctx, A, exp, order, seed=SEED, lanes=0, what=""):
    """run the call on operand A and compare everything; returns (mate, info)"""
    n = exp.mate.size
    P, mate, info = ctx.maximal_matching(A, order, seed, mate=True)
    try:
        assert (P.rows, P.cols, P.nnz) == (n, n, n), what
        rp, labels = P.download()
        assert rp.dtype == np.int32 and np.array_equal(rp, np.arange(n + 1)), what
        assert mate.dtype == np.int32 and np.array_equal(mate, exp.mate), (what, order, np.flatnonzero(mate != exp.mate)[:8])
        assert labels.dtype == np.int32 and np.array_equal(labels, exp.labels), (what, order, np.flatnonzero(labels != exp.labels)[:8])
        want = exp._replace(lanes=lanes if lanes and exp.rounds else exp.lanes)
        for k in INFO:
            assert info[k] == getattr(want, k), (what, order, k, info[k], getattr(want, k))
    finally:
        P.free()
    return mate, info


# ---------------------------------------------------------------- 1. every named graph against the model --------------
@pytest.mark.parametrize("name", match_ref.SMALL)
def test_mates_equal_the_model(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for order in match_ref.ORDERS:
            mate, info = _check(ctx, A, _expected(name, order), order, what=name)
            if name.startswith("empty") or name == "self_loop":
                assert (mate == -1).all() and not any(info.values())
    finally:
        A.free()


def test_the_stars_and_the_path_take_the_rounds_they_are_built_for():
    for star in ("star_hub_last", "star_hub_middle", "star_leaf_rows"):
        assert (_expected(star, "random").rounds, _expected(star, "random").pairs) == (2, 1)
    assert (_expected("path200", "natural").rounds, _expected("path200", "natural").pairs) == (100, 100)
    assert _expected("chains4099", "natural").rounds == 684


# ---------------------------------------------------------------- 2. the lane groups -----------------------------------
@pytest.mark.parametrize("name", list(match_ref.GROUP_GRAPHS))
def test_rows_around_the_group_width_under_every_lanes(ctx, name):
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for lanes in match_ref.LANES:
            ctx.set_option("match_lanes", lanes)
            for order in match_ref.ORDERS:
                _, info = _check(ctx, A, _expected(name, order), order, lanes=lanes, what=(name, lanes))
                assert info["lanes"] == (lanes or _expected(name, order).lanes)
    finally:
        ctx.set_option("match_lanes", 0)
        A.free()
    # the automatic choice: a quarter of the mean degree, so every width runs once
    assert [_expected(g, "random").lanes for g in match_ref.GROUP_GRAPHS] == [4, 16, 64]


# ---------------------------------------------------------------- 3. the hub chunks ------------------------------------
@pytest.mark.parametrize("name", list(match_ref.HUB_GRAPHS))
def test_hub_chunks(ctx, name):
    rp, ci, n = _graph(name)
    if name == "hub_live3":                                  # the hub is live in all three rounds: two records in each
        e = _expected(name, "natural")
        assert (e.rounds, e.hub_chunks) == (3, 6) and e.mate[n - 1] == -1
    if name == "two_hubs":                                   # the hubs see each other's (long) rows
        assert [_expected(name, order).hub_chunks for order in match_ref.ORDERS] == [4, 4, 4]
    A = ctx.upload(rp, ci, n)
    try:
        for lanes in (0, 64):
            ctx.set_option("match_lanes", lanes)
            for order in match_ref.ORDERS:
                _check(ctx, A, _expected(name, order), order, lanes=lanes, what=(name, lanes))
    finally:
        ctx.set_option("match_lanes", 0)
        A.free()


def test_the_chunk_size_is_the_models(ctx):
    """a row of CHUNK entries is walked by its group, one of CHUNK + 1 entries by two chunk records"""
    got = []
    for name in ("star_chunk", "star_chunk_plus_1"):
        rp, ci, n = _graph(name)
        assert np.diff(match_ref.simple(rp, ci, n)[0]).max() == match_ref.CHUNK + (name != "star_chunk")
        A = ctx.upload(rp, ci, n)
        try:
            got.append(_check(ctx, A, _expected(name, "random"), "random", what=name)[1]["hub_chunks"])
        finally:
            A.free()
    assert got == [0, 2]


def test_the_winner_in_the_first_a_middle_and_the_last_chunk(ctx):
    name, leaves = "star_2chunks_plus_1", 2 * match_ref.CHUNK + 1
    rp, ci, n = _graph(name)
    for c, seed in match_ref.CHUNK_SEEDS.items():           # the coverage, from the model, before anything runs
        winner = match_ref.hub_winner(leaves, seed)
        assert winner // match_ref.CHUNK == c and _expected(name, "random", seed).mate[leaves] == winner, (c, seed, winner)
    assert match_ref.hub_winner(leaves, match_ref.CHUNK_SEEDS[2]) == leaves - 1      # the last chunk's only entry
    A = ctx.upload(rp, ci, n)
    try:
        for seed in match_ref.CHUNK_SEEDS.values():
            _check(ctx, A, _expected(name, "random", seed), "random", seed=seed, what=(name, seed))
    finally:
        A.free()


# ---------------------------------------------------------------- 4. the input forms -----------------------------------
def test_input_forms_give_identical_bits(ctx):
    """A, its transpose (the in-edges), A with shuffled rows and repeats, and the strict lower triangle of S alone"""
    name = "rmat12"
    rp, ci, n = _graph(name)
    srp, sci = match_ref.simple(rp, ci, n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    rng = np.random.default_rng(5450)
    again = rng.random(ci.size) < 0.3
    r2, c2 = np.concatenate([rows, rows[again]]), np.concatenate([ci, ci[again]])
    mix = rng.permutation(r2.size)
    s_rows = np.repeat(np.arange(n), np.diff(srp))
    low = sci < s_rows
    forms = {"A": (rp, ci), "transpose": scc_ref.transposed(rp, ci, n)[:2], "shuffled with repeats": cc_ref.csr(r2[mix], c2[mix], n)[:2],
             "strict lower triangle": cc_ref.csr(s_rows[low], sci[low], n)[:2]}
    for what, (f_rp, f_ci) in forms.items():
        M = ctx.upload(np.ascontiguousarray(f_rp, np.int32), np.ascontiguousarray(f_ci, np.int32), n)
        try:
            for order in match_ref.ORDERS:
                _check(ctx, M, _expected(name, order), order, what=what)
        finally:
            M.free()
    A = ctx.upload(rp, ci, n)
    T = ctx.transpose(A)
    S = ctx.symmetrize(A, drop_diagonal=True)
    try:
        for M, what in ((T, "device transpose"), (S, "symmetrized")):
            _check(ctx, M, _expected(name, "light"), "light", what=what)
    finally:
        for h in (S, T, A):
            h.free()


# ---------------------------------------------------------------- 5. the option, seeds, repeatability ------------------
def test_match_lanes_option(ctx):
    for bad in (-1, 1, 8, 32, 65, 128):
        with pytest.raises(bspgemm.BspgemmError):
            ctx.set_option("match_lanes", bad)
    assert ctx.get_option("match_lanes") == 0
    ctx.set_option("match_lanes", 16)
    assert ctx.get_option("match_lanes") == 16
    ctx.set_option("match_lanes", 0)
    assert ctx.get_option("match_lanes") == 0


def test_seeds_and_repeatability(ctx):
    name = "rmat12"
    rp, ci, n = _graph(name)
    A = ctx.upload(rp, ci, n)
    try:
        for order in ("random", "light"):
            a = _check(ctx, A, _expected(name, order, 1), order, seed=1, what="seed 1")
            b = _check(ctx, A, _expected(name, order, 2), order, seed=2, what="seed 2")
            assert not np.array_equal(a[0], b[0]), order
        big = _check(ctx, A, _expected(name, "random", 0xFFFFFFFF), "random", seed=0xFFFFFFFF, what="seed 2^32 - 1")
        assert not np.array_equal(big[0], _expected(name, "random", 1).mate)
        x = _check(ctx, A, _expected(name, "natural"), "natural", seed=1, what="natural, seed 1")
        y = _check(ctx, A, _expected(name, "natural"), "natural", seed=99, what="natural, seed 99")
        assert np.array_equal(x[0], y[0]) and x[1] == y[1]
        first = _check(ctx, A, _expected(name, "random"), "random", what="first")
        second = _check(ctx, A, _expected(name, "random"), "random", what="second")
        assert np.array_equal(first[0], second[0]) and first[1] == second[1]
    finally:
        A.free()


def test_optional_outputs_may_be_null_and_the_statistics_are_untouched(ctx):
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    R = ctx.multiply(A, A)
    out = C.c_void_p()
    try:
        before = ctx.stats()
        assert bspgemm.lib().bspgemm_maximal_matching(ctx._h, A._h, 2, SEED, C.byref(out), None, None) == 0
        labels = np.zeros(n, np.int32)
        assert bspgemm.lib().bspgemm_matrix_download(ctx._h, out, None, labels.ctypes.data) == 0
        assert np.array_equal(labels, _expected("rmat10", "random").labels)
        assert ctx.stats() == before and before["rows"] == n
    finally:
        bspgemm.lib().bspgemm_matrix_free(out)
        R.free()
        A.free()


def test_timing_mode_gives_the_same_bits(capfd):
    """a second context, created under BSPGEMM_MATCH_TIMING (read once, in bspgemm_create): one line per call, the same bits"""
    os.environ["BSPGEMM_MATCH_TIMING"] = "1"
    try:
        timed = bspgemm.Context(0)
    finally:
        del os.environ["BSPGEMM_MATCH_TIMING"]
    name = "star_2chunks_plus_1"
    rp, ci, n = _graph(name)
    A = timed.upload(rp, ci, n)
    try:
        capfd.readouterr()
        _check(timed, A, _expected(name, "light"), "light", what="timed")
        lines = [ln for ln in capfd.readouterr().err.splitlines() if NAME + ":" in ln]
        assert len(lines) == 1 and "pairs 1 " in lines[0] and "hub chunks 3 " in lines[0] and "2 point launches" in lines[0], lines
    finally:
        A.free()
        timed.close()


# ---------------------------------------------------------------- 6. through the library's own calls -------------------
def test_the_contracted_graph_through_transpose_and_products(ctx):
    name, order = "rmat12", "light"
    rp, ci, n = _graph(name)
    exp = _expected(name, order)
    srp, sci = match_ref.simple(rp, ci, n)
    A = ctx.upload(rp, ci, n)
    P, _, info = ctx.maximal_matching(A, order, SEED)
    S = ctx.symmetrize(A, drop_diagonal=True)
    T = ctx.transpose(P)
    R1 = ctx.multiply(T, S)
    M1 = ctx.matrix_from_result(R1, n)
    R2 = ctx.multiply(M1, P)
    try:
        # transpose(P): the members of every contracted vertex, at most two, ascending
        t_rp, t_ci = T.download()
        sizes = np.diff(t_rp)
        assert sizes.max() == 2 and int((sizes == 2).sum()) == info["pairs"] == exp.pairs
        assert np.array_equal(sizes, np.bincount(exp.labels, minlength=n))
        assert np.array_equal(t_ci, np.argsort(exp.labels, kind="stable"))
        # P^T * S * P: the quotient, whose diagonal marks the contracted edges
        q_rp, q_ci = R2.download()
        s_rows = np.repeat(np.arange(n), np.diff(srp))
        pairs = np.unique(exp.labels[s_rows].astype(np.int64) * n + exp.labels[sci])
        e_rows, e_cols = pairs // n, pairs % n
        assert np.array_equal(q_rp, np.concatenate([[0], np.cumsum(np.bincount(e_rows, minlength=n))]))
        assert np.array_equal(q_ci, e_cols)
        q_rows = np.repeat(np.arange(n), np.diff(q_rp))
        assert np.array_equal(q_rows[q_rows == q_ci], np.flatnonzero(sizes == 2))
    finally:
        for h in (R2, M1, R1, T, S, P, A):
            h.free()


# ---------------------------------------------------------------- 7. errors --------------------------------------------
def test_errors_leave_no_result_and_a_usable_context(ctx):
    import torch
    L = bspgemm.lib()
    rp, ci, n = _graph("rmat10")
    A = ctx.upload(rp, ci, n)
    rect = ctx.upload(rp[:11], ci[:rp[10]], n)                          # 10 x n
    other = bspgemm.Context(0)
    foreign = other.upload(rp, ci, n)
    trp = torch.from_numpy(rp).cuda()
    wrapped = []
    for at, col in ((ci.size // 2, n), (ci.size - 1, -1), (0, 2**31 - 1)):   # checked on the device before it indexes
        c = ci.copy()
        c[at] = col
        tci = torch.from_numpy(c).cuda()
        wrapped.append(ctx.wrap_device(n, n, c.size, trp.data_ptr(), tci.data_ptr(), keep=(trp, tci)))
    torch.cuda.synchronize()

    def call(a, order=2):
        out, info = C.c_void_p(0x5A5A), bspgemm.MatchInfo()
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = L.bspgemm_maximal_matching(ctx._h, a._h, order, SEED, C.byref(out), None, C.byref(info))
        return st, out.value, L.bspgemm_last_error().decode(), bytes(info) == bytes(C.sizeof(info))

    try:
        st, out, msg, zeroed = call(rect)
        assert st == ERR_INVALID and not out and NAME in msg and "square" in msg and zeroed, msg
        st, out, msg, zeroed = call(foreign)
        assert st == ERR_INVALID and not out and NAME in msg and "context" in msg and zeroed, msg
        for order in (0, 4, -3):
            st, out, msg, zeroed = call(A, order)
            assert st == ERR_INVALID and not out and NAME in msg and "order" in msg and zeroed, msg
        for W in wrapped:
            st, out, msg, zeroed = call(W)
            assert st == ERR_INVALID and not out and "column" in msg and zeroed, msg
            _check(ctx, A, _expected("rmat10", "light"), "light", what="after an out-of-range column")
        with pytest.raises(ValueError):
            ctx.maximal_matching(A, "heavy")
        # the context still multiplies correctly
        R = ctx.multiply(A, A)
        g_rp, g_ci = R.download()
        R.free()
        e_rp, e_ci = gen.small_reference(rp, ci, rp, ci)
        assert np.array_equal(g_rp, e_rp) and np.array_equal(g_ci, e_ci)
        _check(ctx, A, _expected("rmat10", "random"), "random", what="after the errors")
    finally:
        for h in wrapped:
            h.free()
        foreign.free()
        other.close()
        rect.free()
        A.free()
