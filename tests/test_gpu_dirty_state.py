"""Every compute entry point on poisoned workspaces and guarded allocations (the test hooks of include/bspgemm.h:
bspgemm_debug_fill_alloc, bspgemm_debug_guard_alloc / bspgemm_debug_check_guards, bspgemm_debug_scribble).

The entry points share the context's scratch arrays and each relies on having initialised exactly the words it later reads.
A fresh context hides a forgotten reset (fresh device memory tends to read as zeros) and a warm repeat finds its own
well-formed leftovers, so here every allocation is handed out filled with a poison word, every scratch array the context
keeps is overwritten with it between calls, and every allocation carries a canary zone in front and behind.  The words are
0xFFFFFFFF (-1, an infinite distance, every flag set) and 0x00000001 (the smallest flag, a count of one, a valid index):
a misread word then shows as a wrong result rather than as a wild address.  The cases, their operands and their references
are the table of tests/state_cases.py.  Every case prints a line `DIRTYSTATE name word cold warm after-dirtier` (seconds).
"""
import contextlib
import ctypes as C
import functools
import time

import numpy as np
import pytest

import bspgemm
import gen
import state_cases
from state_cases import WORDS

pytestmark = pytest.mark.gpu
WORD_IDS = {0xFFFFFFFF: "ffffffff", 0x00000001: "00000001"}


@contextlib.contextmanager
def hooks(word=None, guard=True):
    """the fill (word not None) and guard hooks on; off again on the way out, whatever happened"""
    if word is not None:
        bspgemm.debug_fill_alloc(True, word)
    bspgemm.debug_guard_alloc(guard)
    try:
        yield
    finally:
        bspgemm.debug_fill_alloc(False)
        bspgemm.debug_guard_alloc(False)


def _live():
    return bspgemm.debug_alloc_state()[1:3]


def _guards_intact(what):
    damaged, text = bspgemm.debug_check_guards()
    assert damaged == 0, "%s: %d damaged allocation(s): %s" % (what, damaged, text)


@functools.lru_cache(maxsize=None)
def _dirtier_operands():
    """the larger pair of the dirtier: R-MAT scale 13, stored untidily"""
    rp, ci, n = gen.rmat(13, 8, (0.45, 0.22, 0.22, 0.11), state_cases.SEED + 1)
    r = np.repeat(np.arange(n), np.diff(rp))
    return state_cases.graph_ops("dirtier", *state_cases.untidy_store(r, ci, n), n)


def _dirty(ctx, d):
    """a plain and a counting product plus transposes on the larger pair: every workspace of the products and of the
    transposes has grown and holds their contents, and the cache of freed results holds theirs"""
    T = ctx.transpose(d.A)
    R = ctx.multiply(d.A, T)
    V = ctx.multiply_masked_count(d.A, d.A, d.A)
    U = ctx.transpose(T)
    for x in (R, V, U, T):
        x.free()


def _run_and_check(ctx, name, g, what, cold=None):
    t0 = time.perf_counter()
    out = state_cases.run_case(ctx, name, g)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    state_cases.check_case(name, g, *out)
    if cold is not None:
        assert state_cases.same(cold, out), "%s: the result differs from the cold run's" % what
    _guards_intact(what)
    return out, dt


@pytest.mark.parametrize("word", WORDS, ids=[WORD_IDS[w] for w in WORDS])
@pytest.mark.parametrize("name,on", state_cases.IDS, ids=["%s@%s" % i for i in state_cases.IDS])
def test_entry_point_on_poisoned_memory(name, on, word):
    before = _live()
    what = "%s@%s %s" % (name, on, WORD_IDS[word])
    with hooks(word):
        ctx = bspgemm.Context(0)
        try:
            g = state_cases.fresh(on).upload(ctx)
            d = state_cases.Ops("dirtier", _dirtier_operands().host).upload(ctx)
            cold, t_cold = _run_and_check(ctx, name, g, what + " cold")
            ctx.debug_scribble(word)
            _, t_warm = _run_and_check(ctx, name, g, what + " scribbled", cold)
            _dirty(ctx, d)
            ctx.debug_scribble(word)
            _, t_after = _run_and_check(ctx, name, g, what + " after the dirtier", cold)
        finally:
            ctx.close()
        _guards_intact(what + " closed")
    assert _live() == before, "%s: live allocations and bytes %s, before the test %s" % (what, _live(), before)
    print("DIRTYSTATE %s@%s %s %.3f %.3f %.3f" % (name, on, WORD_IDS[word], t_cold, t_warm, t_after))


@pytest.mark.parametrize("seed", (1, 2))
def test_long_lived_context(seed):
    """one context for every case of the table in a seeded order, its scratch scribbled between the calls"""
    before = _live()
    order = np.random.default_rng(seed).permutation(len(state_cases.IDS))
    with hooks(WORDS[seed % 2]):
        ctx = bspgemm.Context(0)
        try:
            for k, i in enumerate(order):
                name, on = state_cases.IDS[i]
                word = WORDS[(k + seed) % 2]
                what = "long-lived seed %d, call %d: %s@%s after %s" % (seed, k, name, on, WORD_IDS[word])
                g = state_cases.fresh(on).upload(ctx)
                try:
                    ctx.debug_scribble(word)
                    _run_and_check(ctx, name, g, what)
                finally:
                    g.free()
        finally:
            ctx.close()
        _guards_intact("long-lived seed %d closed" % seed)
    assert _live() == before


# ---------------------------------------------------------------- the hooks themselves -------------------------------
def _device_ints(ptr, first, count):
    """int32[count] from the device array at `ptr`, starting at element `first`"""
    import torch
    from bspgemm import dist as bdist
    dev = torch.device("cuda", 0)
    return bdist.device_tensor(int(ptr) + 4 * first, count, torch.int32, dev).cpu().numpy().view(np.uint32)


def _small_product(ctx, g):
    """the general flow's product of the 300-row pair: (Result, nnz, capacity of col_idx in entries).  The upper bound
    is within 4096 of nnz, so col_idx holds `products` entries and four more (csrc/multiply.hip col_cap_for)"""
    ctx.set_option("small_path", 0)
    R = ctx.multiply(g.dev["A"], g.dev["B"])
    st = ctx.stats()
    assert st["small_path"] == 0 and st["nnz_c"] == R.nnz and R.nnz < st["products"] <= R.nnz + 4096
    return R, R.nnz, int(st["products"])


@pytest.mark.parametrize("word", WORDS, ids=[WORD_IDS[w] for w in WORDS])
def test_fill_hands_out_poisoned_allocations(word):
    """the entries of a fresh result's col_idx past its capacity (the four spare ones, which no kernel stores to when nnz is
    below the capacity) hold the fill word, and so does every entry between nnz and the capacity that no kernel wrote"""
    with hooks(word, guard=False):
        ctx = bspgemm.Context(0)
        try:
            g = state_cases.fresh("uniform300").upload(ctx)
            R, nnz, cap = _small_product(ctx, g)
            tail = _device_ints(R.col_idx_device, nnz, cap + 4 - nnz)
            print("fill %s: %d of the %d entries past nnz hold the word" % (WORD_IDS[word], int((tail == word).sum()), tail.size))
            assert (tail[-4:] == word).all(), tail[-4:]
        finally:
            ctx.close()


def test_scribble_reaches_the_cache_of_freed_results():
    """a result buffer that went into the cache comes back holding the word scribble was given -- each of the two in turn"""
    ctx = bspgemm.Context(0)
    try:
        g = state_cases.fresh("uniform300").upload(ctx)
        R, nnz, cap = _small_product(ctx, g)
        first = R.col_idx_device
        R.free()
        for word in WORDS:
            ctx.debug_scribble(word)
            R, nnz2, cap2 = _small_product(ctx, g)
            assert R.col_idx_device == first and (nnz2, cap2) == (nnz, cap), "the product did not take its buffer from the cache"
            spare = _device_ints(R.col_idx_device, cap, 4)
            assert (spare == word).all(), (WORD_IDS[word], spare)
            R.free()
    finally:
        ctx.close()


def test_guards_catch_a_store_one_past_an_allocation():
    """a 4-byte host-initiated copy to the first address past an uploaded operand's col_idx (nnz + 1 ints were requested)
    lands in the back zone: no fault, one damaged allocation, named with its size, zone and offset; the count stays after
    the operand is freed"""
    import torch
    from bspgemm import dist as bdist
    with hooks(None):
        ctx = bspgemm.Context(0)
        try:
            rp, ci, n, _ = state_cases.operands("untidy").host["A"]
            A = ctx.upload(rp, ci, n)
            # bspgemm_matrix (csrc/internal.hpp): {ctx *, int rows, cols, long long nnz, int *d_row_ptr, *d_col_idx, ...};
            # no accessor hands the operand's arrays out, so the pointer is read from the handle and checked by its contents
            assert C.c_int64.from_address(A._h.value + 16).value == ci.size
            d_col_idx = C.c_void_p.from_address(A._h.value + 32).value
            assert np.array_equal(_device_ints(d_col_idx, 0, ci.size).view(np.int32), ci)
            assert bspgemm.debug_check_guards() == (0, "")
            past = bdist.device_tensor(d_col_idx + 4 * (ci.size + 1), 1, torch.int32, torch.device("cuda", 0))
            past.copy_(torch.tensor([0x12345678], dtype=torch.int32))
            torch.cuda.synchronize()
            damaged, text = bspgemm.debug_check_guards()
            assert damaged == 1 and text == "guard damaged: allocation of %d bytes, back zone, offset 0" % (4 * (ci.size + 1)), text
            assert bspgemm.debug_check_guards()[0] == 1                  # (a live one is not counted twice)
            A.free()
            assert bspgemm.debug_check_guards()[0] == 1                  # freed: remembered
        finally:
            ctx.close()
        assert bspgemm.debug_check_guards()[0] == 1
    with hooks(None):                                                    # a new guarded stretch starts clean
        assert bspgemm.debug_check_guards() == (0, "")
