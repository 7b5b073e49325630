"""The flat prepass (csrc/prepass.hip: k_tile_rows + k_row_work_flat, the path of B's blocked extents table): tiles of
kRowWorkTile = 4096 merged positions (each row's nonzeros, then one end item), rows that cross a tile boundary summed by
atomic adds.  Full products against the CPU oracle, under both flows, and the products count (sum of F_i, which the
upper-bound flow would hide when too large) against the oracle's, on A rows placed on the tile edges: rows ending exactly
on a multiple of the tile and one nonzero either side, a row longer than several tiles, runs of empty rows (thousands at
once, and a million at once in the middle and at the end), nnz(A) not a multiple of the tile, interior row ranges.  B has 2^21 rows
(the size where the blocked table is chosen by itself) with rows of 255+ nonzeros, whose clamped lengths fall through to
B.row_ptr; the blocked table and the padded rows are also forced on and off."""
import numpy as np
import pytest

import bspgemm
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TILE = 4096                                    # csrc/kernels.hpp kRowWorkTile
B_ROWS = 1 << 21                               # csrc/context.hip ensure_blk8: the blocked table from 2^21 rows of B


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def csr(lengths, cols_of):
    rp = np.zeros(len(lengths) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lengths)
    ci = np.concatenate([cols_of(i, n) for i, n in enumerate(lengths)] or [np.zeros(0, dtype=np.int64)])
    return rp.astype(np.int32), ci.astype(np.int32)


def edge_a(rng):
    """A row lengths put on the tile edges: a running position is steered onto multiples of TILE, -1 and +1 of them"""
    lengths = []
    pos = 0

    def add(n):
        nonlocal pos
        lengths.append(n)
        pos += n

    add(0)
    add(0)
    add(TILE)                                  # one row exactly one tile
    add(TILE - 1)                              # ends one before the boundary
    add(2)                                     # crosses it by one
    add(TILE - 1 - (pos % TILE))               # ends exactly on a boundary
    for _ in range(3000):                      # short rows: ~16 nonzeros, like the bench matrix
        add(int(rng.integers(0, 33)))
    for _ in range(5000):                      # a run of empty rows
        add(0)
    add(3 * TILE + 5)                          # longer than several tiles
    add((TILE - pos % TILE) + 1)               # ends one past a boundary
    for _ in range(20000):                     # rows of one nonzero and empty rows: a tile's rows mostly empty
        add(int(rng.integers(0, 2)))
    add(36000)                                 # a power-law hub
    for _ in range(400):
        add(int(rng.integers(1, 64)))
    add(TILE - (pos % TILE) + 7)               # nnz(A) not a multiple of the tile
    for _ in range(3000):
        add(0)
    return lengths


def make_b(rng):
    """2^21 rows, mostly 0-3 nonzeros, every 4099th row 255-400 nonzeros (clamped in the blocked table)"""
    lengths = rng.integers(0, 4, size=B_ROWS)
    heavy = np.arange(5, B_ROWS, 4099)
    lengths[heavy] = rng.integers(255, 401, size=heavy.size)
    cols = 50000
    rp = np.zeros(B_ROWS + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lengths)
    ci = np.empty(int(rp[-1]), dtype=np.int32)
    for r in np.flatnonzero(lengths >= 255):     # distinct sorted columns in the long rows
        ci[rp[r]:rp[r + 1]] = np.sort(rng.choice(cols, size=int(lengths[r]), replace=False))
    short = np.repeat(lengths < 255, lengths)
    ci[short] = rng.integers(0, cols, size=int(short.sum()))
    return rp.astype(np.int32), ci, cols


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(2024)
    b_rp, b_ci, b_cols = make_b(rng)
    heavy = np.flatnonzero(np.diff(b_rp) >= 255)

    def cols_of(i, n):
        c = rng.integers(0, B_ROWS, size=n)
        if n > 4:                                # some of every longer row on B's long rows (fall-through lookups)
            c[: n // 5] = rng.choice(heavy, size=n // 5)
        return c

    a_rp, a_ci = csr(edge_a(rng), cols_of)
    assert a_rp[-1] % TILE != 0
    return a_rp, a_ci, b_rp, b_ci, b_cols


def product(ctx, operands, flow, r0, r1, blocked, padded):
    """C rows [r0, r1) with the knobs forced for this product only; (row_ptr, col_idx, stats, B's blocked-table use)"""
    a_rp, a_ci, b_rp, b_ci, b_cols = operands
    saved = {k: ctx.get_option(k) for k in ("small_path", "blocked_extents", "padded_rows")}
    try:
        ctx.set_flow(flow)
        ctx.set_option("small_path", 0)        # the general flow, whose prepass this file is about, at every size
        ctx.set_option("blocked_extents", blocked)
        ctx.set_option("padded_rows", padded)
        A = ctx.upload(a_rp, a_ci, B_ROWS)
        B = ctx.upload(b_rp, b_ci, b_cols)
        try:
            C = ctx.multiply(A, B, r0, r1)
            crp, cci = C.download()
            st = ctx.stats()
            C.free()
            uses = B.uses_blocked_table
        finally:
            A.free()
            B.free()
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
        ctx.set_flow("auto")
    return crp, cci, st, uses


def check(ctx, ops, flow, r0, r1, blocked, padded):
    a_rp, a_ci, b_rp, b_ci, b_cols = ops
    what = "%s, rows %d..%d, blocked %d, padded %d" % (flow, r0, r1, blocked, padded)
    erp, eci = O.spgemm_rows(a_rp, a_ci, b_rp, b_ci, b_cols, r0, r1)
    crp, cci, st, uses = product(ctx, ops, flow, r0, r1, blocked, padded)
    assert uses == (0 if blocked == 0 else 1), what
    assert st["prepass_kernel"] == (0 if blocked == 0 else 1), what
    assert st["padded_rows"] == padded, what
    assert st["products"] == O.count_products(a_rp, a_ci, b_rp, r0, r1), "sum of F_i differs (%s)" % what
    assert np.array_equal(np.asarray(crp, dtype=np.int64), np.asarray(erp, dtype=np.int64)), "row_ptr differs (%s)" % what
    assert np.array_equal(cci, eci), "col_idx differs (%s)" % what


def ranges(a_rp):
    n = a_rp.size - 1
    # the whole of A; an interior range starting inside the tile-edge rows; one starting inside the long row's neighbours
    return [(0, n), (3, n - 1000), (3008, n)]


@pytest.mark.parametrize("flow", ["upper-bound", "exact"])
@pytest.mark.parametrize("blocked,padded", [(-1, 0), (1, 0), (1, 1), (0, 0), (0, 1)])
def test_flat_prepass_parity(ctx, operands, flow, blocked, padded):
    for r0, r1 in ranges(operands[0]):
        check(ctx, operands, flow, r0, r1, blocked, padded)


@pytest.mark.parametrize("flow", ["upper-bound", "exact"])
def test_flat_prepass_tile_multiples(ctx, flow):
    """nnz(A) an exact multiple of the tile, and a range whose nonzeros are exactly one tile; every row crosses a boundary
    or ends on one"""
    rng = np.random.default_rng(7)
    b_rp, b_ci, b_cols = make_b(rng)
    lengths = [TILE // 2 + 1, TILE // 2 - 1, TILE, 1, TILE - 1, 2 * TILE, 0, 0]
    a_rp, a_ci = csr(lengths, lambda i, n: rng.integers(0, B_ROWS, size=n))
    assert a_rp[-1] % TILE == 0
    ops = (a_rp, a_ci, b_rp, b_ci, b_cols)
    for r0, r1 in [(0, len(lengths)), (0, 2), (2, 3), (1, 6), (6, 8)]:
        check(ctx, ops, flow, r0, r1, -1, 0)


@pytest.mark.parametrize("flow", ["upper-bound", "exact"])
def test_flat_prepass_empty_runs(ctx, flow):
    """a million empty rows between short rows, and 400000 at the end: empty rows take tile positions like nonzeros, so no
    tile walks a long run of them; interior ranges start and end inside the runs"""
    rng = np.random.default_rng(11)
    b_rp, b_ci, b_cols = make_b(rng)
    lengths = np.zeros(1000 + 1000000 + 3000 + 400000, dtype=np.int64)
    lengths[:1000] = rng.integers(0, 33, size=1000)
    lengths[1001000:1004000] = rng.integers(0, 33, size=3000)
    lengths[1002000] = 3 * TILE + 1
    a_rp = np.zeros(lengths.size + 1, dtype=np.int64)
    a_rp[1:] = np.cumsum(lengths)
    a_ci = rng.integers(0, B_ROWS, size=int(a_rp[-1]))
    ops = (a_rp.astype(np.int32), a_ci.astype(np.int32), b_rp, b_ci, b_cols)
    n = lengths.size
    for r0, r1 in [(0, n), (500, n - 1000), (600000, 1002500), (1001500, n)]:
        check(ctx, ops, flow, r0, r1, -1, 0)
