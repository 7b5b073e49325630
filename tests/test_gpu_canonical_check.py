"""The canonical-form check (k_set_flags of csrc/setop.hip; launch_canonical_check) at every edge of its geometry, seen
where the library shows its verdict: info["canonicalised"] of multiply_masked_dot (bit 1, 2, 4 for A, B, F) and of
bfs_tree (a caller's AT), and the complete results, bit for bit against dot_ref.py, bfs_tree_ref.py and setop_ref.py.

A lane checks four consecutive entries per step; the pair in front of its first entry needs the left neighbour it loaded
separately (before[j]), and the steps (256 entries), waves (1024) and tiles (4096) are further seams.  So the operands
here are canonical but for ONE pair, placed at each position class in turn: a repeat (ci[p] = ci[p - 1]) or a descent
(the two swapped).  The products are arranged so that a defect the check missed also changes a value, and so the verdict
and the result fail independently.  The controls hold the same positions as the first entry of a row whose column does
not exceed the last one of the row before: a check that forgot the row boundary would canonicalise them.  Further: a
tile that spans more than 4096 rows (the window is searched in row_ptr itself), col_idx one int off 16-byte alignment
(the entry-by-entry path of load4), E % 4 == 1 (its tail), the <true> instance behind the set operations, and columns
out of range at the same positions.  tests/test_transpose_shapes.py proves the cases without a GPU.
"""
import functools

import numpy as np
import pytest

import bfs_tree_ref
import bspgemm
import dot_ref
import setop_ref
import transpose_ref as T

pytestmark = pytest.mark.gpu
ERR_INVALID = 1
ROLES = "ABF"
KINDS = ("repeat", "descent")
CASES = [(E, p) for E in T.CHECK_E for p in T.check_positions(E)]
CASE_IDS = ["E%d-p%d" % c for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


def _wrap_off_alignment(ctx, m, rows, cols):
    """the operand as wrapped device arrays whose col_idx is one int off 16-byte alignment"""
    import torch
    trp = torch.from_numpy(np.array(m[0], np.int32)).cuda()
    buf = torch.zeros(m[1].size + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + m[1].size] = torch.from_numpy(np.array(m[1], np.int32)).cuda()
    torch.cuda.synchronize()
    assert buf[1:].data_ptr() % 16 == 4
    return ctx.wrap_device(rows, cols, m[1].size, trp.data_ptr(), buf[1:].data_ptr(), keep=(trp, buf))


def _dot(ctx, x, cols, role, off_alignment=False):
    """the masked dot product of transpose_ref.dot_operands with x in `role`: (failures of the result, canonicalised)"""
    args = T.dot_operands(x, cols, role)
    a, b, f, a_rows, b_rows, ab_cols, f_cols = args
    exp = dot_ref.dot_ref(*args)
    hs = []
    for k, (m, rows, c) in enumerate(((a, a_rows, ab_cols), (b, b_rows, ab_cols), (f, a_rows, f_cols))):
        hs.append(_wrap_off_alignment(ctx, m, rows, c) if off_alignment and k == role else ctx.upload(m[0], m[1], c))
    Cr = None
    try:
        Cr, info = ctx.multiply_masked_dot(*hs)
        rp, ci = Cr.download()
        got = (rp, ci, Cr.download_values())
    finally:
        for h in [Cr] + hs:
            if h is not None:
                h.free()
    bad = []
    for name, g, e in zip(("row_ptr", "col_idx", "values"), got, exp):
        if g.shape != e.shape:
            bad.append("%s has %d entries, expected %d" % (name, g.size, e.size))
        elif not np.array_equal(g, e):
            k = int(np.flatnonzero(g != e)[0])
            bad.append("%s differs first at %d: got %d, expected %d (%d differ)" % (name, k, g[k], e[k], int((g != e).sum())))
    if info["kept"] != exp[1].size:
        bad.append("info.kept %d, expected %d" % (info["kept"], exp[1].size))
    return bad, info["canonicalised"]


def _judge(bad, canon, expected_bits, what):
    """both findings in one message: the verdict of the check and the result fail independently"""
    msgs = list(bad)
    if canon != expected_bits:
        msgs.insert(0, "canonicalised %d, expected %d" % (canon, expected_bits))
    assert not msgs, "%s: %s" % (what, "; ".join(msgs))


# ---------------------------------------------------------------- 1. one defect, every position class ----------------
@pytest.mark.parametrize("E,p", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("role", [0, 1, 2], ids=list(ROLES))
def test_one_defect(ctx, role, kind, E, p):
    x = T.check_base(E)
    d = T.with_defect(x["rp"], x["ci"], p, kind)
    bad, canon = _dot(ctx, (x["rp"], d), x["cols"], role)
    _judge(bad, canon, 1 << role, "%s at %d of %d in %s" % (kind, p, E, ROLES[role]))


# ---------------------------------------------------------------- 2. controls ----------------------------------------
@pytest.mark.parametrize("E", T.CHECK_E)
@pytest.mark.parametrize("role", [0, 1, 2], ids=list(ROLES))
def test_controls(ctx, role, E):
    for name, x in (("base", T.check_base(E)), ("control", T.check_control(E))):
        bad, canon = _dot(ctx, (x["rp"], x["ci"]), x["cols"], role)
        _judge(bad, canon, 0, "%s of %d entries as %s" % (name, E, ROLES[role]))


# ---------------------------------------------------------------- 3. a tile whose window is not staged ---------------
@pytest.mark.parametrize("kind", KINDS + ("control",))
@pytest.mark.parametrize("role", [0, 1, 2], ids=list(ROLES))
def test_unstaged_tile(ctx, role, kind):
    x, p = T.check_unstaged(kind == "control")
    ci = x["ci"] if kind == "control" else T.with_defect(x["rp"], x["ci"], p, kind)
    bad, canon = _dot(ctx, (x["rp"], ci), x["cols"], role)
    _judge(bad, canon, 0 if kind == "control" else 1 << role, "%s at %d behind 4200 empty rows in %s" % (kind, p, ROLES[role]))


# ---------------------------------------------------------------- 4. the entry-by-entry loads ------------------------
@pytest.mark.parametrize("E", T.CHECK_E)
@pytest.mark.parametrize("kind", KINDS + ("control",))
@pytest.mark.parametrize("role", [0, 1, 2], ids=list(ROLES))
def test_off_alignment(ctx, role, kind, E):
    if kind == "control":
        x = T.check_control(E)
        bad, canon = _dot(ctx, (x["rp"], x["ci"]), x["cols"], role, off_alignment=True)
        _judge(bad, canon, 0, "control of %d entries, wrapped off alignment as %s" % (E, ROLES[role]))
        return
    x = T.check_base(E)
    for p in (4, 256, 4096, E - 1):
        d = T.with_defect(x["rp"], x["ci"], p, kind)
        bad, canon = _dot(ctx, (x["rp"], d), x["cols"], role, off_alignment=True)
        _judge(bad, canon, 1 << role, "%s at %d of %d in %s, wrapped off alignment" % (kind, p, E, ROLES[role]))


# ---------------------------------------------------------------- 5. the other entry points --------------------------
@functools.lru_cache(maxsize=None)
def _bfs_case(p, kind):
    """(A, AT with the defect, the expected tree): A = the transpose of the defective AT's pattern, so AT is A's
    transpose but for its form"""
    x = T.check_base(T.CHECK_E[0])
    n = x["rows"]
    at = (x["rp"], T.with_defect(x["rp"], x["ci"], p, kind))
    a = T.ref_transpose(at[0], at[1], n)
    return a, at, n, bfs_tree_ref.bfs_tree(a[0], a[1], n, 0)


@pytest.mark.parametrize("p", [4, 1024, 4096])
@pytest.mark.parametrize("kind", KINDS)
def test_bfs_tree_pull_with_a_defective_transpose(ctx, kind, p):
    a, at, n, (e_rp, e_parent, e_level) = _bfs_case(p, kind)
    assert e_parent.size > n // 2 and e_level.max() >= 2
    A, AT = ctx.upload(a[0], a[1], n), ctx.upload(at[0], at[1], n)
    R = None
    try:
        R, info = ctx.bfs_tree(A, AT, 0, "pull")
        rp, parent = R.download()
        level = R.download_values()
    finally:
        for h in (R, AT, A):
            if h is not None:
                h.free()
    what = "%s at %d of AT" % (kind, p)
    assert info["canonicalised"] == 1 and info["transposed"] == 0 and info["pull_levels"] > 0, (what, info)
    assert np.array_equal(rp, e_rp) and np.array_equal(parent, e_parent) and np.array_equal(level, e_level), what


def _same(got, exp):
    return all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(got, exp))


@pytest.mark.parametrize("p", [4, 1024, 4096])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("side", ["A", "B"])
def test_setop_with_a_defect(ctx, side, kind, p):
    """the <true> instance (the first operand's pass) and the <false> one (the second's) behind bspgemm_matrix_setop and
    bspgemm_matrix_equal, judged by the result"""
    E = T.CHECK_E[0]
    x, y = T.check_base(E), T.check_partner(E)
    n = x["rows"]
    d = (x["rp"], T.with_defect(x["rp"], x["ci"], p, kind))
    canon = setop_ref.canonical_ref(d[0], d[1], n, n)
    assert (canon[1].size == E) == (kind == "descent")                   # a repeat loses a column, a descent nothing
    D, Y, X, K = (ctx.upload(m[0], m[1], n) for m in (d, (y["rp"], y["ci"]), (x["rp"], x["ci"]), canon))
    bad = []
    try:
        for op in ("or", "and", "xor", "andnot"):
            (l, L), (r, R) = ((d, D), ((y["rp"], y["ci"]), Y))
            if side == "B":
                (l, L), (r, R) = (r, R), (l, L)
            S = ctx.setop(L, R, op)
            got, nnz = S.download(), S.nnz
            S.free()
            exp = setop_ref.setop_ref(l[0], l[1], r[0], r[1], n, n, op)
            if not _same(got, exp) or nnz != exp[1].size:
                bad.append(op)
        first, second = (D, K) if side == "A" else (K, D)
        if not ctx.matrix_equal(first, second):
            bad.append("equal(defective, its canonical form)")
        first, second = (D, X) if side == "A" else (X, D)
        if ctx.matrix_equal(first, second) != (kind == "descent"):
            bad.append("equal(defective, base)")
        first, second = (D, Y) if side == "A" else (Y, D)
        if ctx.matrix_equal(first, second):
            bad.append("equal(defective, partner)")
    finally:
        for h in (D, Y, X, K):
            h.free()
    assert not bad, "%s at %d in %s: %s" % (kind, p, side, bad)


# ---------------------------------------------------------------- 6. columns out of range ----------------------------
@pytest.mark.parametrize("value", ["cols", "negative"])
@pytest.mark.parametrize("role", [0, 1, 2], ids=list(ROLES))
def test_column_out_of_range(ctx, role, value):
    E = T.CHECK_E[0]
    x = T.check_base(E)
    for p in (0, 4, 4096, E - 1):
        ci = x["ci"].copy()
        ci[p] = x["cols"] if value == "cols" else -1
        a, b, f, a_rows, b_rows, ab_cols, f_cols = T.dot_operands((x["rp"], ci), x["cols"], role)
        hs = [ctx.upload(a[0], a[1], ab_cols), ctx.upload(b[0], b[1], ab_cols), ctx.upload(f[0], f[1], f_cols)]
        try:
            with pytest.raises(bspgemm.BspgemmError) as e:
                ctx.multiply_masked_dot(*hs)
        finally:
            for h in hs:
                h.free()
        assert e.value.status == ERR_INVALID, (p, str(e.value))
        assert "bspgemm_multiply_masked_dot" in str(e.value) and "operand %s" % ROLES[role] in str(e.value), (p, str(e.value))
        bad, canon = _dot(ctx, (x["rp"], x["ci"]), x["cols"], role)     # the context still computes a correct product
        _judge(bad, canon, 0, "after column %s at %d of %s" % (value, p, ROLES[role]))
