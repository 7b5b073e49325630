"""The int32 drop-ins' destination policies (csrc/dropin.hip, csrc/early_dest.hpp) on the GPU: the early destination across a
128 MiB piece boundary, with its second piece abandoned, with its overshoot given back; a caller's buffer grown or kept;
an empty product; a refusal.  Expected results come from the handle API (Context.multiply(...).download(), itself checked
against the oracle in test_gpu_parity.py) and from counts computed on the CPU with scipy when the cases were chosen."""
import ctypes as C
import os

import numpy as np
import pytest

import bspgemm
import gen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIECE = 1 << 27                     # EarlyDest's default piece: 128 MiB
VP = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    c = bspgemm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def raw():
    """the drop-ins with plain pointer arguments (NULL allowed), and libc's malloc / free"""
    bspgemm.lib()                                       # (loads torch's HIP runtime first)
    L = C.CDLL(bspgemm.LIB_PATH)                        # the same library, prototypes of its own
    L.SpGEMM_hip.argtypes = [VP, VP, C.c_int, VP, VP, C.c_int, C.POINTER(VP), VP, C.c_int]
    L.SpGEMM_hip_bigslice.argtypes = [VP, VP, C.c_int, VP, VP, C.c_int, C.POINTER(VP), VP, C.POINTER(C.c_int), C.c_int, C.c_int]
    L.SpGEMM_hip_masked.argtypes = [VP, VP, C.c_int, VP, VP, C.c_int, VP, VP, C.POINTER(VP), VP, C.POINTER(C.c_int)]
    libc = C.CDLL(None)
    libc.malloc.restype, libc.malloc.argtypes = VP, [C.c_size_t]
    libc.free.restype, libc.free.argtypes = None, [VP]
    return L, libc


def ptr(a):
    return VP(a.ctypes.data)


def handle_product(ctx, rp, ci, n):
    A = ctx.upload(rp, ci, n)
    Cr = ctx.multiply(A, A)
    crp, cci = Cr.download()
    products = ctx.stats()["products"]
    Cr.free()
    A.free()
    return crp, cci, products


def bound_of(rp, ci, n):
    """bspgemm_par_output_bound: sum over the rows of min(F_i, columns)"""
    return int(np.minimum(gen.row_products(rp, ci, rp, 0, n), n).sum())


def dropin(raw, rp, ci, n):
    """SpGEMM_hip(A, A) -> (Crow, Ccol copied out of the malloc'ed result, which libc's free has taken)"""
    L, libc = raw
    crow = np.full(n + 1, -1, np.int32)
    cc = VP()
    assert L.SpGEMM_hip(ptr(ci), ptr(rp), n, ptr(ci), ptr(rp), n, C.byref(cc), ptr(crow), 0) == 0
    assert cc.value
    ccol = np.ctypeslib.as_array(C.cast(cc, C.POINTER(C.c_int32)), shape=(max(int(crow[-1]), 1),))[:int(crow[-1])].copy()
    libc.free(cc)
    return crow, ccol


def test_two_pieces_one_boundary_crossed(ctx, raw):
    rp, ci, n = gen.uniform(1 << 20, 6, 9101)
    erp, eci, products = handle_product(ctx, rp, ci, n)
    assert products == 37_748_593 and erp[-1] == 37_748_070
    assert erp[-1] * 4 > PIECE and bound_of(rp, ci, n) * 4 <= 2 * PIECE          # 1.125 pieces: one boundary
    crow, ccol = dropin(raw, rp, ci, n)
    assert np.array_equal(crow, erp) and np.array_equal(ccol, eci)


def test_second_piece_abandoned(ctx, raw):
    rp, ci, n = gen.rmat(14, 16, (0.57, 0.19, 0.19, 0.05), 9105)
    erp, eci, _ = handle_product(ctx, rp, ci, n)
    assert bound_of(rp, ci, n) == 39_633_573 and erp[-1] == 20_268_828
    assert PIECE < 39_633_573 * 4 <= 2 * PIECE and erp[-1] * 4 <= PIECE          # two pieces, the product in piece 0
    for _ in range(2):                                  # (the second call: the abandoned helper left nothing behind)
        crow, ccol = dropin(raw, rp, ci, n)
        assert np.array_equal(crow, erp) and np.array_equal(ccol, eci)


def test_shrink_path_one_pinned_piece(ctx, raw):
    rp, ci, n = gen.rmat(13, 16, (0.57, 0.19, 0.19, 0.05), 9104)
    erp, eci, _ = handle_product(ctx, rp, ci, n)
    bound = bound_of(rp, ci, n)
    assert bound == 13_475_217 and erp[-1] == 7_097_659
    assert (1 << 20) <= bound * 4 <= PIECE and bound - erp[-1] > (1 << 20)       # pinned, one piece, overshoot given back
    crow, ccol = dropin(raw, rp, ci, n)                 # (frees the shrunk block with libc's free)
    assert np.array_equal(crow, erp) and np.array_equal(ccol, eci)


def grow_case(raw, call, nrows, erp, eci, size):
    """one call of a grow-policy drop-in with a libc-malloc'ed buffer of `size` entries (None: *Ccol NULL, *Csize 0)"""
    L, libc = raw
    nnz = int(erp[-1])
    buf = VP(libc.malloc(size * 4)) if size is not None else VP()
    before = buf.value
    csize = C.c_int(size or 0)
    crow = np.full(nrows + 1, -1, np.int32)
    assert call(C.byref(buf), ptr(crow), C.byref(csize)) == 0
    assert buf.value
    if size == nnz:
        assert buf.value == before and csize.value == nnz            # large enough: the caller's buffer as it was
    else:
        assert csize.value == nnz
    ccol = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_int32)), shape=(nnz,)).copy()
    libc.free(buf)
    assert np.array_equal(crow, erp) and np.array_equal(ccol, eci)


@pytest.mark.parametrize("size", ["nnz", "nnz-1", "1", "null"])
def test_grow_policy_bigslice(raw, size):
    g = np.load(os.path.join(GOLDEN, "uniform_n4096_rows1024_3072_omp.npz"), allow_pickle=False)
    n, r0, rows = int(g["n"]), int(g["row0"]), int(g["rows"])
    a_rp, a_ci = bspgemm._i32(g["a_rp"]), bspgemm._i32(g["a_ci"])
    nnz = int(g["c_rp"][-1])
    L = raw[0]
    grow_case(raw, lambda cc, crow, cs: L.SpGEMM_hip_bigslice(ptr(a_ci), ptr(a_rp), n, ptr(a_ci), ptr(a_rp), n, cc, crow, cs, r0, r0 + rows),
              rows, g["c_rp"], g["c_ci"], {"nnz": nnz, "nnz-1": nnz - 1, "1": 1, "null": None}[size])


@pytest.mark.parametrize("size", ["nnz", "nnz-1", "1", "null"])
def test_grow_policy_masked(raw, size):
    g = np.load(os.path.join(GOLDEN, "masked_n512.npz"), allow_pickle=False)
    n = int(g["n"])
    a_rp, a_ci, f_rp, f_ci = (bspgemm._i32(g[k]) for k in ("a_rp", "a_ci", "f_rp", "f_ci"))
    nnz = int(g["c_rp"][-1])
    L = raw[0]
    grow_case(raw, lambda cc, crow, cs: L.SpGEMM_hip_masked(ptr(a_ci), ptr(a_rp), n, ptr(a_ci), ptr(a_rp), n, ptr(f_ci), ptr(f_rp), cc, crow, cs),
              n, g["c_rp"], g["c_ci"], {"nnz": nnz, "nnz-1": nnz - 1, "1": 1, "null": None}[size])


def test_empty_product(raw):
    rp, ci = np.zeros(6, np.int32), np.zeros(1, np.int32)           # 5 rows, no entries
    crow, ccol = dropin(raw, rp, ci, 5)                              # (*Ccol non-NULL, freed)
    assert np.array_equal(crow, np.zeros(6, np.int32)) and ccol.size == 0


def test_refusal_then_a_valid_call(raw):
    L = raw[0]
    g = np.load(os.path.join(GOLDEN, "uniform_n4096_rows1024_3072_omp.npz"), allow_pickle=False)
    n = int(g["n"])
    rp, ci = bspgemm._i32(g["a_rp"]), bspgemm._i32(g["a_ci"])
    cc = VP(1)
    assert L.SpGEMM_hip(ptr(ci), ptr(rp), n, ptr(ci), ptr(rp), n, C.byref(cc), None, 0) == 1       # BSPGEMM_ERR_INVALID
    assert not cc.value
    r0, rows = int(g["row0"]), int(g["rows"])
    crow, ccol = bspgemm.SpGEMM_hip(ci, rp, rows, ci, rp, n, row0=r0)
    assert np.array_equal(crow, g["c_rp"]) and np.array_equal(ccol, g["c_ci"])
