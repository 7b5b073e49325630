"""The submatrix extraction (bspgemm_matrix_extract, bspgemm_matrix_extract_rows_of) at the ABI level, without a GPU: the
header declares the flag, the struct, the two functions and option 14 as agreed, between bspgemm_matrix_symmetrize and
bspgemm_result_values_sum, and carries the definition; the library exports them, the Python view has them, a C99 caller
compiles cleanly, and every argument error that needs no operand is refused by name before anything is dereferenced.
"""
import ctypes as C

import bspgemm
from abi_kit import ERR_INVALID, FAKE, header_code, header_text, compile_c99, last_error

NAME, NAME_ROWS = "bspgemm_matrix_extract", "bspgemm_matrix_extract_rows_of"

FLAG = "#define BSPGEMM_EXTRACT_KEEP_SHAPE 1u"
STRUCT = ("typedef struct bspgemm_extract_info { int64_t kept; int64_t scanned; int64_t hub_chunks; int lanes; int cols_monotone; "
          "int sorted_by; int canonicalised; } bspgemm_extract_info;")
DECLARATION = ("bspgemm_status bspgemm_matrix_extract(bspgemm_context *ctx, const bspgemm_matrix *A, int ni, const int *I, int nj, "
               "const int *J, unsigned flags, bspgemm_matrix **out, bspgemm_extract_info *info);")
DECLARATION_ROWS = ("bspgemm_status bspgemm_matrix_extract_rows_of(bspgemm_context *ctx, const bspgemm_matrix *A, "
                    "const bspgemm_matrix *MI, int ri, const bspgemm_matrix *MJ, int rj, unsigned flags, bspgemm_matrix **out, "
                    "bspgemm_extract_info *info);")


def test_header_declares_them_between_symmetrize_and_values_sum():
    code = header_code()
    for piece in (FLAG, STRUCT, DECLARATION, DECLARATION_ROWS):
        assert piece in code, "include/bspgemm.h does not hold as agreed: " + piece
    assert code.index("bspgemm_matrix_symmetrize(") < code.index(FLAG) < code.index(STRUCT) < code.index(NAME + "(") \
        < code.index(NAME_ROWS + "(") < code.index("bspgemm_result_values_sum(")
    assert "BSPGEMM_OPT_EXTRACT_LANES = 14" in code
    text = header_text()
    comment = text.split("#define BSPGEMM_EXTRACT_KEEP_SHAPE")[0].rsplit("/*", 1)[1]
    # the definition is the contract
    for word in ('NULL means "all, in order"', "out is ni x nj", "(I[r], J[c]) in pattern(A)", "copied that many times",
                 "J must not name a column", "induced subgraph", "D_I * A * D_J", "strictly ascending and duplicate-free",
                 "canonicalised = 1", "layout of an uploaded one", "ni == 0, nj == 0, A.rows == 0", "canonical copy of A",
                 "stored col_idx of row ri of MI", "ri == -1", "never leave the device", "bit for bit", "kept = nnz(out)",
                 "scanned", "hub_chunks", "cols_monotone", "sorted_by", "BSPGEMM_OPT_EXTRACT_LANES", "BSPGEMM_EXTRACT_TIMING",
                 "Synchronisations: TWO", "one length read-back", "No kernel waits for another workgroup",
                 "before anything is launched", "BSPGEMM_ERR_OVERFLOW", "BSPGEMM_ERR_ALLOC", "Nothing is leaked"):
        assert word in comment, word
    assert "EXTRACT_LANES" in text.split("typedef enum bspgemm_option")[0]
    assert "BSPGEMM_EXTRACT_TIMING" in text.split("typedef struct bspgemm_context")[0]


def test_library_exports_and_python_view():
    L = bspgemm.lib()
    for name, nargs in ((NAME, 9), (NAME_ROWS, 9)):
        assert hasattr(L, name), "%s is not exported by libbspgemm.so" % name
        assert name in bspgemm.EXPORTS
        assert len(getattr(L, name).argtypes) == nargs
    assert callable(getattr(bspgemm.Context, "extract", None)), "Context.extract"
    assert callable(getattr(bspgemm.Context, "extract_rows_of", None)), "Context.extract_rows_of"
    assert bspgemm.OPTIONS["extract_lanes"] == 14 and bspgemm.EXTRACT_KEEP_SHAPE == 1
    assert C.sizeof(bspgemm.ExtractInfo) == 3 * 8 + 4 * 4
    assert [f for f, _ in bspgemm.ExtractInfo._fields_] == ["kept", "scanned", "hub_chunks", "lanes", "cols_monotone", "sorted_by",
                                                            "canonicalised"]
    assert [getattr(bspgemm.ExtractInfo, f).offset for f, _ in bspgemm.ExtractInfo._fields_] == [0, 8, 16, 24, 28, 32, 36]


C99_CALLER = r"""
#include <stddef.h>
#include "bspgemm.h"
/* the subgraph induced by the first k vertices, then the members of row c of PT cut out in place; entries kept, or -1 */
long long induced(bspgemm_context *ctx, const bspgemm_matrix *A, const bspgemm_matrix *PT, int c, int k, int *first)
{
    bspgemm_extract_info info;
    bspgemm_matrix *S = NULL, *T = NULL;
    long long kept;
    int v;
    for (v = 0; v < k; v++) first[v] = v;
    if (bspgemm_set_option(ctx, BSPGEMM_OPT_EXTRACT_LANES, 16) != BSPGEMM_OK) return -1;
    if (bspgemm_matrix_extract(ctx, A, k, first, k, first, 0u, &S, &info) != BSPGEMM_OK) return -1;
    kept = (long long)info.kept;
    if (bspgemm_matrix_extract(ctx, A, 0, NULL, 0, NULL, BSPGEMM_EXTRACT_KEEP_SHAPE, &T, NULL) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(T);
    if (bspgemm_matrix_extract_rows_of(ctx, A, PT, c, PT, c, BSPGEMM_EXTRACT_KEEP_SHAPE, &T, &info) != BSPGEMM_OK) return -1;
    bspgemm_matrix_free(T);
    bspgemm_matrix_free(S);
    return kept + 0 * (long long)(info.scanned + info.hub_chunks)
           + 0 * (info.lanes + info.cols_monotone + info.sorted_by + info.canonicalised);
}
"""


def test_c99_caller_compiles(tmp_path):
    r = compile_c99(tmp_path, C99_CALLER)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_by_name():
    L = bspgemm.lib()
    fake = FAKE            # never dereferenced: the bad argument is refused first
    three = (C.c_int * 3)(0, 1, 2)

    last = last_error

    def zeroed(info, out, armed_out):
        assert bytes(info) == bytes(C.sizeof(info)), "info is not zeroed"
        if armed_out:
            assert out.value is None, "*out is not NULL"

    def call(ctx, A, ni, I, nj, J, flags, with_out=True):
        info, out = bspgemm.ExtractInfo(), C.c_void_p(77)
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = L.bspgemm_matrix_extract(ctx, A, ni, I, nj, J, flags, C.byref(out) if with_out else None, C.byref(info))
        zeroed(info, out, with_out)
        return st

    def call_rows(ctx, A, MI, ri, MJ, rj, flags, with_out=True):
        info, out = bspgemm.ExtractInfo(), C.c_void_p(77)
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        st = L.bspgemm_matrix_extract_rows_of(ctx, A, MI, ri, MJ, rj, flags, C.byref(out) if with_out else None, C.byref(info))
        zeroed(info, out, with_out)
        return st

    for ctx, A, with_out in ((None, fake, True), (fake, None, True), (fake, fake, False)):
        assert call(ctx, A, 3, three, 3, three, 0, with_out) == ERR_INVALID and NAME in last() and "NULL" in last(), last()
        assert call_rows(ctx, A, None, -1, None, -1, 0, with_out) == ERR_INVALID and NAME_ROWS in last() and "NULL" in last(), last()
    for flags in (2, 3, 0x80000000):
        assert call(fake, fake, 3, three, 3, three, flags) == ERR_INVALID and NAME in last() and "flag" in last(), last()
        assert call_rows(fake, fake, None, -1, None, -1, flags) == ERR_INVALID and NAME_ROWS in last() and "flag" in last(), last()
    for k in (-1, -1000):
        assert call(fake, fake, k, three, 3, three, 0) == ERR_INVALID and NAME in last() and "ni < 0" in last(), last()
        assert call(fake, fake, 3, three, k, three, 1) == ERR_INVALID and NAME in last() and "nj < 0" in last(), last()
