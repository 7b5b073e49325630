/*
 * spgemm_hip_extract.c -- a submatrix or an induced subgraph of a matrix, cut out on the GPU (include/bspgemm.h:
 * bspgemm_matrix_extract), beside the k-core, components and transpose-based drivers.
 *
 *     SpGEMM_hip_extract  A.mtx  [--rows FILE]  [--cols FILE]  [--keep-shape]  [-o OUT.mtx]
 *
 * The operand is what the loader hands back (readCOO, final/utils.c:47-81: the file transposed in memory), N rows of M
 * columns for a file of M x N.  The list files hold one 0-based index per line; without a file the list is "all".
 * Prints two lines: the shape  rows,cols,kept,ms  of the result (wall time of the call, the operand already on the
 * device) and the info line  scanned,hub_chunks,lanes,cols_monotone,sorted_by,canonicalised.
 * -o writes the result with bspgemm_write_mtx, such that the loader reconstructs exactly that operand.
 * A bad index ends the program with status 1 and the library's message on stderr.
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_extract  path-to-matrix  [--rows FILE]  [--cols FILE]  [--keep-shape]  [-o path-to-result]\n");
    exit(1);
}

/* one integer per line; *n entries */
static int *read_list(const char *path, int *n)
{
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
    size_t cap = 1024, k = 0;
    int *x = malloc(cap * sizeof(int));
    long long v;
    int got;
    if (!x) exit(1);
    while ((got = fscanf(f, "%lld", &v)) == 1) {
        if (k == cap) {
            cap *= 2;
            x = realloc(x, cap * sizeof(int));
            if (!x) exit(1);
        }
        if (v < -2147483647ll || v > 2147483647ll || k >= 2147483647u) { fprintf(stderr, "%s: entry %zu does not fit an int\n", path, k); exit(1); }
        x[k++] = (int)v;
    }
    if (got != EOF) { fprintf(stderr, "%s: entry %zu is not an integer\n", path, k); exit(1); }
    fclose(f);
    *n = (int)k;
    return x;
}

int main(int argc, char **argv)
{
    const char *rows_path = NULL, *cols_path = NULL, *out_path = NULL;
    unsigned flags = 0;
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        if (cli_flag(argv[i], "--keep-shape")) flags |= BSPGEMM_EXTRACT_KEEP_SHAPE;
        else if (!cli_value(argc, argv, &i, "--rows", &rows_path) && !cli_value(argc, argv, &i, "--cols", &cols_path) &&
                 !cli_value(argc, argv, &i, "-o", &out_path))
            usage();
    }
    uint32_t *Arow, *Acol, M, N, nnz;
    cli_load(argv[1], 0, &Arow, &Acol, &M, &N, &nnz);
    int ni = 0, nj = 0;
    int *I = rows_path ? read_list(rows_path, &ni) : NULL, *J = cols_path ? read_list(cols_path, &nj) : NULL;
    bspgemm_context *ctx = cli_context(0);
    bspgemm_matrix *A, *S;
    bspgemm_extract_info info;
    CHECK(bspgemm_matrix_upload(ctx, (int)N, (int)M, (const int *)Arow, (const int *)Acol, &A), "upload");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    double ms;
    CLI_TIMED(ms, ctx, bspgemm_matrix_extract(ctx, A, ni, I, nj, J, flags, &S, &info), "bspgemm_matrix_extract");
    const int rows = bspgemm_matrix_rows(S), cols = bspgemm_matrix_cols(S);
    printf("%d,%d,%lld,%.3f\n", rows, cols, (long long)info.kept, ms);
    printf("%lld,%lld,%d,%d,%d,%d\n", (long long)info.scanned, (long long)info.hub_chunks, info.lanes, info.cols_monotone,
           info.sorted_by, info.canonicalised);
    if (out_path) {
        int *rp = malloc(((size_t)rows + 1) * sizeof(int));
        int *ci = malloc((size_t)(info.kept > 0 ? info.kept : 1) * sizeof(int));
        if (!rp || !ci) exit(1);
        CHECK(bspgemm_matrix_download(ctx, S, rp, ci), "download");
        CHECK(bspgemm_write_mtx(out_path, rows, cols, rp, ci), "write");
        free(rp); free(ci);
    }
    bspgemm_matrix_free(S);
    bspgemm_matrix_free(A);
    bspgemm_destroy(ctx);
    free(I); free(J);
    free(Arow); free(Acol);
    return 0;
}
