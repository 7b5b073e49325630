/*
 * spgemm_hip_closure.c -- reflexive-transitive closure of a pattern matrix by repeated boolean
 * squaring, everything resident on the GPU (the application the reference's
 * report motivates the kernel with -- its old/BSpGEMM.c:75-126 keeps an OR-accumulating variant).
 *
 *     SpGEMM_hip_closure  A.mtx  [C_out.mtx]
 *
 * Prints: path,n,nnz(A),products_computed,nnz(closure),seconds.  A.mtx is read like every other
 * input (readCOO, final/utils.c:47-81: transposed in memory; the closure of the transpose is the
 * transpose of the closure, and the writer transposes back).
 */
#include "cli_common.h"

int main(int argc, char **argv)
{
    if (argc != 2 && argc != 3) {
        printf("usage: SpGEMM_hip_closure  path-to-matrix  [path-to-result]\n");
        exit(1);
    }
    cli_session s = cli_open(argv[1], 0, "closure");
    const uint32_t M = s.M;
    bspgemm_context *ctx = s.ctx = cli_context(0);  /* open, not cli_upload: no synchronise stands before this timer */
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)s.Arow, (const int *)s.Acol, &s.A), "upload");
    const struct timespec t0 = cli_now();
    bspgemm_result *T;
    int products = 0;
    CHECK(bspgemm_closure(ctx, s.A, 64, &T, &products), "bspgemm_closure");
    const double secs = cli_ms(t0, cli_now()) * 1e-3;
    printf("%s,%u,%u,%d,%lld,%lf\n", argv[1], M, s.nnz, products, (long long)bspgemm_result_nnz(T), secs);
    if (argc == 3) {
        const long long tn = bspgemm_result_nnz(T);
        int64_t *rp = malloc(((size_t)M + 1) * sizeof(int64_t));
        int *ci = malloc((size_t)(tn > 0 ? tn : 1) * sizeof(int));
        if (!rp || !ci) exit(1);
        CHECK(bspgemm_result_download(ctx, T, rp, ci), "download");
        CHECK(bspgemm_write_result_mtx(argv[2], (int)M, (int)M, rp, ci), "write");
        free(rp); free(ci);
    }
    bspgemm_result_free(T);
    cli_close(&s);
    return 0;
}
