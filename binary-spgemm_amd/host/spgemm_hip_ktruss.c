/*
 * spgemm_hip_ktruss.c -- triangle count and k-truss of an undirected graph, everything resident on the GPU: the
 * applications the counting masked product was added for (include/bspgemm.h: bspgemm_triangle_count, bspgemm_ktruss),
 * beside the closure driver (spgemm_hip_closure.c).
 *
 *     SpGEMM_hip_ktruss  [--symmetrize]  [--dot]  file.mtx  k  [out.mtx]
 *
 * --dot: both the count and the truss take their support from bspgemm_multiply_masked_dot (BSPGEMM_SUPPORT_DOT of
 * bspgemm_triangle_count_ex / bspgemm_ktruss_ex) instead of the counting product; the output is the same but for ms.
 * Prints one CSV line: n,nnz,triangles,k,truss_nnz,iterations,converged,ms.  file.mtx is read with
 * BSPGEMM_READ_EXPAND_SYMMETRIC, so a file that stores one triangle of a symmetric matrix gives the whole graph (nnz is the
 * expanded count); the loader hands back the transpose of the file's matrix (readCOO, final/utils.c:47-81), which for a
 * symmetric pattern is the matrix itself, and bspgemm_write_mtx writes T such that the loader reconstructs exactly T.
 * --symmetrize: the uploaded operand is replaced by A | A^T without its diagonal (bspgemm_matrix_symmetrize) before the
 * timer starts, so a `general` file of a directed graph gives the triangles and the truss of its underlying undirected
 * graph; nnz stays the loader's count.
 * ms: wall time of the triangle count and the k-truss together, operands already on the device.
 */
#include "cli_common.h"

int main(int argc, char **argv)
{
    int symmetrize = 0;
    bspgemm_support_method method = BSPGEMM_SUPPORT_PRODUCT;
    while (argc > 1 && strncmp(argv[1], "--", 2) == 0) {     /* the options, in any order */
        if (cli_flag(argv[1], "--symmetrize")) symmetrize = 1;
        else if (cli_flag(argv[1], "--dot")) method = BSPGEMM_SUPPORT_DOT;
        else break;
        argv++;
        argc--;
    }
    if (argc != 3 && argc != 4) {
        printf("usage: SpGEMM_hip_ktruss  [--symmetrize]  [--dot]  path-to-matrix  k  [path-to-truss]\n");
        exit(1);
    }
    const int k = atoi(argv[2]);
    cli_session s = cli_open(argv[1], BSPGEMM_READ_EXPAND_SYMMETRIC, "k-truss");
    const uint32_t M = s.M, nnz = s.nnz;
    bspgemm_context *ctx = s.ctx = cli_context(0);  /* open, not cli_upload: a synchronise only after --symmetrize */
    bspgemm_matrix *A, *T;
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)s.Arow, (const int *)s.Acol, &A), "upload");
    if (symmetrize) {
        bspgemm_matrix *U;
        CHECK(bspgemm_matrix_symmetrize(ctx, A, BSPGEMM_SYMMETRIZE_DROP_DIAGONAL, &U), "bspgemm_matrix_symmetrize");
        bspgemm_matrix_free(A);
        A = U;
        CHECK(bspgemm_synchronize(ctx), "synchronize");
    }
    s.A = A;
    const struct timespec t0 = cli_now();
    int64_t triangles = 0;
    int iterations = 0, converged = 0;
    CHECK(bspgemm_triangle_count_ex(ctx, A, method, &triangles), "bspgemm_triangle_count");
    CHECK(bspgemm_ktruss_ex(ctx, A, k, 0, method, &T, &iterations, &converged), "bspgemm_ktruss");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const double ms = cli_ms(t0, cli_now());
    const long long tn = bspgemm_matrix_nnz(T);
    printf("%u,%u,%lld,%d,%lld,%d,%d,%.3f\n", M, nnz, (long long)triangles, k, tn, iterations, converged, ms);
    if (argc == 4) {
        int *rp = malloc(((size_t)M + 1) * sizeof(int));
        int *ci = malloc((size_t)(tn > 0 ? tn : 1) * sizeof(int));
        if (!rp || !ci) exit(1);
        CHECK(bspgemm_matrix_download(ctx, T, rp, ci), "download");
        CHECK(bspgemm_write_mtx(argv[3], (int)M, (int)M, rp, ci), "write");
        free(rp); free(ci);
    }
    bspgemm_matrix_free(T);
    cli_close(&s);
    return 0;
}
