/*
 * spgemm_hip_lcc.c -- the local clustering coefficient of every vertex, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_local_clustering), beside the k-core, colouring and label-propagation drivers.
 *
 *     SpGEMM_hip_lcc  file.mtx  [--directed]  [--out lcc.txt]
 *
 * The transpose that the loader hands back (readCOO, final/utils.c:47-81) is used as it is: the neighbourhoods are those of
 * the undirected graph, and the directed count is invariant under transposition, so the in-edges give the file's answer.
 * Prints one line  n,nnz,triangles,mean_lcc,max_degree,ms  -- the triangles of the undirected graph, the mean of the
 * coefficients over all n vertices (%.17g; 0 for n == 0), the largest degree, and the call's wall time, the operand already
 * on the device.
 * --out writes one line per vertex, "vertex lcc", the vertex 0-based and the coefficient with %.17g.
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_lcc  path-to-matrix  [--directed]  [--out lcc.txt]\n");
    exit(1);
}

int main(int argc, char **argv)
{
    const char *out_path = NULL;
    unsigned flags = 0;
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        if (strcmp(argv[i], "--directed") == 0) {
            flags = BSPGEMM_LCC_DIRECTED;
        } else if (strcmp(argv[i], "--out") == 0 && i + 1 < argc) {
            out_path = argv[++i];
        } else {
            usage();
        }
    }
    uint32_t *Arow, *Acol, M, N, nnz;
    cli_load(argv[1], 0, &Arow, &Acol, &M, &N, &nnz);
    cli_need_square("the clustering coefficient", M, N);
    bspgemm_context *ctx = cli_context(0);
    bspgemm_matrix *A;
    bspgemm_result *counts;
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)Arow, (const int *)Acol, &A), "upload");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    int *degree = malloc(((size_t)M + 1) * sizeof(int));
    double *lcc = malloc(((size_t)M + 1) * sizeof(double));
    if (!degree || !lcc) exit(1);
    const struct timespec t0 = cli_now();
    bspgemm_lcc_info info;
    CHECK(bspgemm_local_clustering(ctx, A, flags, &counts, degree, lcc, &info), "bspgemm_local_clustering");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const double ms = cli_ms(t0, cli_now());
    double sum = 0;
    int max_degree = 0;
    for (uint32_t v = 0; v < M; v++) {
        sum += lcc[v];
        if (degree[v] > max_degree) max_degree = degree[v];
    }
    if (out_path) {
        FILE *f = fopen(out_path, "w");
        if (!f) { fprintf(stderr, "cannot write %s\n", out_path); exit(1); }
        for (uint32_t v = 0; v < M; v++) fprintf(f, "%u %.17g\n", v, lcc[v]);
        if (fclose(f)) { fprintf(stderr, "cannot write %s\n", out_path); exit(1); }
    }
    printf("%u,%u,%lld,%.17g,%d,%.3f\n", M, nnz, (long long)info.triangles, M ? sum / M : 0.0, max_degree, ms);
    free(degree); free(lcc);
    bspgemm_result_free(counts);
    bspgemm_matrix_free(A);
    bspgemm_destroy(ctx);
    free(Arow); free(Acol);
    return 0;
}
