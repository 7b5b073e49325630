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
        if (cli_flag(argv[i], "--directed")) flags = BSPGEMM_LCC_DIRECTED;
        else if (!cli_value(argc, argv, &i, "--out", &out_path)) usage();
    }
    cli_session s = cli_open(argv[1], 0, "the clustering coefficient");
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_result *counts;
    int *degree = malloc(((size_t)M + 1) * sizeof(int));
    double *lcc = malloc(((size_t)M + 1) * sizeof(double));
    if (!degree || !lcc) exit(1);
    bspgemm_lcc_info info;
    double ms;
    CLI_TIMED(ms, s.ctx, bspgemm_local_clustering(s.ctx, s.A, flags, &counts, degree, lcc, &info), "bspgemm_local_clustering");
    double sum = 0;
    int max_degree = 0;
    for (uint32_t v = 0; v < M; v++) {
        sum += lcc[v];
        if (degree[v] > max_degree) max_degree = degree[v];
    }
    if (out_path) {
        FILE *f = cli_create(out_path);
        for (uint32_t v = 0; v < M; v++) fprintf(f, "%u %.17g\n", v, lcc[v]);
        cli_finish(f, out_path);
    }
    printf("%u,%u,%lld,%.17g,%d,%.3f\n", M, s.nnz, (long long)info.triangles, M ? sum / M : 0.0, max_degree, ms);
    free(degree); free(lcc);
    bspgemm_result_free(counts);
    cli_close(&s);
    return 0;
}
