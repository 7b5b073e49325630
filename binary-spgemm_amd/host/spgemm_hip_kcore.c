/*
 * spgemm_hip_kcore.c -- k-core decomposition of a graph, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_core_numbers, bspgemm_kcore), beside the closure, k-truss, BFS and components drivers.
 *
 *     SpGEMM_hip_kcore  file.mtx  [--numbers out.txt]  [--k K --out core.mtx]
 *
 * The file's entries are read as undirected edges, so the transpose that the loader hands back (readCOO,
 * final/utils.c:47-81) is used as it is: the call symmetrizes its operand.
 * Prints one line  n,nnz,degeneracy,top,rounds,ms  -- the largest core number, the number of vertices that have it
 * (counted on the host from the downloaded values), the peel launches the call took and its wall time, the operand already
 * on the device.
 * --numbers writes one core number per line, line v that of vertex v (0-based).
 * --k K --out writes the K-core (bspgemm_kcore: the subgraph induced by the vertices of core number >= K, both directions
 * of every edge) with bspgemm_write_mtx, such that the loader reconstructs exactly that operand.
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_kcore  path-to-matrix  [--numbers out.txt]  [--k K --out path-to-core]\n");
    exit(1);
}

int main(int argc, char **argv)
{
    const char *numbers_path = NULL, *out_path = NULL, *k_arg = NULL;
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        if (!cli_value(argc, argv, &i, "--numbers", &numbers_path) && !cli_value(argc, argv, &i, "--k", &k_arg) &&
            !cli_value(argc, argv, &i, "--out", &out_path))
            usage();
    }
    if ((k_arg == NULL) != (out_path == NULL)) usage();
    cli_session s = cli_open(argv[1], 0, "k-core");
    const uint32_t M = s.M, nnz = s.nnz;
    cli_upload(&s);
    bspgemm_context *ctx = s.ctx;
    bspgemm_matrix *A = s.A;
    bspgemm_result *R;
    int degeneracy = 0, rounds = 0;
    double ms;
    CLI_TIMED(ms, ctx, bspgemm_core_numbers(ctx, A, &R, &degeneracy, &rounds), "bspgemm_core_numbers");
    int *core = malloc(((size_t)M + 1) * sizeof(int));
    if (!core) exit(1);
    CHECK(bspgemm_result_download_values(ctx, R, core), "download");
    int top = 0;
    for (uint32_t v = 0; v < M; v++) top += core[v] == degeneracy;
    if (numbers_path) cli_write_ints(numbers_path, core, M);
    printf("%u,%u,%d,%d,%d,%.3f\n", M, nnz, degeneracy, top, rounds, ms);
    if (out_path) {
        bspgemm_matrix *T;
        CHECK(bspgemm_kcore(ctx, A, atoi(k_arg), &T, NULL), "bspgemm_kcore");
        const long long tn = bspgemm_matrix_nnz(T);
        int *rp = malloc(((size_t)M + 1) * sizeof(int));
        int *ci = malloc((size_t)(tn > 0 ? tn : 1) * sizeof(int));
        if (!rp || !ci) exit(1);
        CHECK(bspgemm_matrix_download(ctx, T, rp, ci), "download");
        CHECK(bspgemm_write_mtx(out_path, (int)M, (int)M, rp, ci), "write");
        free(rp); free(ci);
        bspgemm_matrix_free(T);
    }
    free(core);
    bspgemm_result_free(R);
    cli_close(&s);
    return 0;
}
