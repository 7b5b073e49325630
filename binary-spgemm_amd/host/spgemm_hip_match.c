/*
 * spgemm_hip_match.c -- maximal matching of an undirected graph, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_maximal_matching), beside the colouring, connected-components and k-core drivers.
 *
 *     SpGEMM_hip_match  file.mtx  [--order natural|random|light]  [--seed S]  [--out pairs.txt]
 *
 * The transpose that the loader hands back (readCOO, final/utils.c:47-81) is used as it is: the call reads the entries as
 * undirected edges.  The order defaults to random, the seed to 0.
 * Prints one line  n,nnz,pairs,rounds,ms  -- the matched edges, the rounds the call took and its wall time, the operand
 * already on the device.
 * --out writes one line "v mate" per matched edge, v < mate, v ascending (0-based).
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_match  path-to-matrix  [--order natural|random|light]  [--seed S]  [--out pairs.txt]\n");
    exit(1);
}

int main(int argc, char **argv)
{
    const char *out_path = NULL;
    bspgemm_match_order order = BSPGEMM_MATCH_RANDOM;
    unsigned seed = 0;
    if (argc < 2 || argc % 2 != 0) usage();
    for (int i = 2; i < argc; i += 2) {
        if (strcmp(argv[i], "--order") == 0) {
            if (strcmp(argv[i + 1], "natural") == 0) order = BSPGEMM_MATCH_NATURAL;
            else if (strcmp(argv[i + 1], "random") == 0) order = BSPGEMM_MATCH_RANDOM;
            else if (strcmp(argv[i + 1], "light") == 0) order = BSPGEMM_MATCH_LIGHT_FIRST;
            else usage();
        } else if (strcmp(argv[i], "--seed") == 0) {
            char *end;
            seed = (unsigned)strtoul(argv[i + 1], &end, 0);
            if (end == argv[i + 1] || *end) usage();
        } else if (strcmp(argv[i], "--out") == 0) {
            out_path = argv[i + 1];
        } else {
            usage();
        }
    }
    uint32_t *Arow, *Acol, M, N, nnz;
    cli_load(argv[1], 0, &Arow, &Acol, &M, &N, &nnz);
    cli_need_square("matching", M, N);
    bspgemm_context *ctx = cli_context(0);
    bspgemm_matrix *A, *P;
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)Arow, (const int *)Acol, &A), "upload");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    int *mate = malloc(((size_t)M + 1) * sizeof(int));
    if (!mate) exit(1);
    const struct timespec t0 = cli_now();
    bspgemm_match_info info;
    CHECK(bspgemm_maximal_matching(ctx, A, order, seed, &P, mate, &info), "bspgemm_maximal_matching");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const double ms = cli_ms(t0, cli_now());
    if (out_path) {
        FILE *f = fopen(out_path, "w");
        if (!f) { fprintf(stderr, "cannot write %s\n", out_path); exit(1); }
        for (uint32_t v = 0; v < M; v++)
            if (mate[v] > (int)v) fprintf(f, "%u %d\n", v, mate[v]);
        if (fclose(f)) { fprintf(stderr, "cannot write %s\n", out_path); exit(1); }
    }
    printf("%u,%u,%lld,%d,%.3f\n", M, nnz, (long long)info.pairs, info.rounds, ms);
    free(mate);
    bspgemm_matrix_free(P);
    bspgemm_matrix_free(A);
    bspgemm_destroy(ctx);
    free(Arow); free(Acol);
    return 0;
}
