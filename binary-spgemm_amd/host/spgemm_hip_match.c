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
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        const char *val;
        if (cli_value(argc, argv, &i, "--order", &val)) {
            if (strcmp(val, "natural") == 0) order = BSPGEMM_MATCH_NATURAL;
            else if (strcmp(val, "random") == 0) order = BSPGEMM_MATCH_RANDOM;
            else if (strcmp(val, "light") == 0) order = BSPGEMM_MATCH_LIGHT_FIRST;
            else usage();
        } else if (cli_value(argc, argv, &i, "--seed", &val)) {
            char *end;                  /* open: no errno or sign check, so "-1" and a value past 2^64 - 1 are taken and wrap */
            seed = (unsigned)strtoul(val, &end, 0);
            if (end == val || *end) usage();
        } else if (!cli_value(argc, argv, &i, "--out", &out_path)) {
            usage();
        }
    }
    cli_session s = cli_open(argv[1], 0, "matching");
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_matrix *P;
    int *mate = malloc(((size_t)M + 1) * sizeof(int));
    if (!mate) exit(1);
    bspgemm_match_info info;
    double ms;
    CLI_TIMED(ms, s.ctx, bspgemm_maximal_matching(s.ctx, s.A, order, seed, &P, mate, &info), "bspgemm_maximal_matching");
    if (out_path) {
        FILE *f = cli_create(out_path);
        for (uint32_t v = 0; v < M; v++)
            if (mate[v] > (int)v) fprintf(f, "%u %d\n", v, mate[v]);
        cli_finish(f, out_path);
    }
    printf("%u,%u,%lld,%d,%.3f\n", M, s.nnz, (long long)info.pairs, info.rounds, ms);
    free(mate);
    bspgemm_matrix_free(P);
    cli_close(&s);
    return 0;
}
