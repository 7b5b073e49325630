/*
 * spgemm_hip_color.c -- greedy colouring of an undirected graph, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_graph_coloring), beside the connected-components, k-core and strong-components drivers.
 *
 *     SpGEMM_hip_color  file.mtx  [--order natural|random|largest]  [--seed S]  [--colors out.txt]
 *
 * The transpose that the loader hands back (readCOO, final/utils.c:47-81) is used as it is: the call reads the entries as
 * undirected edges.  The order defaults to random, the seed to 0.
 * Prints one line  n,nnz,colors,largest_class,rounds,ms  -- the number of colours, the size of the largest colour class
 * (counted on the host from the downloaded colours), the frontier launches the call took and its wall time, the operand
 * already on the device.
 * --colors writes one colour per line, line v the colour (0-based) of vertex v.
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_color  path-to-matrix  [--order natural|random|largest]  [--seed S]  [--colors out.txt]\n");
    exit(1);
}

int main(int argc, char **argv)
{
    const char *colors_path = NULL;
    bspgemm_color_order order = BSPGEMM_COLOR_RANDOM;
    unsigned seed = 0;
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        const char *val;
        if (cli_value(argc, argv, &i, "--order", &val)) {
            if (strcmp(val, "natural") == 0) order = BSPGEMM_COLOR_NATURAL;
            else if (strcmp(val, "random") == 0) order = BSPGEMM_COLOR_RANDOM;
            else if (strcmp(val, "largest") == 0) order = BSPGEMM_COLOR_LARGEST_FIRST;
            else usage();
        } else if (cli_value(argc, argv, &i, "--seed", &val)) {
            char *end;                  /* open: no errno or sign check, so "-1" and a value past 2^64 - 1 are taken and wrap */
            seed = (unsigned)strtoul(val, &end, 0);
            if (end == val || *end) usage();
        } else if (!cli_value(argc, argv, &i, "--colors", &colors_path)) {
            usage();
        }
    }
    cli_session s = cli_open(argv[1], 0, "colouring");
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_matrix *P;
    int colors = 0, rounds = 0;
    double ms;
    CLI_TIMED(ms, s.ctx, bspgemm_graph_coloring(s.ctx, s.A, order, seed, &P, &colors, &rounds), "bspgemm_graph_coloring");
    int *color = malloc(((size_t)M + 1) * sizeof(int));
    int *size = calloc((size_t)M + 1, sizeof(int));
    if (!color || !size) exit(1);
    CHECK(bspgemm_matrix_download(s.ctx, P, NULL, color), "download");
    int largest = 0;
    for (uint32_t v = 0; v < M; v++)
        if (++size[color[v]] > largest) largest = size[color[v]];
    if (colors_path) cli_write_ints(colors_path, color, M);
    printf("%u,%u,%d,%d,%d,%.3f\n", M, s.nnz, colors, largest, rounds, ms);
    free(color); free(size);
    bspgemm_matrix_free(P);
    cli_close(&s);
    return 0;
}
