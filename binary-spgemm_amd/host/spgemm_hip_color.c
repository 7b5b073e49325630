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
    if (argc < 2 || argc % 2 != 0) usage();
    for (int i = 2; i < argc; i += 2) {
        if (strcmp(argv[i], "--order") == 0) {
            if (strcmp(argv[i + 1], "natural") == 0) order = BSPGEMM_COLOR_NATURAL;
            else if (strcmp(argv[i + 1], "random") == 0) order = BSPGEMM_COLOR_RANDOM;
            else if (strcmp(argv[i + 1], "largest") == 0) order = BSPGEMM_COLOR_LARGEST_FIRST;
            else usage();
        } else if (strcmp(argv[i], "--seed") == 0) {
            char *end;
            seed = (unsigned)strtoul(argv[i + 1], &end, 0);
            if (end == argv[i + 1] || *end) usage();
        } else if (strcmp(argv[i], "--colors") == 0) {
            colors_path = argv[i + 1];
        } else {
            usage();
        }
    }
    uint32_t *Arow, *Acol, M, N, nnz;
    cli_load(argv[1], 0, &Arow, &Acol, &M, &N, &nnz);
    cli_need_square("colouring", M, N);
    bspgemm_context *ctx = cli_context(0);
    bspgemm_matrix *A, *P;
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)Arow, (const int *)Acol, &A), "upload");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const struct timespec t0 = cli_now();
    int colors = 0, rounds = 0;
    CHECK(bspgemm_graph_coloring(ctx, A, order, seed, &P, &colors, &rounds), "bspgemm_graph_coloring");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const double ms = cli_ms(t0, cli_now());
    int *color = malloc(((size_t)M + 1) * sizeof(int));
    int *size = calloc((size_t)M + 1, sizeof(int));
    if (!color || !size) exit(1);
    CHECK(bspgemm_matrix_download(ctx, P, NULL, color), "download");
    int largest = 0;
    for (uint32_t v = 0; v < M; v++)
        if (++size[color[v]] > largest) largest = size[color[v]];
    if (colors_path) cli_write_ints(colors_path, color, M);
    printf("%u,%u,%d,%d,%d,%.3f\n", M, nnz, colors, largest, rounds, ms);
    free(color); free(size);
    bspgemm_matrix_free(P);
    bspgemm_matrix_free(A);
    bspgemm_destroy(ctx);
    free(Arow); free(Acol);
    return 0;
}
