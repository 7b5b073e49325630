/*
 * spgemm_hip_cc.c -- connected components of a graph, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_connected_components), beside the closure, k-truss and BFS drivers.
 *
 *     SpGEMM_hip_cc  file.mtx  [--labels out.txt]
 *
 * The file's entries are read as undirected edges, so the transpose that the loader hands back (readCOO,
 * final/utils.c:47-81) is used as it is: weak connectivity ignores direction.
 * Prints one line  n,nnz,components,largest,rounds,ms  -- the number of components, the size of the largest one (counted
 * on the host from the downloaded labels), the rounds the call took and its wall time, the operand already on the device.
 * --labels writes one label per line, line v the smallest vertex id (0-based) of v's component.
 */
#include "cli_common.h"

int main(int argc, char **argv)
{
    const char *labels_path = NULL;
    if (argc == 4 && strcmp(argv[2], "--labels") == 0) labels_path = argv[3];
    if (argc != 2 && !labels_path) {
        printf("usage: SpGEMM_hip_cc  path-to-matrix  [--labels out.txt]\n");
        exit(1);
    }
    cli_session s = cli_open(argv[1], 0, "cc");
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_matrix *P;
    int components = 0, rounds = 0;
    double ms;
    CLI_TIMED(ms, s.ctx, bspgemm_connected_components(s.ctx, s.A, &P, &components, &rounds), "bspgemm_connected_components");
    int *label = malloc(((size_t)M + 1) * sizeof(int));
    int *size = calloc((size_t)M + 1, sizeof(int));
    if (!label || !size) exit(1);
    CHECK(bspgemm_matrix_download(s.ctx, P, NULL, label), "download");
    int largest = 0;
    for (uint32_t v = 0; v < M; v++)
        if (++size[label[v]] > largest) largest = size[label[v]];
    if (labels_path) cli_write_ints(labels_path, label, M);
    printf("%u,%u,%d,%d,%d,%.3f\n", M, s.nnz, components, largest, rounds, ms);
    free(label); free(size);
    bspgemm_matrix_free(P);
    cli_close(&s);
    return 0;
}
