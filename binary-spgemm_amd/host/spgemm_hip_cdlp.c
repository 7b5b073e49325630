/*
 * spgemm_hip_cdlp.c -- community detection by synchronous label propagation on an undirected graph, everything resident
 * on the GPU (include/bspgemm.h: bspgemm_label_propagation), beside the connected-components, k-core and colouring drivers.
 *
 *     SpGEMM_hip_cdlp  file.mtx  [--iterations K]  [--labels out.txt]
 *
 * The transpose that the loader hands back (readCOO, final/utils.c:47-81) is used as it is: the call reads the entries as
 * undirected edges.  Every vertex starts with its own id as its label; K defaults to 10 (LDBC Graphalytics' choice).
 * Prints one line  n,nnz,communities,largest_community,iterations,converged,ms  -- the number of distinct labels, the size
 * of the largest community (counted on the host from the downloaded labels), the iterations the call ran, whether the last
 * of them changed nothing, and the call's wall time, the operand already on the device.
 * --labels writes one label per line, line v the label (a 0-based vertex id) of vertex v.
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_cdlp  path-to-matrix  [--iterations K]  [--labels out.txt]\n");
    exit(1);
}

int main(int argc, char **argv)
{
    const char *labels_path = NULL;
    int iterations = 10;
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        const char *val;
        if (cli_value(argc, argv, &i, "--iterations", &val)) {
            long long k;                /* (a value that overflows saturates past the bound: errno changes nothing here) */
            if (!cli_signed(val, 0, 0, 0x7fffffffLL, &k)) usage();
            iterations = (int)k;
        } else if (!cli_value(argc, argv, &i, "--labels", &labels_path)) {
            usage();
        }
    }
    cli_session s = cli_open(argv[1], 0, "label propagation");
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_matrix *P;
    bspgemm_lp_info info;
    double ms;
    CLI_TIMED(ms, s.ctx, bspgemm_label_propagation(s.ctx, s.A, NULL, iterations, &P, &info), "bspgemm_label_propagation");
    int *label = malloc(((size_t)M + 1) * sizeof(int));
    int *size = calloc((size_t)M + 1, sizeof(int));
    if (!label || !size) exit(1);
    CHECK(bspgemm_matrix_download(s.ctx, P, NULL, label), "download");
    int largest = 0;
    for (uint32_t v = 0; v < M; v++)
        if (++size[label[v]] > largest) largest = size[label[v]];
    if (labels_path) cli_write_ints(labels_path, label, M);
    printf("%u,%u,%d,%d,%d,%d,%.3f\n", M, s.nnz, info.communities, largest, info.iterations, info.converged, ms);
    free(label); free(size);
    bspgemm_matrix_free(P);
    cli_close(&s);
    return 0;
}
