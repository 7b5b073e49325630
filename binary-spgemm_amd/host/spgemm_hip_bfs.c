/*
 * spgemm_hip_bfs.c -- multi-source breadth-first search of a directed graph, everything resident on the GPU: the
 * application the complemented mask was added for (include/bspgemm.h: bspgemm_bfs), beside the closure and k-truss
 * drivers (spgemm_hip_closure.c, spgemm_hip_ktruss.c).
 *
 *     SpGEMM_hip_bfs  file.mtx  source  [source ...]
 *
 * A file entry `i j` is the edge i -> j (1-based in the file); the sources on the command line are 0-based vertex ids.
 * The loader hands back the transpose of the file's matrix (readCOO, final/utils.c:47-81), so the operand is transposed
 * once on the device before the timer starts.
 * Prints one line per source, in the order given:  source,reached,eccentricity,sum_of_levels  -- the vertices reachable
 * from it (itself included), the largest level among them and the sum of their levels -- and then one line
 * n,nnz,nsources,depth,complete,ms.  ms: wall time of bspgemm_bfs, the operand already on the device.
 */
#include "cli_common.h"
#include <limits.h>

int main(int argc, char **argv)
{
    if (argc < 3) {
        printf("usage: SpGEMM_hip_bfs  path-to-matrix  source  [source ...]\n");
        exit(1);
    }
    const int S = argc - 2;
    int *sources = malloc((size_t)S * sizeof(int));
    if (!sources) exit(1);
    for (int i = 0; i < S; i++) {
        long long v;
        if (!cli_signed(argv[2 + i], 10, INT_MIN, INT_MAX, &v)) {
            fprintf(stderr, "source %d (\"%s\") is not a vertex id\n", i, argv[2 + i]);
            exit(1);
        }
        sources[i] = (int)v;
    }
    cli_session s = cli_open(argv[1], 0, "bfs");
    cli_upload(&s);
    bspgemm_context *ctx = s.ctx;
    bspgemm_matrix *A;                                /* the out-edge operand replaces the loader's transpose */
    CHECK(bspgemm_matrix_transpose(ctx, s.A, &A), "bspgemm_matrix_transpose");
    bspgemm_matrix_free(s.A);
    s.A = A;
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    bspgemm_result *L;
    int depth = 0, complete = 0;
    double ms;
    CLI_TIMED(ms, ctx, bspgemm_bfs(ctx, A, S, sources, 0, &L, &depth, &complete), "bspgemm_bfs");
    const long long total = bspgemm_result_nnz(L);
    int64_t *rp = malloc(((size_t)S + 1) * sizeof(int64_t));
    int *lv = malloc((size_t)(total > 0 ? total : 1) * sizeof(int));
    if (!rp || !lv) exit(1);
    CHECK(bspgemm_result_download(ctx, L, rp, NULL), "download");
    CHECK(bspgemm_result_download_values(ctx, L, lv), "download_values");
    for (int i = 0; i < S; i++) {
        long long sum = 0;
        int ecc = 0;
        for (int64_t p = rp[i]; p < rp[i + 1]; p++) {
            sum += lv[p];
            if (lv[p] > ecc) ecc = lv[p];
        }
        printf("%d,%lld,%d,%lld\n", sources[i], (long long)(rp[i + 1] - rp[i]), ecc, sum);
    }
    printf("%u,%u,%d,%d,%d,%.3f\n", s.M, s.nnz, S, depth, complete, ms);
    free(rp); free(lv); free(sources);
    bspgemm_result_free(L);
    cli_close(&s);
    return 0;
}
