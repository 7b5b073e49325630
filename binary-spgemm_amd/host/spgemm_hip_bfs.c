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
#include <errno.h>
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
        char *end;
        errno = 0;
        const long v = strtol(argv[2 + i], &end, 10);
        if (errno || end == argv[2 + i] || *end || v < INT_MIN || v > INT_MAX) {
            fprintf(stderr, "source %d (\"%s\") is not a vertex id\n", i, argv[2 + i]);
            exit(1);
        }
        sources[i] = (int)v;
    }
    uint32_t *Arow, *Acol, M, N, nnz;
    cli_load(argv[1], 0, &Arow, &Acol, &M, &N, &nnz);
    cli_need_square("bfs", M, N);
    bspgemm_context *ctx = cli_context(0);
    bspgemm_matrix *At, *A;
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)Arow, (const int *)Acol, &At), "upload");
    CHECK(bspgemm_matrix_transpose(ctx, At, &A), "bspgemm_matrix_transpose");
    bspgemm_matrix_free(At);
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const struct timespec t0 = cli_now();
    bspgemm_result *L;
    int depth = 0, complete = 0;
    CHECK(bspgemm_bfs(ctx, A, S, sources, 0, &L, &depth, &complete), "bspgemm_bfs");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const double ms = cli_ms(t0, cli_now());
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
    printf("%u,%u,%d,%d,%d,%.3f\n", M, nnz, S, depth, complete, ms);
    free(rp); free(lv); free(sources);
    bspgemm_result_free(L);
    bspgemm_matrix_free(A);
    bspgemm_destroy(ctx);
    free(Arow); free(Acol);
    return 0;
}
