/*
 * spgemm_hip_bfs_tree.c -- single-source direction-optimising breadth-first search with parents and levels, everything
 * resident on the GPU (include/bspgemm.h: bspgemm_bfs_tree), beside the multi-source driver (spgemm_hip_bfs.c).
 *
 *     SpGEMM_hip_bfs_tree  file.mtx  source  [--push|--pull]  [--symmetric]
 *
 * A file entry `i j` is the edge i -> j (1-based in the file); the source is a 0-based vertex id.  The loader hands back
 * the transpose of the file's matrix (readCOO, final/utils.c:47-81): that is the in-edge operand AT, and it is transposed
 * once on the device, before the timer starts, for the out-edge operand A.  --symmetric: the file holds every edge both
 * ways, and the one operand is passed as A and as AT.  --push / --pull force the direction of every level.
 * Prints  source,reached,depth,sum_of_levels,sum_of_parents  and then  n,nnz,push_levels,pull_levels,ms.  ms: wall time
 * of bspgemm_bfs_tree, the operands already on the device.
 */
#include "cli_common.h"
#include <errno.h>
#include <limits.h>

int main(int argc, char **argv)
{
    bspgemm_bfs_direction dir = BSPGEMM_BFS_AUTO;
    int symmetric = 0, bad = argc < 3;
    for (int i = 3; i < argc && !bad; i++) {
        if (!strcmp(argv[i], "--push")) dir = BSPGEMM_BFS_PUSH;
        else if (!strcmp(argv[i], "--pull")) dir = BSPGEMM_BFS_PULL;
        else if (!strcmp(argv[i], "--symmetric")) symmetric = 1;
        else bad = 1;
    }
    if (bad) {
        printf("usage: SpGEMM_hip_bfs_tree  path-to-matrix  source  [--push|--pull]  [--symmetric]\n");
        exit(1);
    }
    char *end;
    errno = 0;
    const long src = strtol(argv[2], &end, 10);
    if (errno || end == argv[2] || *end || src < INT_MIN || src > INT_MAX) {
        fprintf(stderr, "source (\"%s\") is not a vertex id\n", argv[2]);
        exit(1);
    }
    uint32_t *Arow, *Acol, M, N, nnz;
    cli_load(argv[1], 0, &Arow, &Acol, &M, &N, &nnz);
    cli_need_square("bfs_tree", M, N);
    bspgemm_context *ctx = cli_context(0);
    bspgemm_matrix *At, *A;
    CHECK(bspgemm_matrix_upload(ctx, (int)M, (int)M, (const int *)Arow, (const int *)Acol, &At), "upload");
    if (symmetric) A = At;
    else CHECK(bspgemm_matrix_transpose(ctx, At, &A), "bspgemm_matrix_transpose");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const struct timespec t0 = cli_now();
    bspgemm_result *T;
    bspgemm_bfs_tree_info info;
    CHECK(bspgemm_bfs_tree(ctx, A, At, (int)src, dir, 0, &T, &info), "bspgemm_bfs_tree");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    const double ms = cli_ms(t0, cli_now());
    const long long reached = bspgemm_result_nnz(T);
    int64_t *rp = malloc(((size_t)M + 1) * sizeof(int64_t));
    int *parent = malloc((size_t)(reached > 0 ? reached : 1) * sizeof(int));
    int *level = malloc((size_t)(reached > 0 ? reached : 1) * sizeof(int));
    if (!rp || !parent || !level) exit(1);
    CHECK(bspgemm_result_download(ctx, T, rp, parent), "download");
    CHECK(bspgemm_result_download_values(ctx, T, level), "download_values");
    long long sum_levels = 0, sum_parents = 0;
    for (long long p = 0; p < reached; p++) {
        sum_levels += level[p];
        sum_parents += parent[p];
    }
    printf("%ld,%lld,%d,%lld,%lld\n", src, reached, info.depth, sum_levels, sum_parents);
    printf("%u,%u,%d,%d,%.3f\n", M, nnz, info.push_levels, info.pull_levels, ms);
    free(rp); free(parent); free(level);
    bspgemm_result_free(T);
    if (!symmetric) bspgemm_matrix_free(A);
    bspgemm_matrix_free(At);
    bspgemm_destroy(ctx);
    free(Arow); free(Acol);
    return 0;
}
