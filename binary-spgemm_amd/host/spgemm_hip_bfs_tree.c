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
#include <limits.h>

int main(int argc, char **argv)
{
    bspgemm_bfs_direction dir = BSPGEMM_BFS_AUTO;
    int symmetric = 0, bad = argc < 3;
    for (int i = 3; i < argc && !bad; i++) {
        if (cli_flag(argv[i], "--push")) dir = BSPGEMM_BFS_PUSH;
        else if (cli_flag(argv[i], "--pull")) dir = BSPGEMM_BFS_PULL;
        else if (cli_flag(argv[i], "--symmetric")) symmetric = 1;
        else bad = 1;
    }
    if (bad) {
        printf("usage: SpGEMM_hip_bfs_tree  path-to-matrix  source  [--push|--pull]  [--symmetric]\n");
        exit(1);
    }
    long long src;
    if (!cli_signed(argv[2], 10, INT_MIN, INT_MAX, &src)) {
        fprintf(stderr, "source (\"%s\") is not a vertex id\n", argv[2]);
        exit(1);
    }
    cli_session s = cli_open(argv[1], 0, "bfs_tree");                     /* s.A: the in-edge operand AT */
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_context *ctx = s.ctx;
    bspgemm_matrix *A = s.A;
    if (!symmetric) CHECK(bspgemm_matrix_transpose(ctx, s.A, &A), "bspgemm_matrix_transpose");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    bspgemm_result *T;
    bspgemm_bfs_tree_info info;
    double ms;
    CLI_TIMED(ms, ctx, bspgemm_bfs_tree(ctx, A, s.A, (int)src, dir, 0, &T, &info), "bspgemm_bfs_tree");
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
    printf("%lld,%lld,%d,%lld,%lld\n", src, reached, info.depth, sum_levels, sum_parents);
    printf("%u,%u,%d,%d,%.3f\n", M, s.nnz, info.push_levels, info.pull_levels, ms);
    free(rp); free(parent); free(level);
    bspgemm_result_free(T);
    if (!symmetric) bspgemm_matrix_free(A);
    cli_close(&s);
    return 0;
}
