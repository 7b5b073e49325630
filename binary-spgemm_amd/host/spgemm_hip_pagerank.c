/*
 * spgemm_hip_pagerank.c -- PageRank in 64-bit fixed point, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_pagerank).
 *
 *     SpGEMM_hip_pagerank  file.mtx  [iterations]  [damping]  [--push|--pull]  [--symmetric]  [--tolerance x]  [--top k]
 *
 * A file entry `i j` is the edge i -> j (1-based in the file).  The loader hands back the transpose of the file's matrix
 * (readCOO, final/utils.c:47-81): that is the in-edge operand AT, and it is transposed once on the device, before the timer
 * starts, for the out-edge operand A.  --symmetric: the file holds every edge both ways, and the one operand is passed as A
 * and as AT.  iterations: default 20; damping: default 0.85; --tolerance x > 0 ends the loop at the first iteration whose L1
 * change is at most x; --top k: default 10.
 * Prints  n,nnz,dangling,iterations,delta,mass,ms  and then the k highest-ranked vertices, ties to the smaller id, as
 * vertex,fixed,double  (0-based ids; fixed: 2^62 = 1.0).  ms: wall time of bspgemm_pagerank, the operands already on the
 * device.
 */
#include "cli_common.h"
#include <inttypes.h>

static const uint64_t *g_rank;

static int by_rank(const void *a, const void *b)
{
    const int x = *(const int *)a, y = *(const int *)b;
    if (g_rank[x] != g_rank[y]) return g_rank[x] > g_rank[y] ? -1 : 1;
    return x < y ? -1 : x > y;
}

static void usage(void)
{
    printf("usage: SpGEMM_hip_pagerank  path-to-matrix  [iterations]  [damping]  [--push|--pull]  [--symmetric]  "
           "[--tolerance x]  [--top k]\n");
    exit(1);
}

/* open: every number here goes through strtod ("1e1" iterations are ten), which no whole-number parser accepts */
static double number(const char *text)
{
    char *end;
    errno = 0;
    const double x = strtod(text, &end);
    if (errno || end == text || *end) usage();
    return x;
}

int main(int argc, char **argv)
{
    bspgemm_pr_method method = BSPGEMM_PR_AUTO;
    int symmetric = 0, positional = 0;
    double iterations = 20, damping = 0.85, tolerance = 0.0, top = 10;
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        const char *val;
        if (cli_flag(argv[i], "--push")) method = BSPGEMM_PR_PUSH;
        else if (cli_flag(argv[i], "--pull")) method = BSPGEMM_PR_PULL;
        else if (cli_flag(argv[i], "--symmetric")) symmetric = 1;
        else if (cli_value(argc, argv, &i, "--tolerance", &val)) tolerance = number(val);
        else if (cli_value(argc, argv, &i, "--top", &val)) top = number(val);
        else if (argv[i][0] != '-' && positional == 0) { iterations = number(argv[i]); positional = 1; }
        else if (argv[i][0] != '-' && positional == 1) { damping = number(argv[i]); positional = 2; }
        else usage();
    }
    if (!(iterations >= 0 && iterations <= 1e9) || iterations != (int)iterations || !(top >= 0 && top <= 1e9) ||
        top != (int)top || !(damping >= 0 && damping <= 1) || !(tolerance >= 0))
        usage();
    cli_session s = cli_open(argv[1], 0, "pagerank");                     /* s.A: the in-edge operand AT */
    const uint32_t M = s.M, nnz = s.nnz;
    cli_upload(&s);
    bspgemm_context *ctx = s.ctx;
    bspgemm_matrix *At = s.A, *A = s.A;
    if (!symmetric) CHECK(bspgemm_matrix_transpose(ctx, At, &A), "bspgemm_matrix_transpose");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    uint64_t *fixed = malloc(((size_t)M + 1) * sizeof(uint64_t));
    double *rank = malloc(((size_t)M + 1) * sizeof(double));
    int *order = malloc(((size_t)M + 1) * sizeof(int));
    if (!fixed || !rank || !order) exit(1);
    const struct timespec t0 = cli_now();
    bspgemm_pr_info info;
    CHECK(bspgemm_pagerank(ctx, A, At, method, damping, (int)iterations, tolerance, fixed, rank, &info), "bspgemm_pagerank");
    const double ms = cli_ms(t0, cli_now());
    printf("%u,%u,%" PRId64 ",%d,%" PRIu64 ",%" PRIu64 ",%.3f\n", M, nnz, info.dangling, info.iterations, info.delta, info.mass,
           ms);
    for (uint32_t v = 0; v < M; v++) order[v] = (int)v;
    g_rank = fixed;
    qsort(order, M, sizeof(int), by_rank);
    for (uint32_t k = 0; k < M && k < (uint32_t)top; k++)
        printf("%d,%" PRIu64 ",%.17g\n", order[k], fixed[order[k]], rank[order[k]]);
    free(fixed); free(rank); free(order);
    if (!symmetric) bspgemm_matrix_free(A);
    cli_close(&s);
    return 0;
}
