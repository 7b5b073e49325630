/*
 * spgemm_hip_bc.c -- betweenness centrality from a list of sources, exact in 64-bit integers, everything resident on the GPU
 * (include/bspgemm.h: bspgemm_betweenness).
 *
 *     SpGEMM_hip_bc  file.mtx  [--sources K [--seed S] | --all]  [--symmetrize]  [--top T]  [--out FILE]
 *
 * A file entry `i j` is the edge i -> j (1-based in the file).  The loader hands back the transpose of the file's matrix
 * (readCOO, final/utils.c:47-81), which is transposed once on the device, before the timer starts, for the out-edge operand
 * A.  --symmetrize: the graph is A | A^T instead (self-loops kept).  --all: every vertex is a source, in ascending order.
 * --sources K (default 8) --seed S (default 1): K sources from the generator x <- x * 6364136223846793005 +
 * 1442695040888963407 (mod 2^64) started at x = S, source = (x >> 33) mod n; a vertex drawn twice counts twice.
 * --top T: default 10.  --out FILE: every vertex's fixed value, one per line.
 * Prints  n,nnz,sources,reached,edges_forward,hub_chunks,depth_max,levels,sigma_max,canonicalised,ms  and then the T vertices
 * of the highest centrality, ties to the smaller id, as  vertex,fixed,double  (0-based ids; fixed: 2^32 = 1.0; double with
 * %.17g).  ms: wall time of bspgemm_betweenness, the operand already on the device.
 */
#include "cli_common.h"
#include <inttypes.h>

static const uint64_t *g_bc;

static int by_bc(const void *a, const void *b)
{
    const int x = *(const int *)a, y = *(const int *)b;
    if (g_bc[x] != g_bc[y]) return g_bc[x] > g_bc[y] ? -1 : 1;
    return x < y ? -1 : x > y;
}

static void usage(void)
{
    printf("usage: SpGEMM_hip_bc  path-to-matrix  [--sources K [--seed S] | --all]  [--symmetrize]  [--top T]  [--out FILE]\n");
    exit(1);
}

static long long whole(const char *text, long long lo, long long hi)
{
    long long x;
    if (!cli_signed(text, 10, lo, hi, &x)) usage();
    return x;
}

int main(int argc, char **argv)
{
    int all = 0, symmetrize = 0, counted = 0;
    long long k = 8, top = 10;
    uint64_t seed = 1;
    const char *out = NULL;
    if (argc < 2 || argv[1][0] == '-') usage();
    for (int i = 2; i < argc; i++) {
        const char *val;
        if (cli_flag(argv[i], "--all")) all = 1;
        else if (cli_flag(argv[i], "--symmetrize")) symmetrize = 1;
        else if (cli_value(argc, argv, &i, "--sources", &val)) { k = whole(val, 0, 1000000000); counted = 1; }
        else if (cli_value(argc, argv, &i, "--seed", &val)) seed = (uint64_t)whole(val, 0, 4000000000000000000ll);
        else if (cli_value(argc, argv, &i, "--top", &val)) top = whole(val, 0, 1000000000);
        else if (!cli_value(argc, argv, &i, "--out", &out)) usage();
    }
    if (all && counted) usage();
    cli_session s = cli_open(argv[1], 0, "betweenness");                  /* s.A: the loader's transpose */
    const uint32_t M = s.M;
    cli_upload(&s);
    bspgemm_context *ctx = s.ctx;
    bspgemm_matrix *A;
    if (symmetrize) CHECK(bspgemm_matrix_symmetrize(ctx, s.A, 0u, &A), "bspgemm_matrix_symmetrize");
    else CHECK(bspgemm_matrix_transpose(ctx, s.A, &A), "bspgemm_matrix_transpose");
    CHECK(bspgemm_synchronize(ctx), "synchronize");
    if (all) k = M;
    if (M == 0) k = 0;
    int *sources = malloc(((size_t)k + 1) * sizeof(int));
    uint64_t *fixed = malloc(((size_t)M + 1) * sizeof(uint64_t));
    double *bc = malloc(((size_t)M + 1) * sizeof(double));
    int *order = malloc(((size_t)M + 1) * sizeof(int));
    if (!sources || !fixed || !bc || !order) exit(1);
    uint64_t x = seed;
    for (long long i = 0; i < k; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        sources[i] = all ? (int)i : (int)((x >> 33) % M);
    }
    const struct timespec t0 = cli_now();
    bspgemm_bc_info info;
    CHECK(bspgemm_betweenness(ctx, A, (int)k, sources, fixed, bc, &info), "bspgemm_betweenness");
    const double ms = cli_ms(t0, cli_now());
    printf("%u,%lld,%d,%" PRId64 ",%" PRId64 ",%" PRId64 ",%d,%d,%" PRIu64 ",%d,%.3f\n", M, (long long)bspgemm_matrix_nnz(A),
           info.sources, info.reached, info.edges_forward, info.hub_chunks, info.depth_max, info.levels, info.sigma_max,
           info.canonicalised, ms);
    for (uint32_t v = 0; v < M; v++) order[v] = (int)v;
    g_bc = fixed;
    qsort(order, M, sizeof(int), by_bc);
    for (uint32_t i = 0; i < M && i < (uint32_t)top; i++)
        printf("%d,%" PRIu64 ",%.17g\n", order[i], fixed[order[i]], bc[order[i]]);
    if (out) {
        FILE *f = cli_create(out);
        for (uint32_t v = 0; v < M; v++) fprintf(f, "%" PRIu64 "\n", fixed[v]);
        cli_finish(f, out);
    }
    free(sources); free(fixed); free(bc); free(order);
    bspgemm_matrix_free(A);
    cli_close(&s);
    return 0;
}
