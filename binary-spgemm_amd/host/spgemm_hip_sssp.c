/*
 * spgemm_hip_sssp.c -- single-source shortest paths with integer lengths, everything resident on the GPU (include/bspgemm.h:
 * bspgemm_weights_hashed, bspgemm_sssp), beside the search, matching and centrality drivers.
 *
 *     SpGEMM_hip_sssp  file.mtx  --source s  [--weights seed:wmin:wmax]  [--symmetric]  [--delta d]  [--lanes w]  [--out dist.txt]
 *
 * The transpose that the loader hands back (readCOO, final/utils.c:47-81) is used as it is: row u of it lists the
 * out-neighbours of u.  The loader is a pattern loader: the lengths are the hashed ones of bspgemm_weights_hashed, by default
 * seed 0 in [1, 255] (GAP's); --symmetric gives both directions of an edge the same length.  --delta 0 and --lanes 0 are
 * the library's defaults.
 * Prints one line  n,nnz,source,delta,reached,dist_max,rounds,buckets,entries_walked,improved,hub_chunks,ms  -- the fields
 * of bspgemm_sssp_info and the call's wall time, the operand and the weights already on the device.
 * --out writes one line "v dist parent" per reached vertex, v ascending (0-based).
 */
#include "cli_common.h"

static void usage(void)
{
    printf("usage: SpGEMM_hip_sssp  path-to-matrix  --source s  [--weights seed:wmin:wmax]  [--symmetric]  [--delta d]  "
           "[--lanes w]  [--out dist.txt]\n");
    exit(1);
}

static unsigned long long number(const char *text, unsigned long long most)
{
    unsigned long long v;
    if (!cli_unsigned(text, 0, most, &v)) usage();
    return v;
}

int main(int argc, char **argv)
{
    const char *out_path = NULL;
    unsigned seed = 0, flags = 0;
    uint32_t wmin = 1, wmax = 255;
    long long source = -1;
    bspgemm_sssp_params params = {0, 0, 0};
    if (argc < 2) usage();
    for (int i = 2; i < argc; i++) {
        const char *val;
        if (cli_flag(argv[i], "--symmetric")) {
            flags |= BSPGEMM_WEIGHTS_SYMMETRIC;
        } else if (cli_value(argc, argv, &i, "--source", &val)) {
            source = (long long)number(val, 0x7fffffffull);
        } else if (cli_value(argc, argv, &i, "--weights", &val)) {
            unsigned long long a, b, c;
            char tail;
            if (sscanf(val, "%llu:%llu:%llu%c", &a, &b, &c, &tail) != 3 || a > 0xffffffffull || b > 0xffffffffull ||
                c > 0xffffffffull || b > c)
                usage();
            seed = (unsigned)a;
            wmin = (uint32_t)b;
            wmax = (uint32_t)c;
        } else if (cli_value(argc, argv, &i, "--delta", &val)) {
            params.delta = number(val, ~0ull);
        } else if (cli_value(argc, argv, &i, "--lanes", &val)) {
            params.lanes = (int)number(val, 64);
            if (params.lanes != 0 && params.lanes != 4 && params.lanes != 16 && params.lanes != 64) usage();
        } else if (!cli_value(argc, argv, &i, "--out", &out_path)) {
            usage();
        }
    }
    if (source < 0) usage();
    cli_session s = cli_open(argv[1], 0, "shortest paths");
    const uint32_t M = s.M;
    if (source >= (long long)M) {
        fprintf(stderr, "source %lld is not a vertex of a graph of %u\n", source, M);
        exit(1);
    }
    cli_upload(&s);
    bspgemm_weights *W;
    CHECK(bspgemm_weights_hashed(s.ctx, s.A, seed, wmin, wmax, flags, &W), "bspgemm_weights_hashed");
    CHECK(bspgemm_synchronize(s.ctx), "synchronize");
    uint64_t *dist = malloc(((size_t)M + 1) * sizeof(uint64_t));
    int *parent = malloc(((size_t)M + 1) * sizeof(int));
    if (!dist || !parent) exit(1);
    bspgemm_sssp_info info;
    double ms;
    CLI_TIMED(ms, s.ctx, bspgemm_sssp(s.ctx, s.A, W, (int)source, &params, dist, out_path ? parent : NULL, &info), "bspgemm_sssp");
    if (out_path) {
        FILE *f = cli_create(out_path);
        for (uint32_t v = 0; v < M; v++)
            if (dist[v] != UINT64_MAX) fprintf(f, "%u %llu %d\n", v, (unsigned long long)dist[v], parent[v]);
        cli_finish(f, out_path);
    }
    printf("%u,%u,%lld,%llu,%lld,%llu,%d,%d,%lld,%lld,%lld,%.3f\n", M, s.nnz, source, (unsigned long long)info.delta,
           (long long)info.reached, (unsigned long long)info.dist_max, info.rounds, info.buckets, (long long)info.entries_walked,
           (long long)info.improved, (long long)info.hub_chunks, ms);
    free(dist); free(parent);
    bspgemm_weights_free(W);
    cli_close(&s);
    return 0;
}
