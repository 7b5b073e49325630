/*
 * cli_common.h -- what the C command-line drivers (spgemm_hip_*.c) share: the CHECK macro, the Matrix Market loader with the
 * reference's failure behaviour, the square check, the context of BSPGEMM_DEVICE, wall-clock milliseconds and the
 * one-int-per-line writer.  static inline only; the drivers reach the GPU through the C ABI alone.
 */
#ifndef BSPGEMM_CLI_COMMON_H
#define BSPGEMM_CLI_COMMON_H

#include "../../include/bspgemm.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define CHECK(st, what)                                                                         \
    do {                                                                                        \
        bspgemm_status s_ = (st);                                                               \
        if (s_ != BSPGEMM_OK) {                                                                 \
            fprintf(stderr, "%s: %s: %s\n", what, bspgemm_status_string(s_), bspgemm_last_error()); \
            exit(1);                                                                            \
        }                                                                                       \
    } while (0)

/* readCOO (final/utils.c:47-81): the file transposed in memory, M rows of it.  The reference prints for a bad banner only
 * (utils.c:56-59); fopen and size-line failures exit(1) silently (:54-55, :60-61). */
static inline void cli_load(const char *path, unsigned flags, uint32_t **row, uint32_t **col, uint32_t *M, uint32_t *N,
                            uint32_t *nnz)
{
    const bspgemm_status st = bspgemm_readCOO_ex(path, flags, row, col, M, N, nnz);
    if (st == BSPGEMM_ERR_FORMAT) printf("Could not process Matrix Market banner.\n");
    if (st != BSPGEMM_OK) exit(1);
}

/* what: the driver's word for itself ("closure", "k-truss", ...) */
static inline void cli_need_square(const char *what, uint32_t M, uint32_t N)
{
    if (M != N) {
        fprintf(stderr, "%s needs a square matrix (%ux%u)\n", what, M, N);
        exit(1);
    }
}

/* the device BSPGEMM_DEVICE names, else `fallback` */
static inline int cli_device(int fallback)
{
    const char *devenv = getenv("BSPGEMM_DEVICE");
    return devenv ? atoi(devenv) : fallback;
}

static inline bspgemm_context *cli_context(int fallback_device)
{
    bspgemm_context *ctx;
    CHECK(bspgemm_create(cli_device(fallback_device), &ctx), "bspgemm_create");
    return ctx;
}

static inline struct timespec cli_now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t;
}

static inline double cli_ms(struct timespec t0, struct timespec t1)
{
    return (double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6;
}

/* x[0 .. n) one per line */
static inline void cli_write_ints(const char *path, const int *x, uint32_t n)
{
    FILE *f = fopen(path, "w");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
    for (uint32_t v = 0; v < n; v++) fprintf(f, "%d\n", x[v]);
    if (fclose(f)) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
}

#endif
