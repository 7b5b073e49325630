/*
 * cli_common.h -- what the C command-line drivers (spgemm_hip_*.c) share: the CHECK macro, the two argument-scanning
 * helpers and the two whole-number parsers, the Matrix Market loader with the reference's failure behaviour, the square
 * check, the context of BSPGEMM_DEVICE, the session (load, upload, close) of the square-only drivers, wall-clock
 * milliseconds with the timed call, and the line writers.  static inline only; the drivers reach the GPU through the C ABI
 * alone.  What a driver accepts is part of its behaviour: a parsing rule that these helpers cannot express stays open at
 * its site, with a comment.
 */
#ifndef BSPGEMM_CLI_COMMON_H
#define BSPGEMM_CLI_COMMON_H

#include "../../include/bspgemm.h"

#include <errno.h>
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

/* argument scanning: every driver's loop is a chain of these two, and whatever neither takes goes to its usage() */
static inline int cli_flag(const char *arg, const char *name)
{
    return strcmp(arg, name) == 0;
}

/* is argv[*i] `name` with a value after it?  Then *value is that value and *i stands on it */
static inline int cli_value(int argc, char **argv, int *i, const char *name, const char **value)
{
    if (strcmp(argv[*i], name) != 0 || *i + 1 >= argc) return 0;
    *value = argv[++*i];
    return 1;
}

/* the whole of `text` as a number of `base` (0: C's prefixes) that is at most `most`; a leading '-' is refused (strtoull
 * would negate it), and so is a value past 2^64 - 1 (it saturates, with errno).  0 when refused: what follows is the site's */
static inline int cli_unsigned(const char *text, int base, unsigned long long most, unsigned long long *out)
{
    char *end;
    if (*text == '-') return 0;
    errno = 0;
    *out = strtoull(text, &end, base);
    return !(end == text || *end || errno || *out > most);
}

/* the same, signed, in [lo, hi] */
static inline int cli_signed(const char *text, int base, long long lo, long long hi, long long *out)
{
    char *end;
    errno = 0;
    *out = strtoll(text, &end, base);
    return !(errno || end == text || *end || *out < lo || *out > hi);
}

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

/* a square-only driver's operand: the loaded file, then the context and the file's matrix on the device */
typedef struct cli_session {
    uint32_t *Arow, *Acol, M, N, nnz;
    bspgemm_context *ctx;
    bspgemm_matrix *A;
} cli_session;

/* step 1, no GPU yet: load and refuse what is not square; `what` as in cli_need_square.  A driver refuses its own
 * arguments against the graph (a source that is no vertex) between the steps */
static inline cli_session cli_open(const char *path, unsigned flags, const char *what)
{
    cli_session s = {NULL, NULL, 0, 0, 0, NULL, NULL};
    cli_load(path, flags, &s.Arow, &s.Acol, &s.M, &s.N, &s.nnz);
    cli_need_square(what, s.M, s.N);
    return s;
}

/* step 2: the context, the upload, a synchronise */
static inline void cli_upload(cli_session *s)
{
    s->ctx = cli_context(0);
    CHECK(bspgemm_matrix_upload(s->ctx, (int)s->M, (int)s->M, (const int *)s->Arow, (const int *)s->Acol, &s->A), "upload");
    CHECK(bspgemm_synchronize(s->ctx), "synchronize");
}

/* after the driver has freed what it made itself */
static inline void cli_close(cli_session *s)
{
    bspgemm_matrix_free(s->A);
    bspgemm_destroy(s->ctx);
    free(s->Arow); free(s->Acol);
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

/* ms = the wall time of one library call and the synchronise after it */
#define CLI_TIMED(ms, ctx, call, what)                          \
    do {                                                        \
        const struct timespec t0_ = cli_now();                  \
        CHECK(call, what);                                      \
        CHECK(bspgemm_synchronize(ctx), "synchronize");         \
        (ms) = cli_ms(t0_, cli_now());                          \
    } while (0)

/* an output file of lines: cli_create, fprintf, cli_finish */
static inline FILE *cli_create(const char *path)
{
    FILE *f = fopen(path, "w");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
    return f;
}

static inline void cli_finish(FILE *f, const char *path)
{
    if (fclose(f)) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
}

/* x[0 .. n) one per line */
static inline void cli_write_ints(const char *path, const int *x, uint32_t n)
{
    FILE *f = cli_create(path);
    for (uint32_t v = 0; v < n; v++) fprintf(f, "%d\n", x[v]);
    cli_finish(f, path);
}

#endif
