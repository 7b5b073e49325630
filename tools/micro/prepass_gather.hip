// prepass_gather.hip -- gate for the flat prepass: how fast is the blocked-table gather, per table LAYOUT and per number K
// of gathers each lane keeps in flight?  The bench matrix itself (R-MAT scale 22, edge factor 16, (0.30,0.25,0.25,0.20),
// seed 1, from the library's generator), its real A.col_idx and the extents table of B = A.  Flat over the nonzeros: a
// 256-thread workgroup owns 256*K of them, thread t takes base + t + 256k (A.col_idx read coalesced), issues all K table
// gathers, then decodes {start, length} (clamped lengths looked up in B.row_ptr) and writes ab[] coalesced.  No row sums:
// this is the floor of the access, not a prepass.  Median of 20 timed launches per line.
//
// Layouts (the switch: prepass_gather [b8|l16|l35|all], default all):
//   b8   12 B per  8 rows: {int32 start of the group's first row, 8 x 8-bit lengths}, clamp 255.  1.5 B/row, 6.3 MB.
//   l16  16 B per 16 rows: {int32 start, 3 words of 5 x 6-bit lengths (rows 5i+s at bit 6s of word i) whose two top bits
//        together hold the 16th length}, clamp 63.  1.0 B/row, 4.19 MB.  One aligned dwordx4 gather.
//   l35  32 B per 35 rows: {int32 start, 7 words of 5 x 6-bit lengths; the two top bits of the first six words together
//        hold the exact offset of row 20 from the start (4095: it does not fit, rows 20.. go to B.row_ptr)}, clamp 63.
//        0.914 B/row, 3.83 MB.  Two dwordx4 of one 32-byte piece.
// A group with a clamped length at or below the row is looked up in B.row_ptr itself.
// build: hipcc --offload-arch=gfx950 -O3 -I../../include -o prepass_gather prepass_gather.hip \
//            -L../../binary-spgemm_amd -lbspgemm -Wl,-rpath,'$ORIGIN/../../binary-spgemm_amd'
// run on the GPU box from tools/micro.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bspgemm.h"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

typedef unsigned long long u64;
struct __attribute__((packed, aligned(4))) Int2U { int x, y; };
struct __attribute__((packed, aligned(4))) Blk8 { int base; unsigned lo, hi; };

enum Layout { B8 = 0, L16 = 1, L35 = 2 };
static const char *const kLayoutName[] = {"b8 ", "l16", "l35"};

// ---- 6-bit fields, five to a word at bits 0, 6, .., 24 -------------------------------------------------------------
__device__ __forceinline__ int med3(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }
// the word's fields below bit `bits` (0, 6, .., 30)
__device__ __forceinline__ unsigned low_fields(unsigned w, int bits) { return w & ((1u << bits) - 1u); }
// a bit set in a field that is 63 (and maybe in fields above such a one): x holds fields only (two top bits clear)
__device__ __forceinline__ unsigned full_fields(unsigned x) { return (~x - 0x01041041u) & x & 0x20820820u; }
// sum of all fields of up to four such words: even fields in 12-bit lanes at 0, 12, 24 (4 * 63 = 252 fits the top
// lane's 8 bits), odd ones at 6, 18
__device__ __forceinline__ int sum_fields(unsigned x0, unsigned x1, unsigned x2, unsigned x3)
{
    const unsigned me = 0x3f03f03fu, mo = 0x00fc0fc0u;
    const unsigned e = (x0 & me) + (x1 & me) + (x2 & me) + (x3 & me);
    const unsigned o = (x0 & mo) + (x1 & mo) + (x2 & mo) + (x3 & mo);
    return (int)((e & 0xfffu) + ((e >> 12) & 0xfffu) + (e >> 24) + ((o >> 6) & 0xfffu) + (o >> 18));
}

// row k (0..15) of a 16-row entry {base, w0, w1, w2}
__device__ __forceinline__ void l16_extent(const int4 &g, int k, int &start, int &len, bool &sat)
{
    const unsigned w0 = (unsigned)g.y, w1 = (unsigned)g.z, w2 = (unsigned)g.w;
    const int t = 6 * k;
    const unsigned x0 = low_fields(w0, med3(t, 0, 30)), x1 = low_fields(w1, med3(t - 30, 0, 30)),
                   x2 = low_fields(w2, med3(t - 60, 0, 30));
    start = g.x + sum_fields(x0, x1, x2, 0u);
    const unsigned wk = k < 5 ? w0 : (k < 10 ? w1 : w2);
    const int sh = t - (k < 5 ? 0 : (k < 10 ? 30 : 60));
    const unsigned l15 = (w0 >> 30) | ((w1 >> 30) << 2) | ((w2 >> 30) << 4);
    len = k == 15 ? (int)l15 : (int)((wk >> sh) & 63u);
    sat = ((full_fields(x0) | full_fields(x1) | full_fields(x2)) != 0u) || len == 63;
}

// row k (0..34) of a 35-row entry {base, d1..d7}: rows 0..19 count from base over d1..d4, rows 20..34 from base + mid over
// d5..d7
__device__ __forceinline__ void l35_extent(const int4 &ga, const int4 &gb, int k, int &start, int &len, bool &sat)
{
    const unsigned d1 = (unsigned)ga.y, d2 = (unsigned)ga.z, d3 = (unsigned)ga.w, d4 = (unsigned)gb.x, d5 = (unsigned)gb.y,
                   d6 = (unsigned)gb.z, d7 = (unsigned)gb.w;
    const bool hi = k >= 20;
    const unsigned mid = (d1 >> 30) | ((d2 >> 30) << 2) | ((d3 >> 30) << 4) | ((d4 >> 30) << 6) | ((d5 >> 30) << 8) | ((d6 >> 30) << 10);
    const unsigned w0 = hi ? d5 : d1, w1 = hi ? d6 : d2, w2 = hi ? d7 : d3, w3 = hi ? 0u : d4;
    const int kk = hi ? k - 20 : k, t = 6 * kk;
    const unsigned x0 = low_fields(w0, med3(t, 0, 30)), x1 = low_fields(w1, med3(t - 30, 0, 30)),
                   x2 = low_fields(w2, med3(t - 60, 0, 30)), x3 = low_fields(w3, med3(t - 90, 0, 30));
    start = ga.x + (hi ? (int)mid : 0) + sum_fields(x0, x1, x2, x3);
    const unsigned wk = kk < 5 ? w0 : (kk < 10 ? w1 : (kk < 15 ? w2 : w3));
    const int sh = t - (kk < 5 ? 0 : (kk < 10 ? 30 : (kk < 15 ? 60 : 90)));
    len = (int)((wk >> sh) & 63u);
    sat = ((full_fields(x0) | full_fields(x1) | full_fields(x2) | full_fields(x3)) != 0u) || len == 63 || (hi && mid == 4095u);
}

template <int LAYOUT, int K>
__global__ __launch_bounds__(256) void k_gather(const int *__restrict__ Acol, long long nnz, const int *__restrict__ Brow,
                                                const int *__restrict__ Btab, int2 *__restrict__ ab)
{
    const long long base = (long long)blockIdx.x * (256 * K);
    int j[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const long long p = base + threadIdx.x + 256 * k;
        j[k] = p < nnz ? Acol[p] : -1;
    }
    int start[K], len[K];
    bool sat[K];
    if (LAYOUT == B8) {
        Blk8 w[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            w[k].base = 0; w[k].lo = w[k].hi = 0u;
            if (j[k] >= 0) w[k] = *reinterpret_cast<const Blk8 *>(Btab + 3 * (j[k] >> 3));
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int q = j[k] & 7;
            const u64 d = ((u64)w[k].hi << 32) | (u64)w[k].lo;
            const u64 below = d & ((1ull << (8 * q)) - 1ull);
            const u64 upto = (q == 7) ? d : (d & ((1ull << (8 * q + 8)) - 1ull));
            const u64 v = ~upto;
            start[k] = w[k].base + (int)__builtin_amdgcn_sad_u8((unsigned)below, 0u, 0u)
                       + (int)__builtin_amdgcn_sad_u8((unsigned)(below >> 32), 0u, 0u);
            len[k] = (int)((d >> (8 * q)) & 255ull);
            sat[k] = ((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) != 0ull;
        }
    } else if (LAYOUT == L16) {
        int4 g[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            g[k] = make_int4(0, 0, 0, 0);
            if (j[k] >= 0) g[k] = reinterpret_cast<const int4 *>(Btab)[j[k] >> 4];
        }
#pragma unroll
        for (int k = 0; k < K; k++) l16_extent(g[k], j[k] & 15, start[k], len[k], sat[k]);
    } else {
        int4 ga[K], gb[K];
        int q[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            ga[k] = gb[k] = make_int4(0, 0, 0, 0);
            q[k] = (int)((unsigned)(j[k] < 0 ? 0 : j[k]) / 35u);
            if (j[k] >= 0) {
                ga[k] = reinterpret_cast<const int4 *>(Btab)[2 * q[k]];
                gb[k] = reinterpret_cast<const int4 *>(Btab)[2 * q[k] + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) l35_extent(ga[k], gb[k], j[k] - 35 * q[k], start[k], len[k], sat[k]);
    }
    // clamped lengths: the exact pairs, issued together
    Int2U pr[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        pr[k].x = pr[k].y = 0;
        sat[k] = sat[k] && j[k] >= 0;
        if (sat[k]) pr[k] = *reinterpret_cast<const Int2U *>(Brow + j[k]);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (j[k] < 0) continue;
        if (sat[k]) { start[k] = pr[k].x; len[k] = pr[k].y - pr[k].x; }
        ab[base + threadIdx.x + 256 * k] = make_int2(start[k], len[k]);
    }
}

struct Line { float med, mn, mx; };

template <int LAYOUT, int K>
static Line time_k(const int *Acol, long long nnz, const int *Brow, const int *Btab, int2 *ab)
{
    const int grid = (int)((nnz + 256 * K - 1) / (256 * K));
    hipEvent_t a, b;
    CHK(hipEventCreate(&a));
    CHK(hipEventCreate(&b));
    for (int i = 0; i < 3; i++) hipLaunchKernelGGL((k_gather<LAYOUT, K>), dim3(grid), dim3(256), 0, 0, Acol, nnz, Brow, Btab, ab);
    std::vector<float> ms;
    for (int i = 0; i < 20; i++) {
        CHK(hipEventRecord(a));
        hipLaunchKernelGGL((k_gather<LAYOUT, K>), dim3(grid), dim3(256), 0, 0, Acol, nnz, Brow, Btab, ab);
        CHK(hipEventRecord(b));
        CHK(hipEventSynchronize(b));
        float t = 0.f;
        CHK(hipEventElapsedTime(&t, a, b));
        ms.push_back(t);
    }
    CHK(hipGetLastError());
    CHK(hipEventDestroy(a));
    CHK(hipEventDestroy(b));
    std::sort(ms.begin(), ms.end());
    printf("%s K=%2d  median %.3f ms  min %.3f ms  max %.3f ms\n", kLayoutName[LAYOUT], K, ms[ms.size() / 2], ms.front(), ms.back());
    fflush(stdout);
    return Line{ms[ms.size() / 2], ms.front(), ms.back()};
}

// ---- the tables, built on the host as the library's builder kernel does (no padded copy) ---------------------------
static std::vector<int> build_b8(const int *rp, int n)
{
    const int nb = (n + 7) / 8;
    std::vector<int> t(3 * (size_t)nb + 4, 0);
    for (int b = 0; b < nb; b++) {
        unsigned lo = 0u, hi = 0u;
        for (int k = 0; k < 8; k++) {
            const int r = 8 * b + k;
            const int d = r < n ? rp[r + 1] - rp[r] : 0;
            const unsigned byte = (unsigned)(d < 255 ? d : 255);
            if (k < 4) lo |= byte << (8 * k); else hi |= byte << (8 * (k - 4));
        }
        t[3 * b] = rp[8 * b];
        t[3 * b + 1] = (int)lo;
        t[3 * b + 2] = (int)hi;
    }
    return t;
}
static unsigned len6(const int *rp, int n, int r) { const int d = r < n ? rp[r + 1] - rp[r] : 0; return (unsigned)(d < 63 ? d : 63); }
static std::vector<int> build_l16(const int *rp, int n)
{
    const int ng = (n + 15) / 16;
    std::vector<int> t(4 * (size_t)ng + 4, 0);
    for (int g = 0; g < ng; g++) {
        unsigned w[3] = {0u, 0u, 0u};
        for (int k = 0; k < 15; k++) w[k / 5] |= len6(rp, n, 16 * g + k) << (6 * (k % 5));
        const unsigned l15 = len6(rp, n, 16 * g + 15);
        for (int i = 0; i < 3; i++) w[i] |= ((l15 >> (2 * i)) & 3u) << 30;
        t[4 * (size_t)g] = rp[16 * g];
        for (int i = 0; i < 3; i++) t[4 * (size_t)g + 1 + i] = (int)w[i];
    }
    return t;
}
static std::vector<int> build_l35(const int *rp, int n)
{
    const int ng = (n + 34) / 35;
    std::vector<int> t(8 * (size_t)ng + 8, 0);
    for (int g = 0; g < ng; g++) {
        unsigned w[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (int k = 0; k < 35; k++) w[k / 5] |= len6(rp, n, 35 * g + k) << (6 * (k % 5));
        const int r20 = 35 * g + 20 < n ? 35 * g + 20 : n;
        const unsigned mid = (unsigned)std::min(rp[r20] - rp[35 * g], 4095);   // exact, so a clamped row below row 20 ends there
        for (int i = 0; i < 6; i++) w[i] |= ((mid >> (2 * i)) & 3u) << 30;
        t[8 * (size_t)g] = rp[35 * g];
        for (int i = 0; i < 7; i++) t[8 * (size_t)g + 1 + i] = (int)w[i];
    }
    return t;
}

// share of rows of `clamp` or more entries, and of look-ups that land in a group of `group` rows with such a row at or
// below the looked-up one (those go to B.row_ptr)
// (mid_row > 0: the group counts anew from that row, where it holds an exact offset below 4095)
static void clamp_shares(const int *rp, const int *ci, int n, long long nnz, int group, int clamp, int mid_row, const char *name)
{
    std::vector<unsigned char> esc((size_t)n, 0);
    long long rows = 0, rows_nnz = 0;
    for (int g0 = 0; g0 < n; g0 += group) {
        bool seen = false;
        for (int r = g0; r < n && r < g0 + group; r++) {
            const int d = rp[r + 1] - rp[r];
            if (mid_row > 0 && r == g0 + mid_row) seen = rp[r] - rp[g0] >= 4095;
            if (d >= clamp) { seen = true; rows++; rows_nnz += d; }
            esc[r] = seen ? 1 : 0;
        }
    }
    long long look = 0;
    for (long long p = 0; p < nnz; p++) look += esc[ci[p]];
    printf("%s rows of %d+ entries: %.3f %% of the rows, %.2f %% of the nonzeros; look-ups that go to B.row_ptr: %.2f %%\n", name,
           clamp, 100.0 * rows / n, 100.0 * rows_nnz / nnz, 100.0 * look / nnz);
}

static long long spot_check(const int *rp, const int *ci, long long nnz, const int2 *dab, const char *name)
{
    std::vector<int2> h(nnz);
    CHK(hipMemcpy(h.data(), dab, nnz * sizeof(int2), hipMemcpyDeviceToHost));
    long long bad = 0;
    for (long long p = 0; p < nnz; p += 97) {
        const int j = ci[p];
        if (h[p].x != rp[j] || h[p].y != rp[j + 1] - rp[j]) bad++;
    }
    printf("%s spot check against B.row_ptr: %lld mismatches\n", name, bad);
    return bad;
}

static int *to_device(const std::vector<int> &t)
{
    int *d = nullptr;
    CHK(hipMalloc(&d, t.size() * sizeof(int)));
    CHK(hipMemcpy(d, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
    return d;
}

int main(int argc, char **argv)
{
    const char *which = argc > 1 ? argv[1] : "all";
    const bool all = !strcmp(which, "all");
    const bool do_b8 = all || !strcmp(which, "b8"), do_l16 = all || !strcmp(which, "l16"), do_l35 = all || !strcmp(which, "l35");
    if (!do_b8 && !do_l16 && !do_l35) { printf("usage: prepass_gather [b8|l16|l35|all]\n"); return 2; }
    int *rp = nullptr, *ci = nullptr;
    if (bspgemm_gen_rmat(22, 16, 0.30, 0.25, 0.25, 1, &rp, &ci) != BSPGEMM_OK) { printf("generator failed\n"); return 1; }
    const int n = 1 << 22;
    const long long nnz = rp[n];
    int *dA, *dR;
    int2 *dab;
    CHK(hipMalloc(&dA, nnz * sizeof(int)));
    CHK(hipMalloc(&dR, ((size_t)n + 2) * sizeof(int)));
    CHK(hipMalloc(&dab, nnz * sizeof(int2)));
    CHK(hipMemcpy(dA, ci, nnz * sizeof(int), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dR, rp, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    printf("R-MAT scale 22: n = %d, nnz(A) = %lld; compulsory bytes %.2f GB (A.col_idx + ab[])\n", n, nnz, nnz * 12.0 / 1e9);
    long long bad = 0;
    float b8_best = 0.f, b8_spread = 0.f;
    if (do_b8) {
        const std::vector<int> t = build_b8(rp, n);
        int *dT = to_device(t);
        printf("b8  table %.2f MB\n", t.size() * 4.0 / 1e6);
        clamp_shares(rp, ci, n, nnz, 8, 255, 0, "b8 ");
        const Line l[4] = {time_k<B8, 1>(dA, nnz, dR, dT, dab), time_k<B8, 4>(dA, nnz, dR, dT, dab), time_k<B8, 8>(dA, nnz, dR, dT, dab),
                           time_k<B8, 16>(dA, nnz, dR, dT, dab)};
        float mn = l[0].mn, mx = l[0].mx;
        b8_best = l[0].med;
        for (const Line &x : l) { mn = std::min(mn, x.mn); mx = std::max(mx, x.mx); b8_best = std::min(b8_best, x.med); }
        b8_spread = mx - mn;
        printf("b8  lowest median %.3f ms, spread (max - min over its lines) %.3f ms\n", b8_best, b8_spread);
        bad += spot_check(rp, ci, nnz, dab, "b8 ");
        CHK(hipFree(dT));
    }
    if (do_l16) {
        const std::vector<int> t = build_l16(rp, n);
        int *dT = to_device(t);
        printf("l16 table %.2f MB\n", t.size() * 4.0 / 1e6);
        clamp_shares(rp, ci, n, nnz, 16, 63, 0, "l16");
        const Line l[3] = {time_k<L16, 4>(dA, nnz, dR, dT, dab), time_k<L16, 8>(dA, nnz, dR, dT, dab), time_k<L16, 16>(dA, nnz, dR, dT, dab)};
        const float best = std::min(l[0].med, std::min(l[1].med, l[2].med));
        if (do_b8) printf("l16 lowest median %.3f ms: %.3f ms below b8, %.1f x its spread\n", best, b8_best - best, (b8_best - best) / b8_spread);
        bad += spot_check(rp, ci, nnz, dab, "l16");
        CHK(hipFree(dT));
    }
    if (do_l35) {
        const std::vector<int> t = build_l35(rp, n);
        int *dT = to_device(t);
        printf("l35 table %.2f MB\n", t.size() * 4.0 / 1e6);
        clamp_shares(rp, ci, n, nnz, 35, 63, 20, "l35");
        const Line l[3] = {time_k<L35, 4>(dA, nnz, dR, dT, dab), time_k<L35, 8>(dA, nnz, dR, dT, dab), time_k<L35, 16>(dA, nnz, dR, dT, dab)};
        const float best = std::min(l[0].med, std::min(l[1].med, l[2].med));
        if (do_b8) printf("l35 lowest median %.3f ms: %.3f ms below b8, %.1f x its spread\n", best, b8_best - best, (b8_best - best) / b8_spread);
        bad += spot_check(rp, ci, nnz, dab, "l35");
        CHK(hipFree(dT));
    }
    free(rp);
    free(ci);
    return bad ? 1 : 0;
}
