// prepass_gather.hip -- gate for the flat prepass: how fast is the blocked-table gather when each lane keeps K gathers
// in flight?  The bench matrix itself (R-MAT scale 22, edge factor 16, (0.30,0.25,0.25,0.20), seed 1, from the library's
// generator), its real A.col_idx and the real blocked table B.blk8 of B = A.  Flat over the nonzeros: a 256-thread
// workgroup owns 256*K of them, thread t takes base + t + 256k (A.col_idx read coalesced), issues all K table gathers,
// then decodes {start, length} (two v_sad_u8, clamped bytes looked up in B.row_ptr) and writes ab[] coalesced.  No row
// sums: this is the floor of the access, not a prepass.  K = 1, 4, 8, 16; median of 20 timed launches each.
// build: hipcc --offload-arch=gfx950 -O3 -I../../include -o prepass_gather prepass_gather.hip \
//            -L../../binary-spgemm_amd -lbspgemm -Wl,-rpath,'$ORIGIN/../../binary-spgemm_amd'
// run on the GPU box from tools/micro.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "bspgemm.h"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

typedef unsigned long long u64;
struct __attribute__((packed, aligned(4))) Int2U { int x, y; };
struct __attribute__((packed, aligned(4))) Blk8 { int base; unsigned lo, hi; };

template <int K>
__global__ __launch_bounds__(256) void k_gather(const int *__restrict__ Acol, long long nnz, const int *__restrict__ Brow,
                                                const int *__restrict__ Bblk, int2 *__restrict__ ab)
{
    const long long base = (long long)blockIdx.x * (256 * K);
    int j[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const long long p = base + threadIdx.x + 256 * k;
        j[k] = p < nnz ? Acol[p] : -1;
    }
    Blk8 w[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        w[k].base = 0; w[k].lo = w[k].hi = 0u;
        if (j[k] >= 0) w[k] = *reinterpret_cast<const Blk8 *>(Bblk + 3 * (j[k] >> 3));
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (j[k] < 0) continue;
        const int q = j[k] & 7;
        const u64 d = ((u64)w[k].hi << 32) | (u64)w[k].lo;
        const u64 below = d & ((1ull << (8 * q)) - 1ull);
        const u64 upto = (q == 7) ? d : (d & ((1ull << (8 * q + 8)) - 1ull));
        const u64 v = ~upto;
        int start = w[k].base + (int)__builtin_amdgcn_sad_u8((unsigned)below, 0u, 0u)
                    + (int)__builtin_amdgcn_sad_u8((unsigned)(below >> 32), 0u, 0u);
        int len = (int)((d >> (8 * q)) & 255ull);
        if (((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) != 0ull) {
            const Int2U pr = *reinterpret_cast<const Int2U *>(Brow + j[k]);
            start = pr.x;
            len = pr.y - pr.x;
        }
        ab[base + threadIdx.x + 256 * k] = make_int2(start, len);
    }
}

template <int K>
static float time_k(const int *Acol, long long nnz, const int *Brow, const int *Bblk, int2 *ab)
{
    const int grid = (int)((nnz + 256 * K - 1) / (256 * K));
    hipEvent_t a, b;
    CHK(hipEventCreate(&a));
    CHK(hipEventCreate(&b));
    for (int i = 0; i < 3; i++) hipLaunchKernelGGL(k_gather<K>, dim3(grid), dim3(256), 0, 0, Acol, nnz, Brow, Bblk, ab);
    std::vector<float> ms;
    for (int i = 0; i < 20; i++) {
        CHK(hipEventRecord(a));
        hipLaunchKernelGGL(k_gather<K>, dim3(grid), dim3(256), 0, 0, Acol, nnz, Brow, Bblk, ab);
        CHK(hipEventRecord(b));
        CHK(hipEventSynchronize(b));
        float t = 0.f;
        CHK(hipEventElapsedTime(&t, a, b));
        ms.push_back(t);
    }
    CHK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    printf("K=%2d  median %.3f ms  min %.3f ms  max %.3f ms\n", K, ms[ms.size() / 2], ms.front(), ms.back());
    return ms[ms.size() / 2];
}

int main()
{
    int *rp = nullptr, *ci = nullptr;
    if (bspgemm_gen_rmat(22, 16, 0.30, 0.25, 0.25, 1, &rp, &ci) != BSPGEMM_OK) { printf("generator failed\n"); return 1; }
    const int n = 1 << 22;
    const long long nnz = rp[n];
    // the blocked table as launch_blk8 builds it (no padded copy)
    const int nb = (n + 7) / 8;
    std::vector<int> blk(3 * (size_t)nb + 4, 0);
    for (int b = 0; b < nb; b++) {
        unsigned lo = 0u, hi = 0u;
        for (int k = 0; k < 8; k++) {
            const int r = 8 * b + k;
            const int d = r < n ? rp[r + 1] - rp[r] : 0;
            const unsigned byte = (unsigned)(d < 255 ? d : 255);
            if (k < 4) lo |= byte << (8 * k); else hi |= byte << (8 * (k - 4));
        }
        blk[3 * b] = rp[8 * b];
        blk[3 * b + 1] = (int)lo;
        blk[3 * b + 2] = (int)hi;
    }
    int *dA, *dR, *dB;
    int2 *dab;
    CHK(hipMalloc(&dA, nnz * sizeof(int)));
    CHK(hipMalloc(&dR, ((size_t)n + 2) * sizeof(int)));
    CHK(hipMalloc(&dB, blk.size() * sizeof(int)));
    CHK(hipMalloc(&dab, nnz * sizeof(int2)));
    CHK(hipMemcpy(dA, ci, nnz * sizeof(int), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dR, rp, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dB, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
    printf("R-MAT scale 22: n = %d, nnz(A) = %lld, table %.1f MB; compulsory bytes %.2f GB (A.col_idx + ab[])\n", n, nnz,
           blk.size() * 4.0 / 1e6, nnz * 12.0 / 1e9);
    time_k<1>(dA, nnz, dR, dB, dab);
    time_k<4>(dA, nnz, dR, dB, dab);
    time_k<8>(dA, nnz, dR, dB, dab);
    time_k<16>(dA, nnz, dR, dB, dab);
    // spot check of the K = 16 output against the host
    std::vector<int2> h(nnz);
    CHK(hipMemcpy(h.data(), dab, nnz * sizeof(int2), hipMemcpyDeviceToHost));
    long long bad = 0;
    for (long long p = 0; p < nnz; p += 997) {
        const int j = ci[p];
        if (h[p].x != rp[j] || h[p].y != rp[j + 1] - rp[j]) bad++;
    }
    printf("spot check: %lld mismatches\n", bad);
    free(rp);
    free(ci);
    return bad ? 1 : 0;
}
