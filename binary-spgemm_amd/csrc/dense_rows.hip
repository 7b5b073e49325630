// dense_rows.hip -- heavy rows (F_i > 2048 products), one workgroup per A-row, three kernels over ONE gather (heavy_gather.hpp):
//
//   k_dense_rows        a dense column bitmap in LDS, swept over column windows: the literal GPU form of the reference's accumulator
//                       (final/SpGEMM_mpi_omp.c:21,38-42) -- xb[k] becomes bit k of the LDS bitmap, test-and-set becomes ds_or_b32, and
//                       the quickSort of the row (:47) disappears because the bitmap is read out in column order.  Two shapes: 1024
//                       threads over windows of up to 2^20 columns (128 KiB), 512 threads over 2^18 (32 KiB).  When the columns exceed the
//                       window the row's products are gathered once per window.  The mask mode is a template parameter;
//   k_dense_rows_count  the counting masked product: a window of mask-column ranks and counters;
//   k_rank_rows         rows of at most 6144 products where the small shape would need two to four windows: a two-level rank
//                       bitmap sized by the ROW -- two sweeps and one read-out whatever the column count (see the kernel).
//                       (It shares this file with the window kernels because they compile differently without it: DESIGN.md 4.5.)
#include "heavy_gather.hpp"
#include <atomic>
#include <stdlib.h>

namespace bsp {

// Two shapes of the same kernel (class kDenseBin / kMidBin, kernels.hpp):
//   1024 threads, window up to 2^20 columns (128 KiB): one workgroup per CU -- worth it for hub rows,
//        whose tens of thousands of products amortise the latency of every phase;
//    512 threads, window up to 2^18 columns (32 KiB): four workgroups (32 waves) per CU -- for the many
//        rows with thousands of products, which one workgroup per CU serialises phase by phase
//        (256 threads: the same four rows in flight with half the waves to cover their latencies).
constexpr int kDenseThreadsBig = 1024;
constexpr int kDenseThreadsMid = 512;
constexpr int kMidMinWaves = 8;              // four 8-wave workgroups per CU: 64 VGPRs
constexpr int kBigMinWaves = 4;
constexpr int kDenseMaxWords = 16384;        // 64-bit words per window = 2^20 columns = 128 KiB
constexpr int kMidMaxWords = 4096;           // 4096 words = 2^18 columns = 32 KiB
constexpr int kDenseWordBits = 12;           // 64-column words with at least this many outputs are emitted by a whole wave
constexpr int kDenseQuadsPerThreadBig = 16;  // quads (16-byte pieces of a B row) per thread and tile: 64 / 32 products
constexpr int kDenseQuadsPerThreadMid = 8;   //   (the small shape's four workgroups share the CU's LDS: a smaller plan)
constexpr int kDenseInFlightBig = 8;         // 16-byte B.col_idx loads a thread keeps in flight
constexpr int kDenseInFlightMid = 4;         //   (64 VGPRs)

// One kernel, the mask mode a template constant (what F's row -- Frow / Fcol, absolute row ids; unused by None -- does):
//   None    the plain product.
//   Keep    C = F .* (A*B) (SpGEMM_masked, final/SpGEMM_mpi_omp.c:232-288).  The reference presets its flag array so that only
//           columns of F's row can be appended (:253-255); here the window holds two bitmaps, P (products) and K (kept): after
//           the gather every column of F's row that is set in P is set in K, and K is what gets read out.
//   Drop    C = !F .* (A*B).  One bitmap: after the gather of a window that received any product, every column of F's row
//           that lies in the window is cleared from it, then the window is read out as usual.
//   Insert  C = D | (A*B) (Frow / Fcol: D's CSR).  One bitmap: the columns of D's row that lie in [0, cols) are set in each
//           window after its gather.
// Every instance compiles to the instructions of the separate kernel it replaced (tools/isa_diff.py).
template <MaskMode MODE, int kDenseThreads>
__global__ __launch_bounds__(kDenseThreads, (kDenseThreads == kDenseThreadsBig ? kBigMinWaves : kMidMinWaves)) void k_dense_rows(const int2 *__restrict__ ab,
                                                              const int *__restrict__ Bcol, int nnzB,
                                                              int cols, int wwords,
                                                              const RowRec *__restrict__ rec,
                                                              const long long *__restrict__ recpre,
                                                              int row_begin,
                                                              int *__restrict__ tmp,
                                                              int *__restrict__ cnt,
                                                              const int *__restrict__ Frow,
                                                              const int *__restrict__ Fcol)
{
    constexpr bool MASKED = MODE == MaskMode::Keep;                    // two bitmaps
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    u64 *bmP = reinterpret_cast<u64 *>(lds_raw);                       // products
    u32 *bm32 = reinterpret_cast<u32 *>(lds_raw);
    u64 *bm = MASKED ? bmP + wwords : bmP;                             // what is read out (K or P)
    u32 *bmK32 = reinterpret_cast<u32 *>(bm);
    constexpr int kWaves = kDenseThreads / 64;
    constexpr int kQPT = kDenseThreads == kDenseThreadsBig ? kDenseQuadsPerThreadBig : kDenseQuadsPerThreadMid;
    constexpr int kInFlight = kDenseThreads == kDenseThreadsBig ? kDenseInFlightBig : kDenseInFlightMid;   // 16-byte loads a thread keeps in flight
    __shared__ GatherLds<kDenseThreads, kQPT> G;
    __shared__ int wtot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < (MASKED ? 2 * wwords : wwords); t += kDenseThreads) bmP[t] = 0ull;
    gather_init(G);
    __syncthreads();

    const RowRec q = rec[blockIdx.x];
    const int i = q.row;
    const int a0 = q.a0, a1 = q.a0 + q.alen;
    int *out = tmp + recpre[blockIdx.x];
    const long long W = (long long)wwords * 64;
    const int nwin = (int)(((long long)cols + W - 1) / W);
    int total = 0;

    GatherState g;
    for (int win = 0; win < nwin; win++) {
        const long long lo = (long long)win * W;
        const int lo32 = (int)lo;
        bool any = false;                                          // Drop: this thread inserted a product into the window
        gather_sweep<kDenseThreads, kQPT, kInFlight>(G, g, ab, Bcol, nnzB, a0, a1, win == 0, [&](const Int4U &v, u32 vm, int) {
            const u32 c0 = (u32)(v.x - lo32), c1 = (u32)(v.y - lo32), c2 = (u32)(v.z - lo32), c3 = (u32)(v.w - lo32);
            const bool i0 = (vm & 1u) && c0 < (u32)W, i1 = (vm & 2u) && c1 < (u32)W;   // (columns below the window wrap to huge values)
            const bool i2 = (vm & 4u) && c2 < (u32)W, i3 = (vm & 8u) && c3 < (u32)W;
            if constexpr (MODE == MaskMode::Drop) any |= i0 | i1 | i2 | i3;
            insert_quad(bm32, i0, i1, i2, i3,
                        c0 >> 5, c1 >> 5, c2 >> 5, c3 >> 5, 1u << (c0 & 31), 1u << (c1 & 31), 1u << (c2 & 31), 1u << (c3 & 31), nwin > 1);
        });
        if constexpr (MODE == MaskMode::Insert) {
            // set the window's columns of D's row (read coalesced, a workgroup's width at a time) -- in EVERY window: one that
            // received no product is read out all the same, so D's columns there are not lost
            const int d0 = Frow[i], d1 = Frow[i + 1];
            for (int k = d0 + tid; k < d1; k += kDenseThreads) {
                const u32 c = (u32)Fcol[k], cl = c - (u32)lo32;
                if (c < (u32)cols && cl < (u32)W) atomicOr(&bm32[cl >> 5], 1u << (cl & 31));
            }
            __syncthreads();
        }
        if constexpr (MODE == MaskMode::Drop) {
            // clear the window's columns of F's row (read coalesced, a workgroup's width at a time); a window that
            // received no product has nothing to clear and is not walked
            if (__syncthreads_or(any)) {
                const int f0 = Frow[i], f1 = Frow[i + 1];
                for (int k = f0 + tid; k < f1; k += kDenseThreads) {
                    const long long c = (long long)Fcol[k] - lo;
                    if (c >= 0 && c < W) atomicAnd(&bm32[c >> 5], ~(1u << (c & 31)));
                }
                __syncthreads();
            }
        }
        if (MASKED) {
            // keep the product bits that F's row admits, then wipe P for the next window / row
            const int f0 = Frow[i], f1 = Frow[i + 1];
            for (int k = f0 + tid; k < f1; k += kDenseThreads) {
                const long long c = (long long)Fcol[k] - lo;
                if (c >= 0 && c < W && ((bm32[c >> 5] >> (c & 31)) & 1u)) atomicOr(&bmK32[c >> 5], 1u << (c & 31));
            }
            __syncthreads();
            for (int t = tid; t < wwords; t += kDenseThreads) bmP[t] = 0ull;
            __syncthreads();
        }
        // read-out in column order: wave w owns the words [w*wpw, (w+1)*wpw); a step takes 64*kWpl
        // consecutive words, lane l the kWpl words behind 64-bit word kWpl*l of the step -- a lane's
        // outputs are one contiguous piece of the row, the step's pieces follow each other.  kWpl = 4:
        // ONE wave scan per 256 words (it was one per 64: in a window that is mostly empty -- a row with a
        // few thousand products over 2^18 columns -- the scans were two thirds of the kernel's VALU work).
        constexpr int kWpl = 4;
        constexpr int kStepWords = 64 * kWpl;
        constexpr int kWavesPerWg = kDenseThreads / 64;
        const int wpw = ((wwords + kWavesPerWg - 1) / kWavesPerWg + kStepWords - 1) / kStepWords * kStepWords;
        const int wbeg = wave * wpw;
        const int wend = (wbeg + wpw < wwords) ? wbeg + wpw : wwords;
        int c = 0;
        for (int w = wbeg + lane; w < wend; w += 64) c += __popcll(bm[w]);
        const int inc = wave_incl_scan(c);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int off = 0, btotal = 0;
        for (int k = 0; k < kDenseThreads / 64; k++) {
            const int t = wtot[k];
            if (k < wave) off += t;
            btotal += t;
        }
        int run = total + off;                                 // wave-uniform output cursor
        for (int w0 = wbeg; w0 < wend; w0 += kStepWords) {
            const int wl = w0 + kWpl * lane;                   // this lane's first word
            u64 m[kWpl];
            int cw = 0;
#pragma unroll
            for (int k = 0; k < kWpl; k++) {
                m[k] = 0ull;
                if (wl + k < wend) { m[k] = bm[wl + k]; bm[wl + k] = 0ull; }
                cw += __popcll(m[k]);
            }
            const int iw = wave_incl_scan(cw);
            const int step_total = wave_bcast(iw, 63);
            if (step_total == 0) continue;                     // uniform: an empty stretch of the window
            const int base = (int)(lo + (long long)wl * 64);
            // A step of few outputs is STAGED: the lanes expand their words into the step's own 2 KiB of the window (read and
            // cleared just above, by this wave) and the wave streams the piece out coalesced.  Written straight from the
            // per-lane loop, every store instruction of such a step touches up to 64 different 64-byte sectors -- those
            // stores were 25-30 % of the small shape's time (profiles/r04_heavy_ablation.log, part 6).
            const int stage_cap = 2 * ((wend - w0 < kStepWords) ? wend - w0 : kStepWords);    // 32-bit entries
            if (step_total <= stage_cap) {                     // (uniform)
                u32 *stage = reinterpret_cast<u32 *>(bm + w0);
                int p = iw - cw;
#pragma unroll
                for (int k = 0; k < kWpl; k++) {
                    u64 mk = m[k];
                    while (mk) {
                        stage[p++] = (u32)((base + 64 * k) | (int)__builtin_ctzll(mk));
                        mk &= mk - 1ull;
                    }
                }
                wave_lds_fence();
                for (int j = lane; j < step_total; j += 64) {
                    const u32 v = stage[j];
                    stage[j] = 0u;                             // the window is all zero again
                    out[run + j] = (int)v;
                }
                wave_lds_fence();
                run += step_total;
                continue;
            }
            int pos = run + iw - cw;
#pragma unroll
            for (int k = 0; k < kWpl; k++) {
                const int ck = __popcll(m[k]);
                // dense words (hub columns: up to 64 bits set) are written by the whole wave, one word
                // per store instruction, lane b holding bit b; the per-lane loop below then never runs
                // longer than kDenseWordBits trips while the other lanes idle
                u64 crowded = __ballot(ck >= kDenseWordBits);
                while (crowded) {
                    const int src = (int)__builtin_ctzll(crowded);
                    crowded &= crowded - 1ull;
                    const u64 mw = wave_bcast64(m[k], src);
                    const int pw = wave_bcast(pos, src);
                    const int bw = wave_bcast(base, src) + 64 * k;
                    if ((mw >> lane) & 1ull) out[pw + __popcll(mw & mask_lt(lane))] = bw | lane;
                }
                u64 mk = (ck >= kDenseWordBits) ? 0ull : m[k];
                int p = pos;
                while (mk) {                                   // two outputs per store instruction (8 bytes, only dword aligned)
                    const int v0 = (base + 64 * k) | (int)__builtin_ctzll(mk);
                    mk &= mk - 1ull;
                    if (mk) {
                        Int2U v2;
                        v2.x = v0;
                        v2.y = (base + 64 * k) | (int)__builtin_ctzll(mk);
                        mk &= mk - 1ull;
                        *reinterpret_cast<Int2U *>(out + p) = v2;
                        p += 2;
                    } else {
                        out[p++] = v0;
                    }
                }
                pos += ck;
            }
            run += step_total;
        }
        total += btotal;
        __syncthreads();
    }
    if (tid == 0) cnt[i - row_begin] = total;
}

// ---------------------------------------------------------------------------------------
// COUNTING (MaskMode::Count): C = F .* (A*B) with the number of products of every entry (PLUS_PAIR under the mask) for the
// rows the one-wave kernel does not take.  A window of P/K bitmaps cannot hold counts: a u32 per window column would shrink the
// window sixteen-fold.  Instead a window holds
//   K     the bitmap of F's columns in the window (set from F's row, coalesced),
//   pre   the exclusive popcount prefix of K's 32-bit words: a mask column's RANK in the window,
//   cnt   one u32 counter per DISTINCT mask column of the window, indexed by rank,
// and the gather adds one to the counter of every product whose K bit is set.  The read-out walks K in column order and
// emits the columns with a non-zero count, plus their counts.  A window never holds more distinct mask columns than there
// are counters (kCountSlots): it starts kCountMaxCols wide (2^18 columns), and when F's row puts more distinct columns into
// it, it is narrowed (at least halved, to about kCountSlots / density of the columns seen, a multiple of 32 columns) and K is
// set again -- a window of kCountSlots columns or fewer always fits.  The next window keeps the width while the density holds
// (more than kCountSlots / 2 distinct columns), else it starts twice as wide, up to kCountMaxCols.  Every window but the last
// (clamped to the last column) is a multiple of 32 columns wide, so windows start on whole K words.  Windows without a mask
// column are skipped without a product sweep.  LDS: K 32 KiB + pre 16 KiB + counters 80 KiB = the
// 128 KiB that the window kernels set.
constexpr int kCountMaxCols = 1 << 18;                 // columns of the widest window
constexpr int kCountWords = kCountMaxCols / 32;        // 32-bit words of K (and entries of pre)
constexpr int kCountSlots = 20480;                     // counters: 128 KiB - K - pre
static_assert(kCountWords * 4 + kCountWords * 2 + kCountSlots * 4 <= kDenseMaxWords * 8, "the window kernels' 128 KiB");
static_assert(kCountSlots < 65536, "ranks fit pre's 16 bits");

template <int kDenseThreads>
__global__ __launch_bounds__(kDenseThreads, kBigMinWaves) void k_dense_rows_count(const int2 *__restrict__ ab,
                                                              const int *__restrict__ Bcol, int nnzB, int cols,
                                                              const RowRec *__restrict__ rec,
                                                              const long long *__restrict__ recpre,
                                                              int row_begin,
                                                              int *__restrict__ tmp,
                                                              int *__restrict__ cnt,
                                                              const int *__restrict__ Frow,
                                                              const int *__restrict__ Fcol,
                                                              int *__restrict__ vals)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    u32 *K = reinterpret_cast<u32 *>(lds_raw);
    unsigned short *pre = reinterpret_cast<unsigned short *>(K + kCountWords);
    u32 *ctr = reinterpret_cast<u32 *>(pre + kCountWords);
    constexpr int kWaves = kDenseThreads / 64;
    constexpr int kQPT = kDenseQuadsPerThreadBig, kInFlight = kDenseInFlightBig;
    constexpr int kWPT = kCountWords / kDenseThreads;      // words of K per thread, blocked (at the widest window)
    static_assert(kCountWords % kDenseThreads == 0, "whole words per thread");
    __shared__ GatherLds<kDenseThreads, kQPT> G;
    __shared__ int wtot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < kCountWords; t += kDenseThreads) K[t] = 0u;
    gather_init(G);
    __syncthreads();

    const RowRec q = rec[blockIdx.x];
    const int i = q.row;
    const int a0 = q.a0, a1 = q.a0 + q.alen;
    int *out = tmp + recpre[blockIdx.x];
    int *vout = vals + recpre[blockIdx.x];
    const int f0 = Frow[i], f1 = Frow[i + 1];
    // the sum over the workgroup of every thread's x, and each thread's exclusive prefix (all threads, uniform flow)
    auto block_scan = [&](int x, int &excl) {
        const int inc = wave_incl_scan(x);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int off = 0, tot = 0;
        for (int k = 0; k < kWaves; k++) {
            const int t = wtot[k];
            if (k < wave) off += t;
            tot += t;
        }
        excl = off + inc - x;
        __syncthreads();                                           // (wtot is reused by the next scan)
        return tot;
    };

    int total = 0;
    bool swept = false;
    GatherState g;
    long long W = kCountMaxCols;
    for (long long lo = 0; lo < cols;) {
        if (W > (long long)cols - lo) W = (long long)cols - lo;   // (the last window ends at the last column)
        const u32 Wu = (u32)W;
        const u32 lo32 = (u32)lo;
        // ---- K: F's columns in [lo, lo + W) ----
        bool any = false;
        for (int k = f0 + tid; k < f1; k += kDenseThreads) {
            const u32 c = (u32)Fcol[k] - lo32;
            if ((u32)Fcol[k] < (u32)cols && c < Wu) {
                atomicOr(&K[c >> 5], 1u << (c & 31));
                any = true;
            }
        }
        if (!__syncthreads_or(any)) {                              // no mask column: nothing to count, K is still zero
            lo += W;
            W = W * 2 < kCountMaxCols ? W * 2 : kCountMaxCols;
            continue;
        }
        // ---- pre: ranks of the window's distinct mask columns ----
        u32 kw[kWPT];
        int run = 0;
#pragma unroll
        for (int k = 0; k < kWPT; k++) {
            kw[k] = K[tid * kWPT + k];                             // (zero beyond the window)
            run += __popc(kw[k]);
        }
        int excl = 0;
        const int ndist = block_scan(run, excl);
        if (ndist > kCountSlots) {
            // too dense for the counters: clear K and narrow the window to about kCountSlots columns' worth of mask
            // entries at this density (at least halved; a window of kCountSlots columns or fewer always fits)
#pragma unroll
            for (int k = 0; k < kWPT; k++) K[tid * kWPT + k] = 0u;
            long long Wn = W >> 1;
            while (Wn > kCountSlots && Wn * ndist > (long long)kCountSlots * W) Wn >>= 1;
            W = Wn & ~31ll;                                        // (> kCountSlots / 2: never zero)
            __syncthreads();
            continue;
        }
        {
            int p = excl;
#pragma unroll
            for (int k = 0; k < kWPT; k++) {
                pre[tid * kWPT + k] = (unsigned short)p;
                p += __popc(kw[k]);
            }
        }
        for (int t = tid; t < ndist; t += kDenseThreads) ctr[t] = 0u;
        __syncthreads();
        // ---- the product sweep: a product on a mask column adds one to the column's counter ----
        gather_sweep<kDenseThreads, kQPT, kInFlight>(G, g, ab, Bcol, nnzB, a0, a1, !swept, [&](const Int4U &v, u32 vm, int) {
            const u32 c0 = (u32)v.x - lo32, c1 = (u32)v.y - lo32, c2 = (u32)v.z - lo32, c3 = (u32)v.w - lo32;
            const bool i0 = (vm & 1u) && c0 < Wu, i1 = (vm & 2u) && c1 < Wu;   // (columns below the window wrap to huge values)
            const bool i2 = (vm & 4u) && c2 < Wu, i3 = (vm & 8u) && c3 < Wu;
            if (!__ballot(i0 | i1 | i2 | i3)) return;              // (wave-uniform) nothing of these 64 quads falls into the window
            auto one = [&](bool in, u32 c) {
                if (!in) return;
                const u32 x = K[c >> 5], b = c & 31;
                if ((x >> b) & 1u) atomicAdd(&ctr[pre[c >> 5] + __popc(x & ((1u << b) - 1u))], 1u);
            };
            one(i0, c0);
            one(i1, c1);
            one(i2, c2);
            one(i3, c3);
        });
        swept = true;
        __syncthreads();
        // ---- read-out in column order: the mask columns with a non-zero count, and their counts ----
        int mine = 0;
        for (int t = 0; t < run; t++) mine += ctr[excl + t] != 0u ? 1 : 0;
        int oexcl = 0;
        const int wtotal = block_scan(mine, oexcl);
        {
            int p = total + oexcl, c = excl;
#pragma unroll
            for (int k = 0; k < kWPT; k++) {
                u32 mk = kw[k];
                const int base = (int)lo + 32 * (tid * kWPT + k);
                while (mk) {
                    const u32 v = ctr[c++];
                    if (v) {
                        out[p] = base + (int)__builtin_ctz(mk);
                        vout[p] = (int)v;
                        p++;
                    }
                    mk &= mk - 1u;
                }
                K[tid * kWPT + k] = 0u;                            // the window is all zero again
            }
        }
        total += wtotal;
        __syncthreads();
        lo += W;
        if (ndist <= kCountSlots / 2) W = W * 2 < kCountMaxCols ? W * 2 : kCountMaxCols;   // (else: as dense, as wide)
    }
    if (tid == 0) cnt[i - row_begin] = total;
}

static hipError_t launch_dense_count(const int2 *ab, const int *Bcol, long long nnzB, int cols, const RowRec *rec,
                                     const long long *recpre, int nrows, int row_begin, int *tmp, int *cnt,
                                     const int *Frow, const int *Fcol, int *vals, hipStream_t s)
{
    constexpr auto kernel = k_dense_rows_count<kDenseThreadsBig>;
    if (nrows <= 0) return hipSuccess;
    constexpr int bytes = kCountWords * 4 + kCountWords * 2 + kCountSlots * 4;
    static std::atomic<bool> attr_set[64] = {};          // (per (kernel, device) pair, as in launch_dense_impl)
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kernel, dim3(nrows), dim3(kDenseThreadsBig), bytes, s, ab, Bcol,
                       (int)(nnzB > 0x7fffffffll ? 0x7fffffffll : nnzB), cols, rec, recpre, row_begin, tmp, cnt, Frow, Fcol, vals);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// RANK ROWS (class kRankBin): rows of 2048 < F_i <= kRankCap products when the column range is several windows of the
// small dense shape.  The workgroup's LDS holds a two-level RANK bitmap instead of a dense one -- `top`, one bit per
// 32-column word of the whole column range, and one 32-bit slot per SET top bit, addressed by the bit's rank (the
// one-wave kernels' accumulator at workgroup scope, wave_rows.inc).  Slots are as many as the row has distinct words
// (<= F_i), not as many as the matrix has columns: the row is done in TWO sweeps over its products (top bits; slot bits)
// and ONE read-out proportional to the row, whatever the column count is -- the windowed shape runs one sweep and one
// 4096-word read-out per 2^18 columns, four of each at 2^20 columns for a row that fills 1-2 % of every window, and
// every one of them is a trip to memory that the row's eight waves wait for (profiles/r04_heavy_ablation.log).
// LDS per workgroup: top (cols / 32 bits) + ranks (32 bits per top word) + kRankCap slots: 32 KiB at 2^20 columns,
// beside the gather plan -- four workgroups per CU, as many as the windowed shape.
constexpr int kRankThreads = 512;
constexpr int kRankSlotsPerThread = kRankCap / kRankThreads;
static_assert(kRankCap % kRankThreads == 0, "whole slots per thread");
constexpr int kRankQPT = 8, kRankInFlight = 4;
constexpr int kRankSpan = 1 << 20;           // columns one pass covers: the top bitmap's reach (4 KiB of top bits)

// kSpans false: the column range is one span (the common case: one pass, its quads kept in registers).
// MODE (Frow / Fcol: F's or D's CSR, absolute row ids; unused by None):
//   Drop    C = !F .* (A*B): after each span's slot sweep, the bit of every column of F's row that the span's accumulator
//           holds is cleared from its slot; the read-out takes its positions from the slots' popcounts, so it is unchanged
//   Insert  C = D | (A*B): each span's columns of D's row that lie in [0, cols) are set as top bits after the span's first
//           sweep and in their slots after its second; the read-out is unchanged
// Every instance compiles to the instructions of the separate kernel it replaced (tools/isa_diff.py).
template <bool kSpans, MaskMode MODE>
__global__ __launch_bounds__(kRankThreads, 8) void k_rank_rows(const int2 *__restrict__ ab, const int *__restrict__ Bcol, int nnzB,
                                                               int cols, int topw,
                                                               const RowRec *__restrict__ rec,
                                                               const long long *__restrict__ recpre,
                                                               int row_begin, int *__restrict__ tmp, int *__restrict__ cnt,
                                                               const int *__restrict__ Frow, const int *__restrict__ Fcol)
{
    constexpr bool DROP = MODE == MaskMode::Drop, INS = MODE == MaskMode::Insert;
    // (the class is bound by LDS instruction issue -- profiles/r04_rank_rows_phases.log -- so the layout is chosen for few LDS
    // instructions: a top word and its rank are one 8-byte pair, one read in sweep 2)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint2 *tp = reinterpret_cast<uint2 *>(lds_raw);                             // [topw] x: bit (c >> 5) of the span, 32 per word; y: set bits before the word
    u32 *tp32 = reinterpret_cast<u32 *>(lds_raw);
    u32 *S = tp32 + 2 * topw;                                                   // [kRankCap] slots; later the staged row
    constexpr int kWaves = kRankThreads / 64;
    constexpr int SPT = kRankSlotsPerThread;
    __shared__ GatherLds<kRankThreads, kRankQPT> G;
    __shared__ int wtot[kWaves];
    __shared__ unsigned short fw[kRankThreads];                                 // top word that holds slot t * SPT
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nclear = topw + kRankCap / 2;                                     // 8-byte words of the accumulator
    {
        u64 *z = reinterpret_cast<u64 *>(lds_raw);
        for (int t = tid; t < nclear; t += kRankThreads) z[t] = 0ull;
    }
    gather_init(G);
    __syncthreads();

    const RowRec q = rec[blockIdx.x];
    const int a0 = q.a0, a1 = q.a0 + q.alen;
    int *out = tmp + recpre[blockIdx.x];

    GatherState g;
    // a row whose quads are one step of the gather keeps them in registers for every later sweep: no plan look-ups, no loads
    Int4U hq[kRankInFlight];
    u32 hm[kRankInFlight];
#pragma unroll
    for (int u = 0; u < kRankInFlight; u++) {                      // (slots the gather's last step leaves out stay empty)
        hq[u].x = hq[u].y = hq[u].z = hq[u].w = 0;
        hm[u] = 0u;
    }
    bool held = false;                                             // uniform
    // The column range is taken in SPANS of 2^20 columns (the top bitmap's reach): one for the matrices the class was built
    // for, up to sixteen on wider ones -- where the small dense shape would sweep and read out 4 * sixteen windows.
    const int nspans = kSpans ? (int)(((long long)cols + kRankSpan - 1) / kRankSpan) : 1;
    int total = 0;
    for (int sp = 0; sp < nspans; sp++) {
        const u32 lo = kSpans ? (u32)sp * (u32)kRankSpan : 0u;
        // ---- sweep 1: the top bits -----------------------------------------------------------------------------------
        auto top_bits = [&](const Int4U &v, u32 vm, int u) {
            if (!kSpans) {
                hq[u] = v;
                hm[u] = vm;
            }
            const u32 c0 = (u32)v.x - lo, c1 = (u32)v.y - lo, c2 = (u32)v.z - lo, c3 = (u32)v.w - lo;   // (columns below the span wrap to huge values)
            insert_quad(tp32, (vm & 1u) && (!kSpans || c0 < (u32)kRankSpan), (vm & 2u) && (!kSpans || c1 < (u32)kRankSpan),
                        (vm & 4u) && (!kSpans || c2 < (u32)kRankSpan), (vm & 8u) && (!kSpans || c3 < (u32)kRankSpan), (c0 >> 10) * 2u, (c1 >> 10) * 2u, (c2 >> 10) * 2u, (c3 >> 10) * 2u,
                        1u << ((c0 >> 5) & 31), 1u << ((c1 >> 5) & 31), 1u << ((c2 >> 5) & 31), 1u << ((c3 >> 5) & 31), kSpans);
        };
        gather_sweep<kRankThreads, kRankQPT, kRankInFlight>(G, g, ab, Bcol, nnzB, a0, a1, sp == 0, top_bits);
        if (!kSpans) held = g.plan_kept && g.QB <= kRankInFlight * kRankThreads;   // (only ever used by sweep 2 of the single span)
        if constexpr (INS) {
            // D's row, read coalesced a workgroup's width at a time: its columns in the span are top bits like the products'
            // (the class was sized by F_i + |D_i|: the slots still fit), whether or not a product reached the span
            const int d0 = Frow[q.row], d1 = Frow[q.row + 1];
            for (int k = d0 + tid; k < d1; k += kRankThreads) {
                const u32 c = (u32)Fcol[k], cl = c - lo;
                if (c < (u32)cols && cl < (u32)kRankSpan) atomicOr(&tp32[(cl >> 10) * 2u], 1u << ((cl >> 5) & 31));
            }
            __syncthreads();
        }
        // ---- ranks of the top bits: thread t owns the words [t*WPT, (t+1)*WPT) -----------------------------------------
        int nslots = 0, spt = SPT;
        {
            const int WPT = topw / kRankThreads;                   // 1 or 2
            u32 x[2];
            int c[2], run = 0;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                x[k] = k < WPT ? tp[tid * WPT + k].x : 0u;
                c[k] = run;
                run += __popc(x[k]);
            }
            const int inc = wave_incl_scan(run);
            if (lane == 63) wtot[wave] = inc;
            __syncthreads();
            int off = 0;
            for (int k = 0; k < kWaves; k++) {
                const int t = wtot[k];
                if (k < wave) off += t;
                nslots += t;
            }
            // slots per thread of the read-out: the row's slots spread evenly over the workgroup (a row of 2500 slots: five
            // per thread on all eight waves, not twelve on the first four)
            spt = (nslots + kRankThreads - 1) / kRankThreads;
            spt = spt < 1 ? 1 : (spt > SPT ? SPT : spt);
#pragma unroll
            for (int k = 0; k < 2; k++)
                if (k < WPT) {
                    const int pre = off + inc - run + c[k], end = pre + __popc(x[k]);
                    tp[tid * WPT + k].y = (u32)pre;
                    for (int j = (pre + spt - 1) / spt; j * spt < end && j < kRankThreads; j++) fw[j] = (unsigned short)(tid * WPT + k);   // (the first slot of thread j lies in this word)
                }
            __syncthreads();
        }
        // ---- sweep 2: bit (c & 31) of the slot whose index is the rank of top bit (c >> 5) ----------------------------
        auto slot_bits = [&](const Int4U &v, u32 vm, int) {
            const u32 c0 = (u32)v.x - lo, c1 = (u32)v.y - lo, c2 = (u32)v.z - lo, c3 = (u32)v.w - lo;
            const bool i0 = (vm & 1u) && (!kSpans || c0 < (u32)kRankSpan), i1 = (vm & 2u) && (!kSpans || c1 < (u32)kRankSpan);
            const bool i2 = (vm & 4u) && (!kSpans || c2 < (u32)kRankSpan), i3 = (vm & 8u) && (!kSpans || c3 < (u32)kRankSpan);
            const uint2 x0 = tp[i0 ? c0 >> 10 : 0u], x1 = tp[i1 ? c1 >> 10 : 0u], x2 = tp[i2 ? c2 >> 10 : 0u], x3 = tp[i3 ? c3 >> 10 : 0u];
            const u32 r0 = x0.y + __popc(__builtin_amdgcn_ubfe(x0.x, 0u, (c0 >> 5) & 31)), r1 = x1.y + __popc(__builtin_amdgcn_ubfe(x1.x, 0u, (c1 >> 5) & 31));
            const u32 r2 = x2.y + __popc(__builtin_amdgcn_ubfe(x2.x, 0u, (c2 >> 5) & 31)), r3 = x3.y + __popc(__builtin_amdgcn_ubfe(x3.x, 0u, (c3 >> 5) & 31));
            // (r < kRankCap always on consistent operands: slots <= F_i <= kRankCap; a rewritten operand is cut off, not LDS overrun)
            insert_quad(S, i0 && r0 < (u32)kRankCap, i1 && r1 < (u32)kRankCap, i2 && r2 < (u32)kRankCap, i3 && r3 < (u32)kRankCap, r0, r1, r2, r3,
                        1u << (c0 & 31), 1u << (c1 & 31), 1u << (c2 & 31), 1u << (c3 & 31), kSpans);
        };
        if (held) {
#pragma unroll
            for (int u = 0; u < kRankInFlight; u++)
                if ((long long)u * kRankThreads < g.QB) slot_bits(hq[u], hm[u], u);   // (uniform: the slots the gather's one step filled)
            __syncthreads();
        } else {
            gather_sweep<kRankThreads, kRankQPT, kRankInFlight>(G, g, ab, Bcol, nnzB, a0, a1, false, slot_bits);
        }
        if constexpr (INS) {                                       // D's columns into the slots their top bits rank
            const int d0 = Frow[q.row], d1 = Frow[q.row + 1];
            for (int k = d0 + tid; k < d1; k += kRankThreads) {
                const u32 c = (u32)Fcol[k], cl = c - lo;
                if (c < (u32)cols && cl < (u32)kRankSpan) {
                    const uint2 x = tp[cl >> 10];
                    const u32 r = x.y + __popc(__builtin_amdgcn_ubfe(x.x, 0u, (cl >> 5) & 31));
                    if (r < (u32)kRankCap) atomicOr(&S[r], 1u << (cl & 31));   // (always, on consistent operands)
                }
            }
            __syncthreads();
        }
        if constexpr (DROP) {
            if (nslots > 0) {                                      // (uniform: a span without products has nothing to clear)
                // F's row, read coalesced a workgroup's width at a time: a column whose top bit is set has a slot
                const int f0 = Frow[q.row], f1 = Frow[q.row + 1];
                const u32 reach = (u32)topw << 10;                 // columns the top bitmap covers (F's columns may lie beyond B's)
                for (int k = f0 + tid; k < f1; k += kRankThreads) {
                    const u32 c = (u32)Fcol[k] - lo;
                    if (c < reach) {
                        const uint2 x = tp[c >> 10];
                        const u32 b = (c >> 5) & 31;
                        const u32 r = x.y + __popc(__builtin_amdgcn_ubfe(x.x, 0u, b));
                        if (((x.x >> b) & 1u) && r < (u32)kRankCap) atomicAnd(&S[r], ~(1u << (c & 31)));
                    }
                }
                __syncthreads();
            }
        }
        // ---- read-out: slots are in column order.  Thread t owns the slots [t*SPT, (t+1)*SPT): their masks go to registers,
        // one block scan gives the thread its place in the row, the top word of its first slot was noted by the rank scan and
        // the others follow by walking the top bits; the columns are staged in LDS (over the slots, which every thread has
        // read by then) and streamed out coalesced.
        u32 m[SPT];
        int mine = 0;
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            m[k] = k < spt ? S[tid * spt + k] : 0u;
            mine += __popc(m[k]);
        }
        const int inc = wave_incl_scan(mine);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int pos = inc - mine, stotal = 0;
        for (int k = 0; k < kWaves; k++) {
            const int t = wtot[k];
            if (k < wave) pos += t;
            stotal += t;
        }
        if (nslots > kRankCap) nslots = kRankCap;
        const int s0 = tid * spt;
        if (s0 < nslots) {
            int t = fw[tid];
            const uint2 first = tp[t];
            u32 rem = first.x;
            for (int skip = s0 - (int)first.y; skip > 0; skip--) rem &= rem - 1u;
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                if (k < spt && s0 + k < nslots) {
                    while (!rem && t + 1 < topw) rem = tp[++t].x;
                    const u32 base = lo + (((u32)t << 10) | ((u32)__builtin_ctz(rem | 0x80000000u) << 5));
                    rem &= rem - 1u;
                    u32 mk = m[k];
                    while (mk) {
                        if (pos < kRankCap) S[stage_swz(pos)] = base | (u32)__builtin_ctz(mk);   // (always, on consistent operands)
                        pos++;
                        mk &= mk - 1u;
                    }
                }
            }
        }
        __syncthreads();
        if (total + stotal > q.f) stotal = q.f > total ? q.f - total : 0;          // (never, on consistent operands: the row's room is F_i <= kRankCap)
        for (int t = tid; t < stotal; t += kRankThreads) __builtin_nontemporal_store((int)S[stage_swz(t)], out + total + t);
        total += stotal;
        if (sp + 1 < nspans) {                                     // the accumulator all zero again for the next span
            __syncthreads();
            u64 *z = reinterpret_cast<u64 *>(lds_raw);
            for (int t = tid; t < nclear; t += kRankThreads) z[t] = 0ull;
            __syncthreads();
        }
    }
    if (tid == 0) cnt[q.row - row_begin] = total;
}

template <MaskMode MODE, int THREADS>
static hipError_t launch_dense_impl(const int2 *ab, const int *Bcol, long long nnzB, int cols, const RowRec *rec,
                                    const long long *recpre, int nrows, int row_begin, int *tmp, int *cnt,
                                    const int *Frow, const int *Fcol, hipStream_t s)
{
    constexpr bool MASKED = MODE == MaskMode::Keep;
    constexpr auto kernel = k_dense_rows<MODE, THREADS>;
    if (nrows <= 0) return hipSuccess;
    const long long cap_words = THREADS == kDenseThreadsBig ? kDenseMaxWords : kMidMaxWords;
    const long long max_words = MASKED ? cap_words / 2 : cap_words;   // two bitmaps share the window
    long long words = ((long long)cols + 63) / 64;
    if (words > max_words) words = max_words;
    if (words < 1) words = 1;
    const int bytes = (int)words * 8 * (MASKED ? 2 : 1);
    // the attribute belongs to the (kernel, device) pair: a process may hold contexts on several GPUs
    static std::atomic<bool> attr_set[64] = {};          // (contexts on other threads launch this too)
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap_words * 8);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kernel, dim3(nrows), dim3(THREADS), bytes, s, ab, Bcol,
                       (int)(nnzB > 0x7fffffffll ? 0x7fffffffll : nnzB), cols, (int)words, rec, recpre, row_begin, tmp, cnt, Frow, Fcol);
    return hipGetLastError();
}

// rows of the rank class are told apart by the prepass (bin_of): rank_cap_for_cols(cols) products or fewer
int rank_cap_for_cols(long long cols)
{
    // (development switch, read once: BSPGEMM_RANK_ROWS=0 no rank class, =2 also where the small shape needs ONE window)
    static const int mode = [] { const char *e = getenv("BSPGEMM_RANK_ROWS"); return e ? atoi(e) : 1; }();
    if (mode <= 0 || cols > (1ll << 24)) return 0;                 // (one pass per 2^20 columns: sixteen at most; wider matrices keep the dense shapes)
    if (mode == 1 && cols <= (1ll << 18)) return 0;
    return kRankCap;
}

static hipError_t launch_rank_rows(const int2 *ab, const int *Bcol, long long nnzB, int cols, const RowRec *rec,
                                   const long long *recpre, int nrows, int row_begin, int *tmp, int *cnt, MaskMode mode,
                                   const int *Frow, const int *Fcol, hipStream_t s)
{
    if (nrows <= 0) return hipSuccess;
    const long long span = cols < kRankSpan ? cols : kRankSpan;
    const int topw = (int)(((span + 1023) >> 10) + kRankThreads - 1) / kRankThreads * kRankThreads;   // whole words per thread
    const int bytes = topw * 8 + kRankCap * 4;
    const int nnzB32 = (int)(nnzB > 0x7fffffffll ? 0x7fffffffll : nnzB);
    const bool spans = cols > kRankSpan;
    auto kernel = spans ? k_rank_rows<true, MaskMode::None> : k_rank_rows<false, MaskMode::None>;
    if (mode == MaskMode::Drop) kernel = spans ? k_rank_rows<true, MaskMode::Drop> : k_rank_rows<false, MaskMode::Drop>;
    if (mode == MaskMode::Insert) kernel = spans ? k_rank_rows<true, MaskMode::Insert> : k_rank_rows<false, MaskMode::Insert>;
    hipLaunchKernelGGL(kernel, dim3(nrows), dim3(kRankThreads), bytes, s, ab, Bcol, nnzB32, cols, topw, rec, recpre, row_begin, tmp, cnt,
                       Frow, Fcol);
    return hipGetLastError();
}

hipError_t launch_dense_rows(int bin, const int2 *ab, const int *Bcol, long long nnzB, int cols,
                             const RowRec *rec, const long long *recpre, int nrows, int row_begin,
                             int *tmp, int *cnt, MaskMode mode, const int *Frow, const int *Fcol, hipStream_t s, int *vals)
{
    if (mode == MaskMode::Count)                                   // every counted row the one-wave kernel does not take
        return launch_dense_count(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, Frow, Fcol, vals, s);
    if (mode == MaskMode::Keep)                                    // every masked row, whatever its class
        return launch_dense_impl<MaskMode::Keep, kDenseThreadsBig>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, Frow, Fcol, s);
    if (bin == kRankBin) return launch_rank_rows(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, mode, Frow, Fcol, s);
    const bool mid = bin == kMidBin;
    if (mode == MaskMode::Insert)
        return mid ? launch_dense_impl<MaskMode::Insert, kDenseThreadsMid>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, Frow, Fcol, s)
                   : launch_dense_impl<MaskMode::Insert, kDenseThreadsBig>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, Frow, Fcol, s);
    if (mode == MaskMode::Drop)
        return mid ? launch_dense_impl<MaskMode::Drop, kDenseThreadsMid>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, Frow, Fcol, s)
                   : launch_dense_impl<MaskMode::Drop, kDenseThreadsBig>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, Frow, Fcol, s);
    return mid ? launch_dense_impl<MaskMode::None, kDenseThreadsMid>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, nullptr, nullptr, s)
               : launch_dense_impl<MaskMode::None, kDenseThreadsBig>(ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, nullptr, nullptr, s);
}

}  // namespace bsp
