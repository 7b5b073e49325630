// wave_masked.hip -- masked product C = F .* (A*B), one wavefront per row, MASK-FIRST.
//
// The reference (SpGEMM_masked, final/SpGEMM_mpi_omp.c:232-288) presets its flag array so that
// only the columns of F's row can ever be appended (:253-255), then runs the ordinary Gustavson
// loop.  The same idea with the rank bitmap of wave_rows.inc: the structure is built from the
// MASK row's columns (its size follows |F_i|, not the product count), all its levels are kept,
// and the row's products are then STREAMED through it read-only -- a product whose digit path
// exists down to a set level-0 bit marks that bit in a "kept" word.  Products never have to be
// resident, so a row may have any number of them; what limits the one-wave path is the mask row
// (<= 2048 entries, cols <= 2^23 so that three 5-bit levels suffice and no slot buffer is reused).
// Longer mask rows / wider matrices take the two-bitmap window kernel (dense_rows.hip).
//
// Products are walked 64 A-nonzeros at a time in windows of 256 products, with the same
// starts-bitmap flattening as the unmasked kernel (all 64 lanes load B.col_idx every step).
// Output: the kept bits are read out in rank order = ascending columns, staged in LDS, streamed
// to tmp[recpre ..) coalesced; cnt[row] = their number (<= |F_i|).
//
// k_wave_masked_count, the counting twin (C = F .* (A*B) with the number of products per entry, PLUS_PAIR under the
// mask): one more blocked scan gives the level-0 words' popcount prefix, so every distinct mask column has a rank and an
// LDS counter (CAP per wave, cleared over the row's distinct columns only).  A hit adds one to its counter instead of
// setting a kept bit; the read-out walks the mask row in rank order and emits the columns whose counter is non-zero, the
// counts going to vals at the same offsets as the columns in tmp.  The kernel body is shared text (wave_masked_body.inc).
#include "kernels.hpp"
#include "wave.hpp"

namespace bsp {

constexpr int kMaskWinChunks = 4;       // products per window = 256, kept in registers
constexpr long long kMaskWaveMaxProducts = 8192;   // beyond this a row is streamed by a whole workgroup

template <int LEVELS, int CHUNKS, bool COUNT = false>
struct MaskCfg {
    static constexpr int CAP = 64 * CHUNKS;
    static constexpr int TOPW = 256;
    static constexpr int bytes_per_wave = 4 * TOPW + 2 * TOPW + 8 * kMaskWinChunks + 4 * 64      // top, topPre, starts, delta
                                          + 4 * CAP * 3                                          // SA, K0, L0w
                                          + (LEVELS >= 3 ? 4 * CAP + 2 * CAP : 32)               // SB, preB
                                          + (COUNT ? 4 * CAP + 2 * CAP : 0);                     // counters, their rank bases
    static constexpr int w4 = (4 * bytes_per_wave > 64 * 1024) ? 0 : (160 * 1024 / (4 * bytes_per_wave)) * 4;
    static constexpr int w2 = (2 * bytes_per_wave > 64 * 1024) ? 0 : (160 * 1024 / (2 * bytes_per_wave)) * 2;
    static constexpr int WAVES = (w4 >= w2 && w4 > 0) ? 4 : (w2 > 0 ? 2 : 1);
};

template <int LEVELS, int CHUNKS>
__global__ __launch_bounds__((64 * MaskCfg<LEVELS, CHUNKS>::WAVES))
void k_wave_masked(const int2 *__restrict__ ab, const int *__restrict__ Bcol, int topw,
                   const int *__restrict__ Frow, const int *__restrict__ Fcol,
                   const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                   int nrows, int row_begin, int *__restrict__ tmp, int *__restrict__ cnt)
{
    constexpr bool COUNT = false;
    int *const vals = nullptr;
#include "wave_masked_body.inc"
}

// C = F .* (A*B) with path counts (PLUS_PAIR under the mask): the same kernel with one LDS counter per distinct column of the
// mask row instead of the kept bits; a kept column's count goes to vals at its offset in tmp.  Body: wave_masked_body.inc
template <int LEVELS, int CHUNKS>
__global__ __launch_bounds__((64 * MaskCfg<LEVELS, CHUNKS, true>::WAVES))
void k_wave_masked_count(const int2 *__restrict__ ab, const int *__restrict__ Bcol, int topw,
                         const int *__restrict__ Frow, const int *__restrict__ Fcol,
                         const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                         int nrows, int row_begin, int *__restrict__ tmp, int *__restrict__ cnt, int *__restrict__ vals)
{
    constexpr bool COUNT = true;
#include "wave_masked_body.inc"
}

template <int LEVELS, int CHUNKS, bool COUNT>
static void launch_mask_one(const int2 *ab, const int *Bcol, int topw, const int *Frow, const int *Fcol,
                            const RowRec *rec, const long long *recpre, int nrows, int row_begin,
                            int *tmp, int *cnt, int *vals, hipStream_t s)
{
    using Cfg = MaskCfg<LEVELS, CHUNKS, COUNT>;
    const long long rows_per_wg = (long long)Cfg::WAVES * kRowsPerWave;
    const int grid = (int)((nrows + rows_per_wg - 1) / rows_per_wg);
    if constexpr (COUNT)
        hipLaunchKernelGGL((k_wave_masked_count<LEVELS, CHUNKS>), dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                           ab, Bcol, topw, Frow, Fcol, rec, recpre, nrows, row_begin, tmp, cnt, vals);
    else
        hipLaunchKernelGGL((k_wave_masked<LEVELS, CHUNKS>), dim3(grid), dim3(64 * Cfg::WAVES), 0, s,
                           ab, Bcol, topw, Frow, Fcol, rec, recpre, nrows, row_begin, tmp, cnt);
}

template <int LEVELS, bool COUNT>
static void launch_mask_levels(int bin, const int2 *ab, const int *Bcol, int topw, const int *Frow,
                               const int *Fcol, const RowRec *rec, const long long *recpre, int nrows,
                               int row_begin, int *tmp, int *cnt, int *vals, hipStream_t s)
{
    // the mask-first kernel is instantiated for 7 mask-row capacities; a class uses the smallest
    // one that holds its rows (mask rows are short: the fine classes of the plain product buy nothing)
    const int chunks = kWaveChunks[bin];
#define BSP_MASK(C) launch_mask_one<LEVELS, C, COUNT>(ab, Bcol, topw, Frow, Fcol, rec, recpre, nrows, row_begin, tmp, cnt, vals, s)
    if (chunks <= 1) BSP_MASK(1);
    else if (chunks <= 2) BSP_MASK(2);
    else if (chunks <= 4) BSP_MASK(4);
    else if (chunks <= 8) BSP_MASK(8);
    else if (chunks <= 12) BSP_MASK(12);
    else if (chunks <= 16) BSP_MASK(16);
    else BSP_MASK(32);
#undef BSP_MASK
}

bool wave_masked_supported(int cols) { return levels_for_cols(cols) <= 3; }

void launch_wave_masked(int bin, const int2 *ab, const int *Bcol, int cols, const int *Frow, const int *Fcol,
                        const RowRec *rec, const long long *recpre, int nrows, int row_begin,
                        int *tmp, int *cnt, int *vals, hipStream_t s)
{
    if (nrows <= 0) return;
    const int levels = levels_for_cols(cols);
    const long long span = 1ll << (5 * levels);
    const int topw = (int)(((long long)cols + span - 1) / span);
#define BSP_MASK_L(L) (vals ? launch_mask_levels<L, true>(bin, ab, Bcol, topw, Frow, Fcol, rec, recpre, nrows, row_begin, tmp, cnt, vals, s) \
                            : launch_mask_levels<L, false>(bin, ab, Bcol, topw, Frow, Fcol, rec, recpre, nrows, row_begin, tmp, cnt, vals, s))
    switch (levels) {
    case 1: BSP_MASK_L(1); break;
    case 2: BSP_MASK_L(2); break;
    default: BSP_MASK_L(3); break;
    }
#undef BSP_MASK_L
}

// mask length per row (0 when the row has no products): what the masked multiply bins and offsets by
__global__ void k_mask_lengths(const long long *__restrict__ F, const int *__restrict__ Frow, int row_begin,
                               int n, long long *__restrict__ mlen)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        long long m = F[i] > 0 ? (long long)(Frow[row_begin + i + 1] - Frow[row_begin + i]) : 0;
        // a wave streams its row's products 256 at a time: rows with very many products go to the
        // 1024-thread dense kernel whatever their mask length (class = dense when m > kMaxWaveCap;
        // the larger m only reserves more room in tmp)
        if (m > 0 && m <= kMaxWaveCap && F[i] > kMaskWaveMaxProducts) m = kMaxWaveCap + 1;
        mlen[i] = m;
    }
}

void launch_mask_lengths(const long long *F, const int *Frow, int row_begin, int n, long long *mlen, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_mask_lengths, dim3((n + 255) / 256), dim3(256), 0, s, F, Frow, row_begin, n, mlen);
}

// k_mask_lengths of the counting product, which also needs the range's largest product count: a count is at most its
// row's F_i, and the host refuses the product when that can exceed int32.  *maxF (zeroed by the caller) = max F_i.
__global__ __launch_bounds__(256) void k_mask_lengths_count(const long long *__restrict__ F, const int *__restrict__ Frow,
                                                            int row_begin, int n, long long *__restrict__ mlen,
                                                            unsigned long long *__restrict__ maxF)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    long long f = 0;
    if (i < n) {
        f = F[i];
        long long m = f > 0 ? (long long)(Frow[row_begin + i + 1] - Frow[row_begin + i]) : 0;
        if (m > 0 && m <= kMaxWaveCap && f > kMaskWaveMaxProducts) m = kMaxWaveCap + 1;   // (as k_mask_lengths)
        mlen[i] = m;
    }
    // the wave's maximum, then one atomic per wave
    u32 hi = (u32)((unsigned long long)f >> 32), lo = (u32)f;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 ohi = (u32)__shfl_xor((int)hi, d, 64), olo = (u32)__shfl_xor((int)lo, d, 64);
        if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; }
    }
    if ((threadIdx.x & 63) == 0 && (hi | lo)) atomicMax(maxF, ((unsigned long long)hi << 32) | lo);
}

void launch_mask_lengths_count(const long long *F, const int *Frow, int row_begin, int n, long long *mlen,
                               unsigned long long *maxF, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_mask_lengths_count, dim3((n + 255) / 256), dim3(256), 0, s, F, Frow, row_begin, n, mlen, maxF);
}

}  // namespace bsp
