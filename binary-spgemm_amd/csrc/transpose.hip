// transpose.hip -- AT = pattern(A)^T on the device (bspgemm_matrix_transpose, include/bspgemm.h), and the sorted
// duplicate-free copy of an operand that two of them make (operand_canonical, internal.hpp).
//
// A stable LSD radix sort of the pairs (k = column, i = row) keyed by k alone, then one compaction pass.  A's entries in
// CSR order are already ordered by i, so a stable sort by k leaves every row of AT in ascending i with duplicate pairs
// adjacent; no atomic decides any order, so the result is deterministic.  Per digit pass (8-bit digits, as many passes as
// bits(A.cols - 1) needs, at least one):
//   k_tr_hist     per tile of 4096 entries: digit histogram in LDS (one add per run of equal digits in a wave)
//   scan          launch_scan_counts over the (digit, tile) counts, digit-major: where each tile's digit run goes
//   k_tr_scatter  per tile: stable rank of every entry (wave64 ballots + per-wave digit counters in LDS), the tile
//                 reordered in LDS, written out run by run
// The first pass reads A itself: k from col_idx (range-checked, an error word on the device), i found by a binary search
// of the tile's row_ptr window (staged in LDS).  Then k_tr_dedup_count / scan / k_tr_dedup_write keep the first pair of
// every run of equal pairs, write AT.col_idx at its compacted place (staged per tile in LDS) and AT.row_ptr where k
// changes (long runs of empty rows filled by the whole wave).
#include "internal.hpp"
#include "wave.hpp"

namespace bsp {

constexpr int kTrThreads = 256;                       // four waves
constexpr int kTrItems = 16;
constexpr int kTrTile = kTrThreads * kTrItems;       // entries per workgroup
constexpr int kTrWaveSpan = kTrTile / 4;             // consecutive entries of one wave in a tile
constexpr int kDigitBits = 8;
constexpr int kRadix = 1 << kDigitBits;
static_assert(kRadix == kTrThreads, "one thread per digit in the per-tile digit scan");
// entries the int32 index arithmetic of the kernels allows (tile ends stay below INT_MAX)
constexpr long long kTrMaxNnz = 0x7fffffffll - 2 * kTrTile;

struct TrScalars {
    long long nnz;          // nnz(AT)
    unsigned err;           // 1: a column outside [0, A.cols)
    unsigned pad;
};

// lanes (of those with `in`) whose digit equals this lane's
__device__ __forceinline__ u64 match_digit(unsigned d, int nbits, bool in)
{
    u64 m = __ballot(in);
    for (int b = 0; b < nbits; b++) {
        const bool bit = (d >> b) & 1u;
        const u64 bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__device__ __forceinline__ unsigned digit_of(int k, int shift) { return ((unsigned)k >> shift) & (kRadix - 1); }

// largest r in [lo, hi] with rp[r] <= e: the row that holds entry e (empty rows share their row_ptr with the next row)
template <typename P>
__device__ __forceinline__ int row_of(P rp, int lo, int hi, int e)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rp[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// FIRST: keys are A.col_idx, checked against cols (an out-of-range key sets *err and sorts as 0)
template <bool FIRST>
__global__ __launch_bounds__(kTrThreads) void k_tr_hist(const int *__restrict__ keys, int E, int cols, int shift, int nbits,
                                                       int ntiles, int *__restrict__ hist, unsigned *__restrict__ err)
{
    __shared__ int h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int base = blockIdx.x * kTrTile + w * kTrWaveSpan;
    int key[kTrItems];
#pragma unroll
    for (int j = 0; j < kTrItems; j++) key[j] = base + j * 64 + lane < E ? keys[base + j * 64 + lane] : 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kTrItems; j++) {
        const bool in = base + j * 64 + lane < E;
        int k = key[j];
        if (FIRST && (unsigned)k >= (unsigned)cols) {
            bad |= in;
            k = 0;
        }
        const unsigned d = digit_of(k, shift);
        const u64 peers = match_digit(d, nbits, in);
        if (in && (peers & mask_lt(lane)) == 0) atomicAdd(&h[d], __popcll(peers));
    }
    if (FIRST && bad) atomicOr(err, 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one digit pass.  Entry order inside a tile: wave by wave, each wave's span in chunks of 64.  `prefix`
// (digit-major over tiles) is the scan of k_tr_hist's counts.  FIRST: keys from A.col_idx, values = rows from row_ptr.
template <bool FIRST>
__global__ __launch_bounds__(kTrThreads) void k_tr_scatter(const int *__restrict__ kin, const int *__restrict__ vin,
                                                          const int *__restrict__ row_ptr, int rows, int E, int cols,
                                                          int shift, int nbits, int ntiles,
                                                          const long long *__restrict__ prefix, int *__restrict__ kout,
                                                          int *__restrict__ vout)
{
    __shared__ int wcnt[4][kRadix];      // per wave: entries of each digit so far; then the wave's offset in the tile's run
    __shared__ int dstart[kRadix];       // start of each digit's run in the reordered tile
    __shared__ int gbase[kRadix];        // where that run goes in the output
    __shared__ int stage[2 * kTrTile];   // FIRST: the tile's row_ptr window; then the tile in sorted order (keys, values)
    __shared__ int wsum[4];
    __shared__ int rspan[2];
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int t0 = blockIdx.x * kTrTile;
    const int t1 = min(t0 + kTrTile, E);
    for (int q = tid; q < 4 * kRadix; q += kTrThreads) (&wcnt[0][0])[q] = 0;
    int r_lo = 0, span = 0;
    bool staged = false;
    if (FIRST) {
        if (tid < 2) rspan[tid] = row_of(row_ptr, 0, rows - 1, tid == 0 ? t0 : t1 - 1);
        __syncthreads();
        r_lo = rspan[0];
        span = rspan[1] - r_lo + 1;                     // rows r_lo .. r_lo + span - 1 hold the tile
        staged = span < 2 * kTrTile;
        if (staged)
            for (int q = tid; q <= span; q += kTrThreads) stage[q] = row_ptr[r_lo + q];
    }
    __syncthreads();

    int key[kTrItems], val[kTrItems], rank[kTrItems];
    const int wbase = t0 + w * kTrWaveSpan;
#pragma unroll
    for (int j = 0; j < kTrItems; j++) {
        const int e = wbase + j * 64 + lane;
        const bool in = e < t1;
        int k = 0, v = 0;
        if (in) {
            k = kin[e];
            if (FIRST) {
                if ((unsigned)k >= (unsigned)cols) k = 0;     // (k_tr_hist has flagged it: the call fails)
                v = staged ? r_lo + row_of(stage, 0, span - 1, e) : row_of(row_ptr, r_lo, r_lo + span - 1, e);
            } else {
                v = vin[e];
            }
        }
        const unsigned d = digit_of(k, shift);
        const u64 peers = match_digit(d, nbits, in);
        const int r = __popcll(peers & mask_lt(lane));
        const int before = in ? wcnt[w][d] : 0;
        if (in && r == 0) wcnt[w][d] = before + __popcll(peers);   // (DS ops of a wave run in issue order)
        key[j] = k;
        val[j] = v;
        rank[j] = before + r;
    }
    __syncthreads();
    {
        const int d = tid;
        const int c0 = wcnt[0][d], c1 = wcnt[1][d], c2 = wcnt[2][d], c3 = wcnt[3][d];
        const int tot = c0 + c1 + c2 + c3;
        const int inc = wave_incl_scan(tot);
        if (lane == 63) wsum[w] = inc;
        gbase[d] = (int)prefix[(size_t)d * ntiles + blockIdx.x];
        wcnt[0][d] = 0;
        wcnt[1][d] = c0;
        wcnt[2][d] = c0 + c1;
        wcnt[3][d] = c0 + c1 + c2;
        __syncthreads();
        int off = inc - tot;
        for (int q = 0; q < w; q++) off += wsum[q];
        dstart[d] = off;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTrItems; j++) {
        const int e = wbase + j * 64 + lane;
        if (e < t1) {
            const unsigned d = digit_of(key[j], shift);
            const int p = dstart[d] + wcnt[w][d] + rank[j];
            stage[p] = key[j];
            stage[kTrTile + p] = val[j];
        }
    }
    __syncthreads();
    const int n = t1 - t0;
    for (int p = tid; p < n; p += kTrThreads) {
        const int k = stage[p];
        const unsigned d = digit_of(k, shift);
        const int o = gbase[d] + (p - dstart[d]);
        kout[o] = k;
        vout[o] = stage[kTrTile + p];
    }
}

// this thread's kTrItems consecutive sorted pairs from p0, and the pair before them ((-1, -1) at p0 = 0)
__device__ __forceinline__ int load_items(const int *__restrict__ keys, const int *__restrict__ vals, int p0, int E,
                                          int (&k)[kTrItems], int (&v)[kTrItems], int &pk, int &pv)
{
    pk = p0 > 0 && p0 <= E ? keys[p0 - 1] : -1;
    pv = p0 > 0 && p0 <= E ? vals[p0 - 1] : -1;
    if (p0 + kTrItems <= E) {
#pragma unroll
        for (int q = 0; q < kTrItems / 4; q++) {
            const int4 a = reinterpret_cast<const int4 *>(keys + p0)[q];
            const int4 b = reinterpret_cast<const int4 *>(vals + p0)[q];
            k[4 * q] = a.x; k[4 * q + 1] = a.y; k[4 * q + 2] = a.z; k[4 * q + 3] = a.w;
            v[4 * q] = b.x; v[4 * q + 1] = b.y; v[4 * q + 2] = b.z; v[4 * q + 3] = b.w;
        }
        return kTrItems;
    }
#pragma unroll
    for (int j = 0; j < kTrItems; j++) {
        k[j] = p0 + j < E ? keys[p0 + j] : -1;
        v[j] = p0 + j < E ? vals[p0 + j] : -1;
    }
    return E - p0 < 0 ? 0 : E - p0;
}

__global__ __launch_bounds__(kTrThreads) void k_tr_dedup_count(const int *__restrict__ keys, const int *__restrict__ vals,
                                                              int E, int *__restrict__ counts)
{
    __shared__ int wsum[4];
    int k[kTrItems], v[kTrItems], pk, pv;
    const int have = load_items(keys, vals, blockIdx.x * kTrTile + threadIdx.x * kTrItems, E, k, v, pk, pv);
    int c = 0;
#pragma unroll
    for (int j = 0; j < kTrItems; j++) {
        c += j < have && (k[j] != pk || v[j] != pv);
        pk = k[j];
        pv = v[j];
    }
    const int inc = wave_incl_scan(c);
    if (lane_id() == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// row_out[lo .. hi] = v for every lane that has such a range (lo <= hi).  A short range is the lane's own; the long ones
// are filled by the whole wave, one after the other, so that a long run of empty rows costs coalesced stores, not one
// lane's loop.  Wave-uniform control flow only.
__device__ __forceinline__ void fill_rows(int *__restrict__ row_out, int lo, int hi, int v)
{
    const bool wide = hi - lo >= 8;
    if (!wide)
        for (int r = lo; r <= hi; r++) row_out[r] = v;
    const int lane = lane_id();
    for (u64 pend = __ballot(wide); pend; pend &= pend - 1) {
        const int src = __ffsll((long long)pend) - 1;
        const int l = wave_bcast(lo, src), h = wave_bcast(hi, src), x = wave_bcast(v, src);
        for (long long r = (long long)l + lane; r <= h; r += 64) row_out[r] = x;
    }
}

// AT.col_idx[compacted position] = i for the first pair of every run of equal pairs; AT.row_ptr[r] = position of the first
// pair with k >= r, for r in [0, cols] (rows past the last key get nnz(AT))
__global__ __launch_bounds__(kTrThreads) void k_tr_dedup_write(const int *__restrict__ keys, const int *__restrict__ vals,
                                                              int E, int cols, const long long *__restrict__ tpre, int ntiles,
                                                              int *__restrict__ col_out, int *__restrict__ row_out,
                                                              TrScalars *__restrict__ scal)
{
    __shared__ int wsum[4];
    __shared__ int sval[kTrTile];       // the tile's kept values in output order: written out coalesced
    int k[kTrItems], v[kTrItems], pk, pv;
    const int p0 = blockIdx.x * kTrTile + threadIdx.x * kTrItems;
    const int have = load_items(keys, vals, p0, E, k, v, pk, pv);
    int c = 0;
    {
        int qk = pk, qv = pv;
#pragma unroll
        for (int j = 0; j < kTrItems; j++) {
            c += j < have && (k[j] != qk || v[j] != qv);
            qk = k[j];
            qv = v[j];
        }
    }
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int inc = wave_incl_scan(c);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    const int tbase = (int)tpre[blockIdx.x];
    int lpos = inc - c;                                                       // position in the tile's output
    for (int q = 0; q < w; q++) lpos += wsum[q];
    const int total = (int)tpre[ntiles];
#pragma unroll
    for (int j = 0; j < kTrItems; j++) {
        const bool in = j < have;
        const bool newkey = in && k[j] != pk;
        const bool keep = in && (newkey || v[j] != pv);
        if (keep) sval[lpos] = v[j];
        fill_rows(row_out, newkey ? pk + 1 : 1, newkey ? k[j] : 0, tbase + lpos);     // rows pk+1 .. k start here
        lpos += keep;
        if (in) {
            pk = k[j];
            pv = v[j];
        }
    }
    const bool last = have > 0 && p0 + have == E;                            // rows after the last key are empty
    fill_rows(row_out, last ? pk + 1 : 1, last ? cols : 0, total);
    __syncthreads();
    const int tcount = (int)tpre[blockIdx.x + 1] - tbase;
    for (int q = threadIdx.x; q < tcount; q += kTrThreads) col_out[tbase + q] = sval[q];
    if (blockIdx.x == 0 && threadIdx.x == 0) scal->nnz = total;
}

}  // namespace bsp

using namespace bsp;

// The sort's passes and where its arrays lie in the context's upper-bound workspace (ints): key and value arrays (two of
// each when there are two or more passes), the counts, their int64 scan, the scan's partials, the read-back scalars.
struct TrLayout {
    int bits, passes, ntiles, H;            // bits(cols - 1), radix passes, tiles of kTrTile entries, (digit, tile) counts
    size_t E4, o_hist, o_pre, o_part, o_scal, total;
};

static TrLayout tr_layout(int E, int cols)
{
    TrLayout l;
    l.bits = 0;
    while (l.bits < 31 && (1ll << l.bits) < (long long)cols) l.bits++;
    l.passes = l.bits <= kDigitBits ? 1 : (l.bits + kDigitBits - 1) / kDigitBits;
    l.ntiles = (E + kTrTile - 1) / kTrTile;
    l.H = kRadix * l.ntiles;
    l.E4 = ((size_t)E + 63) & ~(size_t)63;
    const size_t nbuf = l.passes > 1 ? 2 : 1;
    l.o_hist = 2 * nbuf * l.E4;
    l.o_pre = l.o_hist + (((size_t)l.H + 1) & ~(size_t)1);
    l.o_part = l.o_pre + 2 * ((size_t)l.H + 1);
    l.o_scal = l.o_part + 2 * ((size_t)l.H / 2048 + 4);
    l.total = l.o_scal + 4;
    return l;
}

size_t transpose_workspace_ints(long long E, int cols)
{
    return E > 0 && E <= kTrMaxNnz ? tr_layout((int)E, cols).total : 0;
}

extern "C" bspgemm_status bspgemm_matrix_transpose(bspgemm_context *ctx, const bspgemm_matrix *A, bspgemm_matrix **AT)
{
    if (AT) *AT = nullptr;
    if (!ctx || !A || !AT) return FAIL(BSPGEMM_ERR_INVALID, "matrix_transpose");
    if (bspgemm_status st = check_operand(ctx, A, "matrix_transpose", 0)) return st;
    if (A->nnz > kTrMaxNnz) return FAIL(BSPGEMM_ERR_OVERFLOW, "matrix_transpose: too many nonzeros for the int32 sort");
    if (bspgemm_status st = check_operand(ctx, A, "matrix_transpose", NEED_ENTRIES_CONSISTENT)) return st;
    if (bspgemm_status st = use_device(ctx)) return st;
    hipStream_t s = ctx->stream;
    const int E = (int)A->nnz, rows = A->rows, cols = A->cols;
    bspgemm_matrix *m = nullptr;
    auto bail = [&](bspgemm_status st) { hipStreamSynchronize(s); bspgemm_matrix_free(m); return st; };
    // col_idx sized for nnz(A): nnz(AT) (duplicates dropped) is known only at the end
    if (bspgemm_status st = operand_new(ctx, cols, rows, &m)) return bail(st);
    if (bspgemm_status st = operand_cols(m, E)) return bail(st);
    TrScalars h = {0, 0, 0};
    TrScalars *d_scal = nullptr;
    if (E == 0) {
        HIPCHK_B(hipMemsetAsync(m->d_row_ptr, 0, ((size_t)cols + 1) * sizeof(int), s));
    } else {
        const TrLayout lay = tr_layout(E, cols);
        const int bits = lay.bits, passes = lay.passes, ntiles = lay.ntiles, H = lay.H;
        const size_t E4 = lay.E4, o_hist = lay.o_hist, o_pre = lay.o_pre, o_part = lay.o_part, o_scal = lay.o_scal;
        if (bspgemm_status st = ensure_tmp(ctx, lay.total)) return bail(st);
        int *ws = ctx->tmp;
        int *kb[2] = {ws, ws + 2 * E4}, *vb[2] = {ws + E4, ws + 3 * E4};
        int *hist = ws + o_hist;
        long long *pre = reinterpret_cast<long long *>(ws + o_pre);
        long long *part = reinterpret_cast<long long *>(ws + o_part);
        d_scal = reinterpret_cast<TrScalars *>(ws + o_scal);
        unsigned *err = &d_scal->err;
        HIPCHK_B(hipMemsetAsync(d_scal, 0, sizeof(TrScalars), s));
        for (int p = 0; p < passes; p++) {
            const int shift = p * kDigitBits;
            const int nbits = min(kDigitBits, bits - shift);
            int *ko = kb[p & 1], *vo = vb[p & 1];
            if (p == 0) {
                hipLaunchKernelGGL(k_tr_hist<true>, dim3(ntiles), dim3(kTrThreads), 0, s, A->d_col_idx, E, cols, shift,
                                   nbits, ntiles, hist, err);
                launch_scan_counts(hist, H, pre, part, nullptr, s);
                hipLaunchKernelGGL(k_tr_scatter<true>, dim3(ntiles), dim3(kTrThreads), 0, s, A->d_col_idx,
                                   static_cast<const int *>(nullptr), A->d_row_ptr, rows, E, cols, shift, nbits, ntiles,
                                   pre, ko, vo);
            } else {
                const int *ki = kb[(p - 1) & 1], *vi = vb[(p - 1) & 1];
                hipLaunchKernelGGL(k_tr_hist<false>, dim3(ntiles), dim3(kTrThreads), 0, s, ki, E, cols, shift, nbits,
                                   ntiles, hist, err);
                launch_scan_counts(hist, H, pre, part, nullptr, s);
                hipLaunchKernelGGL(k_tr_scatter<false>, dim3(ntiles), dim3(kTrThreads), 0, s, ki, vi,
                                   static_cast<const int *>(nullptr), rows, E, cols, shift, nbits, ntiles, pre, ko, vo);
            }
        }
        const int *ks = kb[(passes - 1) & 1], *vs = vb[(passes - 1) & 1];
        hipLaunchKernelGGL(k_tr_dedup_count, dim3(ntiles), dim3(kTrThreads), 0, s, ks, vs, E, hist);
        launch_scan_counts(hist, ntiles, pre, part, nullptr, s);
        hipLaunchKernelGGL(k_tr_dedup_write, dim3(ntiles), dim3(kTrThreads), 0, s, ks, vs, E, cols, pre, ntiles,
                           m->d_col_idx, m->d_row_ptr, d_scal);
        HIPCHK_B(hipGetLastError());
    }
    if (bspgemm_status st = operand_finish(m, 0)) return bail(st);   // (nnz(AT) comes with the read-back below)
    if (d_scal) HIPCHK_B(hipMemcpyAsync(&h, d_scal, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK_B(hipStreamSynchronize(s));                      // the call's one synchronisation: nnz(AT) and the error word
    if (h.err) {
        snprintf(g_err, sizeof g_err, "matrix_transpose: a column index outside [0, %d) (A.cols)", cols);
        return bail(BSPGEMM_ERR_INVALID);
    }
    m->nnz = h.nnz;
    *AT = m;
    return BSPGEMM_OK;
}

bspgemm_status operand_canonical(bspgemm_context *ctx, const bspgemm_matrix *X, bspgemm_matrix **out)
{
    bspgemm_matrix *t = nullptr;
    bspgemm_status st = bspgemm_matrix_transpose(ctx, X, &t);
    if (!st) st = bspgemm_matrix_transpose(ctx, t, out);
    bspgemm_matrix_free(t);
    return st;
}
