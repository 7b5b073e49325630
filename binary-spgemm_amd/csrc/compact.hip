// compact.hip -- moving finished rows: the compaction that squeezes the upper-bound-placed rows into C.col_idx (k_compact),
// the exact flow's move of the heavy rows to their final place (k_place_heavy) and the hub rows' launch order (k_order_heavy).
#include "kernels.hpp"
#include "wave.hpp"

namespace bsp {

struct __attribute__((packed, aligned(4))) Int4U { int x, y, z, w; };   // 16 B, only dword aligned

// Hub rows in order of decreasing products (longest processing time first): one workgroup per row, one per
// CU, dispatched in list order -- in row order the largest row (it alone is most of the class's critical
// path: 2 M products on one CU) may start last.  n <= kHeavySortMax: ranks by counting, each thread its own.
__global__ __launch_bounds__(256) void k_order_heavy(const RowRec *__restrict__ rec, const long long *__restrict__ recpre,
                                                     int n, RowRec *__restrict__ rec_out, long long *__restrict__ pre_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RowRec me = rec[i];
    int rank = 0;
    for (int j = 0; j < n; j++) {
        const int f = rec[j].f;
        rank += (f > me.f || (f == me.f && j < i)) ? 1 : 0;
    }
    rec_out[rank] = me;
    pre_out[rank] = recpre[i];
}
void launch_order_heavy(const RowRec *rec, const long long *recpre, int n, RowRec *rec_out, long long *pre_out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_order_heavy, dim3((n + 255) / 256), dim3(256), 0, s, rec, recpre, n, rec_out, pre_out);
}

// ---------------------------------------------------------------------------------------
// Exact flow: heavy rows keep the upper-bound placement -- k_dense_rows accumulates AND reads out in the
// symbolic phase (its window bitmap is the expensive part; counting alone would cost almost the same), into
// a workspace sized by sum(min(F_i, cols)) over the heavy rows only, and this kernel moves each
// heavy row to its final place once C.row_ptr exists.  One workgroup per heavy row.
__global__ __launch_bounds__(256) void k_place_heavy(const int *__restrict__ tmp, const RowRec *__restrict__ rec,
                                                     const long long *__restrict__ recpre,
                                                     const long long *__restrict__ row_ptr, int row_begin,
                                                     int *__restrict__ col_idx)
{
    const RowRec q = rec[blockIdx.x];
    const int i = q.row - row_begin;
    const long long d0 = row_ptr[i];
    const int n = (int)(row_ptr[i + 1] - d0);
    const int *src = tmp + recpre[blockIdx.x];
    int *dst = col_idx + d0;
    for (int t = threadIdx.x; t < n; t += 256) dst[t] = src[t];
}

void launch_place_heavy(const int *tmp, const RowRec *rec, const long long *recpre, int nrows,
                        const long long *row_ptr, int row_begin, int *col_idx, hipStream_t s)
{
    if (nrows <= 0) return;
    hipLaunchKernelGGL(k_place_heavy, dim3(nrows), dim3(256), 0, s, tmp, rec, recpre, row_ptr, row_begin, col_idx);
}

// ---------------------------------------------------------------------------------------
// Compaction: every row was written at its upper-bound offset Fprefix[r]; now that the counts
// are scanned into C.row_ptr the rows are copied to their final place.  Pure streaming copy
// (4 B read + 4 B written per output nonzero), driven by the DESTINATION: a workgroup owns
// 4096 consecutive output nonzeros (16 KiB of C.col_idx), takes the rows that cover them from the
// table the count scan left (chunk_row: the row of every 4096th output; without the table -- small
// products -- 32768 outputs or fewer and a binary search in C.row_ptr), keeps their (row_ptr, shift) pairs in LDS 256 rows at a time and
// copies 16 B per lane whenever four outputs lie in one row -- stores are always 16-B aligned
// and fully coalesced, loads are the same stream displaced by the row's shift.  Work per
// workgroup is fixed whatever the row lengths (hub rows and empty rows cost nothing extra).
constexpr int kCompactChunk = 32768;     // output nonzeros per workgroup when its rows are searched (a small product gets smaller chunks: see launch_compact)
constexpr int kCompactChunkTable = 4096; // ... when the count scan left the row table (chunk_row): a multiple of kCompactGran
static_assert(kCompactChunkTable % kCompactGran == 0, "chunk starts must be entries of the row table");
constexpr int kCompactBatch = 256;       // rows staged in LDS at a time
constexpr int kCompactInFlight = 4;      // 16-B groups a thread has in flight (8 measured slower)
constexpr int kCompactSparseRows = 4096; // a chunk spanning more rows than this is searched per output

typedef int v4i __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_compact(const int *__restrict__ tmp,
                                                 const long long *__restrict__ Fprefix,
                                                 const long long *__restrict__ row_ptr,
                                                 int row_lo, int row_hi, int chunk, int *__restrict__ col_idx,
                                                 const int *__restrict__ chunk_row)
{
    __shared__ long long rp[kCompactBatch + 1];
    __shared__ long long sh[kCompactBatch];      // source offset - destination offset of the row
    __shared__ int r_first, r_last;
    const int tid = threadIdx.x;
    const long long out_lo = row_ptr[row_lo], out_hi = row_ptr[row_hi];
    // chunk starts are multiples of 4 outputs so that the 16-B stores stay aligned
    long long o0 = (out_lo & ~3ll) + (long long)blockIdx.x * chunk;
    long long o1 = o0 + chunk;
    if (o0 < out_lo) o0 = out_lo;
    if (o1 > out_hi) o1 = out_hi;
    if (o0 >= o1) return;                        // uniform: the grid is sized by an upper bound
    int rf, rl;                                  // first / last row with outputs in the chunk (rl may be one row further)
    if (chunk_row) {
        // the count scan left the row of every kCompactGran-th output (the chunk is a multiple of that, row_lo == 0):
        // two loads at uniform addresses, no search, no barrier
        rf = chunk_row[o0 / kCompactGran];
        rl = chunk_row[(o1 + kCompactGran - 1) / kCompactGran];       // row of output o1, or of the last output
    } else {
        if (tid == 0) {
            // last row r in [row_lo,row_hi) with row_ptr[r] <= o0: non-empty and contains output o0
            int lo = row_lo, hi = row_hi;            // invariant: row_ptr[lo] <= o0 < row_ptr[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (row_ptr[mid] <= o0) lo = mid; else hi = mid;
            }
            r_first = lo;
            // ... and the row that holds the chunk's last output
            lo = r_first, hi = row_hi;               // invariant: row_ptr[lo] <= o1 - 1 < row_ptr[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (row_ptr[mid] <= o1 - 1) lo = mid; else hi = mid;
            }
            r_last = lo;
        }
        __syncthreads();
        rf = r_first;
        rl = r_last;
    }
    if (chunk_row) {
        // Nearly every chunk of a product with few repeated columns has ONE shift (98 % of the bench matrix's rows have no hole
        // behind them; a row's shift is the holes before it, so first == last means all the same): a plain displaced copy, no row
        // staging, no search, no barrier.  (rl may be the row after the chunk's last: then a hole in between only sends the chunk
        // down the general path.)
        const long long sf = Fprefix[rf] - row_ptr[rf], sl = Fprefix[rl] - row_ptr[rl];
        if (sf == sl) {                              // (uniform)
            const int *__restrict__ src = tmp + sf;
            const int n = (int)(o1 - o0);
            constexpr int kU = 4;
            for (int g0 = tid; 4 * g0 < n; g0 += 256 * kU) {
                Int4U v[kU];
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    const int e = 4 * (g0 + 256 * u);
                    if (e + 3 < n) {                                                          // source only dword aligned
                        const int *q = src + o0 + e;
                        v[u].x = __builtin_nontemporal_load(q), v[u].y = __builtin_nontemporal_load(q + 1);
                        v[u].z = __builtin_nontemporal_load(q + 2), v[u].w = __builtin_nontemporal_load(q + 3);
                    }
                }
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    const int e = 4 * (g0 + 256 * u);
                    if (e + 3 < n) {
                        const v4i w4 = {v[u].x, v[u].y, v[u].z, v[u].w};
                        __builtin_nontemporal_store(w4, reinterpret_cast<v4i *>(col_idx + o0 + e));
                    } else {
                        for (int k = e; k < n; k++) col_idx[o0 + k] = src[o0 + k];             // the product's last outputs
                    }
                }
            }
            return;
        }
    }
    if (rl - rf > kCompactSparseRows) {
        // Mostly empty rows (a masked product, a very sparse result): staging every row of the span
        // through LDS would walk millions of empty rows in ONE workgroup.  Search per output instead.
        for (long long o = o0 + tid; o < o1; o += 256) {
            int lo = rf, hi = rl + 1;            // row_ptr[lo] <= o < row_ptr[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (row_ptr[mid] <= o) lo = mid; else hi = mid;
            }
            col_idx[o] = tmp[Fprefix[lo] + (o - row_ptr[lo])];
        }
        return;
    }
    // From here on positions are ints RELATIVE to the chunk's (unclipped, 16-B aligned) start: row starts are clamped to
    // [0, chunk] (a row that begins before the chunk compares like 0, one that begins after it like `chunk`), the row's
    // shift carries the chunk start, so that a group's source is one 64-bit add.
    const long long obase = (out_lo & ~3ll) + (long long)blockIdx.x * chunk;
    const int o0r = (int)(o0 - obase), o1r = (int)(o1 - obase);
    int *rpr = reinterpret_cast<int *>(rp);      // rp's storage, as ints
    int *__restrict__ dst = col_idx + obase;
    int rbase = rf;
    while (true) {
        // rows staged: up to the chunk's last row (row_ptr[rl + 1] >= o1 ends the loop below), a batch at a time
        const int nb = (rl + 1 - rbase < kCompactBatch) ? rl + 1 - rbase : kCompactBatch;
        __syncthreads();
        for (int t = tid; t <= nb; t += 256) {                   // both loads of a row in one round trip
            const long long start = row_ptr[rbase + t];
            const long long rel = start - obase;
            rpr[t] = rel < 0 ? 0 : (rel > chunk ? chunk : (int)rel);
            if (t < nb) sh[t] = Fprefix[rbase + t] - start + obase;
        }
        __syncthreads();
        const int b0 = rpr[0] > o0r ? rpr[0] : o0r;            // outputs covered by this batch and chunk
        const int b1 = rpr[nb] < o1r ? rpr[nb] : o1r;
        // kCompactInFlight 16-B groups per thread per step: independent row searches and loads in flight
        for (int g0 = (b0 >> 2) + tid; (g0 << 2) < b1; g0 += 256 * kCompactInFlight) {
            int o[kCompactInFlight], lo_r[kCompactInFlight];
            long long src[kCompactInFlight];
            bool fast[kCompactInFlight], live[kCompactInFlight];
#pragma unroll
            for (int u = 0; u < kCompactInFlight; u++) {
                o[u] = (g0 + u * 256) << 2;
                live[u] = o[u] < b1;
                const int oo = !live[u] ? b0 : (o[u] > b0 ? o[u] : b0);
                int lo = 0, hi = nb;             // rpr[lo] <= oo < rpr[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (rpr[mid] <= oo) lo = mid; else hi = mid;
                }
                lo_r[u] = lo;
                fast[u] = live[u] && o[u] >= b0 && o[u] + 3 < b1 && o[u] + 3 < rpr[lo + 1];
                src[u] = o[u] + sh[lo];
            }
            Int4U v[kCompactInFlight];
#pragma unroll
            for (int u = 0; u < kCompactInFlight; u++)
                if (fast[u]) v[u] = *reinterpret_cast<const Int4U *>(tmp + src[u]);     // source only dword aligned
#pragma unroll
            for (int u = 0; u < kCompactInFlight; u++) {
                if (fast[u]) {
                    const v4i w4 = {v[u].x, v[u].y, v[u].z, v[u].w};
                    __builtin_nontemporal_store(w4, reinterpret_cast<v4i *>(dst + o[u]));
                } else if (live[u]) {
                    // a group that straddles rows (or the batch / chunk end): its outputs one by one -- the four loads
                    // first, then the stores (one round trip: nearly every wave has such a group)
                    int r = lo_r[u];
                    int val[4];
                    bool has[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int oe = o[u] + e;
                        has[e] = oe >= b0 && oe < b1;
                        if (has[e]) {
                            while (rpr[r + 1] <= oe) r++;
                            val[e] = tmp[oe + sh[r]];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (has[e]) dst[o[u] + e] = val[e];
                }
            }
        }
        if (rpr[nb] >= o1r || rbase + nb >= row_hi) break;     // uniform: every thread reads the same LDS
        rbase += nb;
    }
}

void launch_compact(const int *tmp, const long long *Fprefix, const long long *row_ptr,
                    int row_lo, int row_hi, long long max_out, int *col_idx, hipStream_t s, const int *chunk_row)
{
    if (row_hi <= row_lo || max_out <= 0) return;
    // chunk: a multiple of 4 outputs (aligned 16-B stores).  With the scan's row table a workgroup's set-up is two
    // loads instead of two binary searches in C.row_ptr, and smaller chunks pay (stitch phase on the bench matrix:
    // 2.35 ms searched at 32768 outputs per workgroup; with the table 2.24 at 32768, 2.18 at 16384, 2.16 at 8192; with
    // the lighter prologue of the final kernel 2.10 at 8192 and 2.11 at 4096, power-law 2.85 -> 2.69 -> 2.43:
    // `profiles/r03_ab_compaction.log`): 4096 outputs (16 KiB).  A small product is
    // cut finer still so that it spreads over the chip (one large chunk would be ONE workgroup walking every row);
    // those chunks are not multiples of the table's grain and are searched.
    long long chunk = ((max_out / 2048) + 3) & ~3ll;
    if (chunk < 256) chunk = 256;
    if (chunk >= kCompactChunkTable && chunk_row && row_lo == 0) {
        chunk = kCompactChunkTable;
    } else {
        chunk_row = nullptr;
        if (chunk > kCompactChunk) chunk = kCompactChunk;
    }
    const int grid = (int)((max_out + 3 + chunk - 1) / chunk) + 1;
    hipLaunchKernelGGL(k_compact, dim3(grid), dim3(256), 0, s, tmp, Fprefix, row_ptr, row_lo, row_hi, (int)chunk, col_idx, chunk_row);
}

}  // namespace bsp
