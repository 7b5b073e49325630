// heavy_gather.hpp -- the gather of the heavy rows (F_i > 2048 products, one workgroup per A-row), shared by the window
// kernels and the rank kernels (dense_rows.hip).  Device code only.
//
//   gather_sweep   the row's A-nonzeros one per thread; their B-row extents (left by the prepass) are scanned into QUAD offsets -- a
//                  quad is four consecutive entries of one B row, one 16-byte load -- and the quads are spread evenly over the
//                  threads in tiles: thread t takes quads t, t+T, ... and finds each one's source row by rank in a per-tile "starts"
//                  bitmap (the wave kernels' gather plan at workgroup scope), whatever the B-row lengths are.
//   insert_quad    one quad into an LDS bitmap, one atomic per word touched.
#pragma once
#include "kernels.hpp"
#include "wave.hpp"
#include <type_traits>

namespace bsp {

struct __attribute__((packed, aligned(4))) Int4U { int x, y, z, w; };   // 16 B, only dword aligned
struct __attribute__((packed, aligned(4))) Int2U { int x, y; };

// ---------------------------------------------------------------------------------------
// One sweep over all the products
// of the row, `ins(quad, valid lanes)` called once per quad.
//
// One source (A-nonzero) per thread, kThreads at a time (a "batch").  The unit is the QUAD: four consecutive entries
// of one B row, one 16-byte load.  A block scan of the sources' quad counts gives every source its place in the batch's
// quad order; the non-empty sources are squeezed into a list of (B address - 4 * first quad, B end).  The quads are
// taken in TILES of kThreads * kQPT: a "starts" bitmap over the tile marks where each source begins, one wave turns its
// words into running source counts, and quad t finds its source by rank -- word, count, popcount: two independent LDS
// reads and a dependent one, the same for B rows of 3 and of 30000 entries -- so that every thread keeps kInFlight
// 16-byte loads in the air.  (Rounds 1-3 looked up every PRODUCT this way, three LDS reads and one 4-byte load each;
// the heavy classes were bound by exactly those, not by memory: profiles/r04_heavy_ablation.log.)
// The last quad of a source is the four entries that END at the row's end: it overlaps the quad before it (the
// accumulators are sets: inserting a column twice is harmless) and for a source of one to three entries it begins
// before the source -- those lanes are masked.  No load ever passes the end of B.col_idx.
// A row of one batch and one tile KEEPS its plan (sd, tw, tpre in LDS) for the later sweeps: they then start at the
// loads -- no extents, no block scan, no tile bitmap, none of their barriers (each of these phases is a latency the
// row's few waves cannot hide).
struct GatherState {
    long long QB = 0;            // quads of the batch
    bool plan_kept = false;      // uniform
    int buf = 0;                 // which of tw / tpre the current tile reads
};

template <int kThreads, int kQPT>
struct GatherLds {
    static constexpr int kWaves = kThreads / 64;
    static constexpr int kTileQ = kThreads * kQPT;                 // quads per tile
    static constexpr int kTileWords = kTileQ / 32;
    static_assert(kTileWords % 64 == 0 && kTileWords <= kThreads, "one wave scans the tile's words, blocked");
    int wcnt[kWaves];
    long long wsum[kWaves];
    int2 sd[kThreads];            // non-empty sources of the batch: (B address - 4 * first quad, B end address)
    u32 tb[kTileWords];           // starts of the sources inside the tile being planned (all zero between tiles)
    u32 tw[2][kTileWords];        // ... as the gather reads them: two tiles, so that the next plan never waits for the slowest gather
    int tpre[2][kTileWords];      // (sources begun before word w) - 1
};

// before the kernel's first barrier
template <int kThreads, int kQPT>
__device__ __forceinline__ void gather_init(GatherLds<kThreads, kQPT> &L)
{
    if ((int)threadIdx.x < GatherLds<kThreads, kQPT>::kTileWords) L.tb[threadIdx.x] = 0u;
}

template <int kThreads, int kQPT, int kInFlight, typename Ins>
__device__ __forceinline__ void gather_sweep(GatherLds<kThreads, kQPT> &L, GatherState &g, const int2 *__restrict__ ab,
                                             const int *__restrict__ Bcol, int nnzB, int a0, int a1, bool first_sweep, Ins ins)
{
    using LT = GatherLds<kThreads, kQPT>;
    constexpr int kWaves = LT::kWaves, kTileQ = LT::kTileQ, kTileWords = LT::kTileWords;
    static_assert(kQPT % kInFlight == 0 && kInFlight % 4 == 0, "whole steps; the last step in quarters");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (a row of several batches -- a hub row has thousands of sources -- loads the extents of batch j+1 while batch j is
    // gathered: one trip to memory less per batch on the row's critical path, and a hub row has the CU to itself)
    int2 e_next = make_int2(0, 0);
    if (!g.plan_kept && a0 + tid < a1) e_next = ab[a0 + tid];
    for (int ja = a0; ja < a1; ja += kThreads) {
        int2 e = make_int2(0, 0);
        int nq = 0, cidx = 0;
        long long qexcl = 0;
        if (!g.plan_kept) {
            e = e_next;
            e_next = make_int2(0, 0);
            if (ja + kThreads + tid < a1) e_next = ab[ja + kThreads + tid];
            nq = (int)(((u32)e.y + 3u) >> 2);
            const int inc = wave_incl_scan(nq);
            const u64 nonempty = __ballot(nq > 0);
            if (lane == 63) L.wsum[wave] = (long long)inc;
            if (lane == 0) L.wcnt[wave] = __popcll(nonempty);
            __syncthreads();
            qexcl = (long long)(inc - nq);
            g.QB = 0;
            cidx = __popcll(nonempty & mask_lt(lane));
            for (int k = 0; k < kWaves; k++) {
                const long long t = L.wsum[k];
                const int c = L.wcnt[k];
                if (k < wave) { qexcl += t; cidx += c; }
                g.QB += t;
            }
            if (nq > 0) L.sd[cidx] = make_int2((int)((u32)e.x - 4u * (u32)qexcl), e.x + e.y);   // (mod 2^32: the sum is a B address again)
            if (g.QB == 0) __syncthreads();                        // (no tile: nothing else orders this batch's wsum reads before the next batch's writes)
        }
        int carry = -1;                                            // wave 0: (sources begun before the tile) - 1
        for (long long T0 = 0; T0 < g.QB; T0 += kTileQ) {
            if (!g.plan_kept) {
                g.buf ^= 1;
                if (nq > 0 && qexcl >= T0 && qexcl < T0 + kTileQ) {    // the source begins in this tile
                    const int rel = (int)(qexcl - T0);
                    atomicOr(&L.tb[rel >> 5], 1u << (rel & 31));
                }
                __syncthreads();
                if (wave == 0) {
                    constexpr int WPL = kTileWords / 64;               // words per lane, blocked
                    u32 x[WPL];
                    int c[WPL], run = 0;
#pragma unroll
                    for (int k = 0; k < WPL; k++) {
                        x[k] = L.tb[lane * WPL + k];
                        L.tb[lane * WPL + k] = 0u;
                        c[k] = run;
                        run += __popc(x[k]);
                    }
                    const int wi = wave_incl_scan(run);
#pragma unroll
                    for (int k = 0; k < WPL; k++) {
                        L.tw[g.buf][lane * WPL + k] = x[k];
                        L.tpre[g.buf][lane * WPL + k] = carry + wi - run + c[k];
                    }
                    carry += wave_bcast(wi, 63);
                }
                __syncthreads();
            }
            const int nqt = (g.QB - T0 < kTileQ) ? (int)(g.QB - T0) : kTileQ;
            const u32 *twb = L.tw[g.buf];
            const int *tpb = L.tpre[g.buf];
            const u32 T0lo = 4u * (u32)T0;
            // a step takes kInFlight quads per thread; the LAST step of a tile is specialised for the number of slots that still
            // hold quads for anybody (workgroup-uniform): it is half empty on average, and a row of 3 K products fills 750 of a
            // step's 2048 quads -- the empty slots used to cost their look-ups and inserts all the same
            auto step = [&](int k0, auto nu_c) {
                constexpr int NU = decltype(nu_c)::value;
                int base[NU];
                u32 vmask[NU];                                     // lanes of the quad that are entries of this source not yet taken
#pragma unroll
                for (int u = 0; u < NU; u++) {
                    const int t = k0 + u * kThreads + tid;
                    const bool ok = t < nqt;
                    const int tt = ok ? t : 0;
                    const u32 w = twb[tt >> 5];
                    const int src = tpb[tt >> 5] + __popc(w & ((2u << (tt & 31)) - 1u));
                    const int2 sq = L.sd[src < 0 ? 0 : src];
                    const int qs = (int)((u32)sq.x + T0lo + 4u * (u32)tt);   // first entry of the quad
                    int b = qs < sq.y - 4 ? qs : sq.y - 4;
                    b = b < 0 ? 0 : b;
                    base[u] = b;
                    u32 m = 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++) m |= (ok && b + k >= qs && b + k < sq.y) ? (1u << k) : 0u;
                    vmask[u] = m;
                }
                Int4U cv[NU];
#pragma unroll
                for (int u = 0; u < NU; u++) {
                    if (nnzB >= 4) {                               // (uniform)
                        cv[u] = *reinterpret_cast<const Int4U *>(Bcol + base[u]);      // only dword aligned
                    } else {                                       // a B.col_idx of one to three entries (never the padded copy: 16+): base is 0, no vector load fits
                        cv[u].x = Bcol[0];
                        cv[u].y = nnzB > 1 ? Bcol[1] : 0;
                        cv[u].z = nnzB > 2 ? Bcol[2] : 0;
                        cv[u].w = 0;
                    }
                }
#pragma unroll
                for (int u = 0; u < NU; u++) ins(cv[u], vmask[u], u);
            };
            for (int k0 = 0; k0 < nqt; k0 += kInFlight * kThreads) {
                const int left = nqt - k0;                         // (uniform)
                if (left > (3 * kInFlight / 4) * kThreads) step(k0, std::integral_constant<int, kInFlight>());
                else if (left > (kInFlight / 2) * kThreads) step(k0, std::integral_constant<int, 3 * kInFlight / 4>());
                else if (left > (kInFlight / 4) * kThreads) step(k0, std::integral_constant<int, kInFlight / 2>());
                else step(k0, std::integral_constant<int, kInFlight / 4>());
            }
        }
        __syncthreads();
    }
    if (first_sweep) g.plan_kept = (a1 - a0 <= kThreads) && g.QB <= kTileQ && g.QB > 0;
}

// One quad into a bitmap: entry k goes to bit b_k of word w_k when i_k.  The quad's columns ascend, so the entries of one
// word are neighbours, and the first of each run ORs the whole run -- one LDS atomic per word touched instead of one per
// product (the dense heads of hub B rows put up to 32 lanes' products into ONE word: same-address atomics serialise).
// Correct for any order (an unsorted B row only merges less).
// `windowed`: the entries are filtered by a column window, and a wave whose 64 quads all miss it leaves at once.
__device__ __forceinline__ void insert_quad(u32 *tgt, bool i0, bool i1, bool i2, bool i3, u32 w0, u32 w1, u32 w2, u32 w3,
                                            u32 b0, u32 b1, u32 b2, u32 b3, bool windowed = false)
{
    if (windowed && !__ballot(i0 | i1 | i2 | i3)) return;          // (wave-uniform) nothing of these 64 quads falls into the window
    w0 = i0 ? w0 : 0xfffffff0u, w1 = i1 ? w1 : 0xfffffff1u, w2 = i2 ? w2 : 0xfffffff2u, w3 = i3 ? w3 : 0xfffffff3u;
    const u32 m2 = b2 | (w3 == w2 ? b3 : 0u);
    const u32 m1 = b1 | (w2 == w1 ? m2 : 0u);
    const u32 m0 = b0 | (w1 == w0 ? m1 : 0u);
    if (i0) atomicOr(&tgt[w0], m0);
    if (i1 && w1 != w0) atomicOr(&tgt[w1], m1);
    if (i2 && w2 != w1) atomicOr(&tgt[w2], m2);
    if (i3 && w3 != w2) atomicOr(&tgt[w3], b3);
}

}  // namespace bsp
