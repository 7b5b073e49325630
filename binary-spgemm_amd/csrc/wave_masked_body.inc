// wave_masked_body.inc -- the body of the mask-first one-wave kernels, included inside k_wave_masked and
// k_wave_masked_count (wave_masked.hip), which provide LEVELS, CHUNKS, the arguments and COUNT (false: C = F .* (A*B), the
// kept bits of the mask row; true: the same pattern with the number of products of every kept column, written to `vals` at
// the column's offset in tmp).  A text body and not a __forceinline__ function, so that k_wave_masked compiles to the same
// code as before its twin existed (see wave_rows_body.inc).
    using Cfg = MaskCfg<LEVELS, CHUNKS, COUNT>;
    constexpr int CAP = Cfg::CAP, TOPW = Cfg::TOPW, WAVES = Cfg::WAVES, TW = TOPW / 64;
    constexpr int PCH = kMaskWinChunks;
    __shared__ __attribute__((aligned(16))) u32 s_top[WAVES][TOPW];
    __shared__ __attribute__((aligned(16))) unsigned short s_topPre[WAVES][TOPW];
    __shared__ __attribute__((aligned(16))) u64 s_starts[WAVES][PCH];
    __shared__ __attribute__((aligned(16))) int s_delta[WAVES][64];
    __shared__ __attribute__((aligned(16))) u32 s_SA[WAVES][CAP];           // level-0 masks of the MASK row
    constexpr int KN = (LEVELS == 1 && !COUNT) ? TOPW : CAP;       // level-0 slots: the top words themselves when LEVELS == 1
    __shared__ __attribute__((aligned(16))) u32 s_K0[WAVES][KN];            // kept bits (COUNT: staging of the counts)
    __shared__ __attribute__((aligned(16))) u32 s_L0w[WAVES][CAP];          // word id of every level-0 slot; emit staging
    __shared__ __attribute__((aligned(16))) u32 s_SB[WAVES][LEVELS >= 3 ? CAP : 4];
    __shared__ __attribute__((aligned(16))) unsigned short s_preB[WAVES][LEVELS >= 3 ? CAP : 8];
    __shared__ __attribute__((aligned(16))) u32 s_cnt[WAVES][COUNT ? CAP : 1];                          // COUNT: one counter per distinct mask column
    __shared__ __attribute__((aligned(16))) unsigned short s_pre0[WAVES][COUNT && LEVELS >= 2 ? CAP : 1]; // ... its rank base per level-0 word

    const int lane = lane_id();
    const int wave_in_wg = threadIdx.x >> 6;
    const long long wave_global = (long long)blockIdx.x * WAVES + wave_in_wg;
    const long long k0 = wave_global * kRowsPerWave;
    if (k0 >= nrows) return;                                       // wave-uniform; no barriers used
    const int nmine = (nrows - k0 < kRowsPerWave) ? (int)(nrows - k0) : kRowsPerWave;

    int r_row = 0, r_a0 = 0, r_alen = 0;
    long long r_pre = 0;
    if (lane < nmine) {
        const RowRec q = rec[k0 + lane];
        r_row = q.row;
        r_a0 = q.a0;
        r_alen = q.alen;
        r_pre = recpre[k0 + lane];
    }

    u32 *top = s_top[wave_in_wg];
    unsigned short *topPre = s_topPre[wave_in_wg];
    u64 *starts = s_starts[wave_in_wg];
    int *delta = s_delta[wave_in_wg];
    u32 *SA = s_SA[wave_in_wg], *K0 = s_K0[wave_in_wg], *L0w = s_L0w[wave_in_wg], *SB = s_SB[wave_in_wg];
    unsigned short *preB = s_preB[wave_in_wg];
    u32 *ccnt = s_cnt[wave_in_wg];
    unsigned short *pre0 = (LEVELS == 1) ? topPre : s_pre0[wave_in_wg];   // (LEVELS == 1 builds no topPre of its own)

    clear_blocked<TW>(top, lane);
    if (lane < PCH) starts[lane] = 0ull;
    clear_blocked<CHUNKS>(SA, lane);
    clear_blocked<KN / 64>(K0, lane);
    if (LEVELS >= 3) clear_blocked<CHUNKS>(SB, lane);
    wave_lds_fence();

    for (int kk = 0; kk < nmine; kk++) {
        const int i = wave_bcast(r_row, kk);
        const int a0 = wave_bcast(r_a0, kk);
        const int alen = wave_bcast(r_alen, kk);
        const u32 pre_lo = (u32)wave_bcast((int)(u32)r_pre, kk);
        const u32 pre_hi = (u32)wave_bcast((int)(u32)((unsigned long long)r_pre >> 32), kk);
        int *out = tmp + (long long)(((u64)pre_hi << 32) | pre_lo);
        const int f0 = Frow[i], mlen = Frow[i + 1] - f0;           // <= CAP by the row's class

        // ---- 1. rank bitmap of the mask row (all levels stay alive) ----------------------
        int mcol[CHUNKS], rank[CHUNKS];
        bool live[CHUNKS];                                         // COUNT: the lane's column of chunk c is a mask column
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            const int p = c * 64 + lane;
            mcol[c] = Fcol[f0 + (p < mlen ? p : 0)];
        }
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            // COUNT: a mask column beyond the top bitmap (at or above B.cols) is dropped here -- its top word would lie
            // outside s_top, and no product can land on it
            const bool ok = c * 64 + lane < mlen && (!COUNT || ((u32)mcol[c] >> (5 * LEVELS)) < (u32)topw);
            const u32 cc = ok ? (u32)mcol[c] : 0u;
            mcol[c] = (int)cc;
            const u32 tw = cc >> (5 * LEVELS);
            if (ok) atomicOr(&top[tw], 1u << ((cc >> (5 * (LEVELS - 1))) & 31));   // tail lanes masked off
            rank[c] = (int)tw;
            live[c] = ok;
        }
        wave_lds_fence();
        u32 *L0 = top;                      // level-0 masks of the mask row
        if (LEVELS >= 2) {
            scan_blocked<TW>(top, topPre, lane);
            wave_lds_fence();
            const u32 *P = top;
            const unsigned short *Ppre = topPre;
#pragma unroll
            for (int lev = LEVELS - 2; lev >= 0; lev--) {
                u32 *S = (lev == 1) ? SB : SA;
                unsigned short *Spre = preB;                       // only level 1 needs ranks
#pragma unroll
                for (int c = 0; c < CHUNKS; c++) {
                    const bool ok = c * 64 + lane < mlen && (!COUNT || live[c]);
                    const u32 cc = (u32)mcol[c];
                    const u32 x = P[rank[c]];
                    const int pre = Ppre[rank[c]];
                    const u32 b = (cc >> (5 * (lev + 1))) & 31;
                    const int r2 = pre + __popc(x & ((1u << b) - 1u));
                    if (ok) {
                        atomicOr(&S[r2], 1u << ((cc >> (5 * lev)) & 31));
                        if (lev == 0) L0w[r2] = cc >> 5;
                    }
                    rank[c] = r2;
                }
                wave_lds_fence();
                if (lev > 0) {
                    scan_blocked<CHUNKS>(S, Spre, lane);
                    wave_lds_fence();
                    P = S;
                    Ppre = Spre;
                }
            }
            L0 = SA;
        }
        if constexpr (COUNT) {
            // a distinct mask column's counter is its rank in the row: pre0[level-0 word] + the word's bits below it.
            // Only the row's distinct columns are cleared.
            constexpr int NW0 = (LEVELS == 1) ? TW : CHUNKS;
            const int ndist = scan_blocked<NW0>(L0, pre0, lane);
            for (int t = lane; t < ndist; t += 64) ccnt[t] = 0u;
            wave_lds_fence();
        }

        // ---- 2. stream the row's products through the structure, read-only ---------------
        for (int ab0 = 0; ab0 < alen; ab0 += 64) {
            int2 e = make_int2(0, 0);
            if (ab0 + lane < alen) e = ab[a0 + ab0 + lane];
            const int bs = e.x, len = e.y;
            const int inc = wave_incl_scan(len);
            const int excl = inc - len;
            const int Fb = wave_bcast(inc, 63);                    // products of this batch of 64 sources
            for (int w0 = 0; w0 < Fb; w0 += 64 * PCH) {
                // sources that own products inside the window [w0, w0 + 256)
                const bool part = len > 0 && excl < w0 + 64 * PCH && excl + len > w0;
                const u64 bal = __ballot(part);
                if (part) {
                    const int sidx = __popcll(bal & mask_lt(lane));
                    const int pos = (excl > w0 ? excl : w0) - w0;
                    delta[sidx] = bs - excl;                       // B address = delta + batch product index
                    atomicOr(&starts[pos >> 6], 1ull << (pos & 63));
                }
                wave_lds_fence();
                u64 sw = 0ull;
                if (lane < PCH) { sw = starts[lane]; starts[lane] = 0ull; }
                const int sinc = wave_incl_scan(__popcll(sw));
                const int sbefore = sinc - __popcll(sw);
                int gaddr[PCH];
#pragma unroll
                for (int c = 0; c < PCH; c++) {
                    const int p = c * 64 + lane;
                    const u64 M = wave_bcast64(sw, c);
                    const int before = wave_bcast(sbefore, c);
                    const bool ok = w0 + p < Fb;
                    int s = before + __popcll(M & mask_le(lane)) - 1;
                    s = ok ? s : 0;
                    gaddr[c] = ok ? delta[s] + w0 + p : 0;          // tail lanes: Bcol[0]
                }
                int pc[PCH];
#pragma unroll
                for (int c = 0; c < PCH; c++) {
                    const bool ok = w0 + c * 64 + lane < Fb;
                    pc[c] = ok ? Bcol[gaddr[c]] : -1;
                }
                wave_lds_fence();
                // probe: follow the digit path; mark the kept bit when every level has it
#pragma unroll
                for (int c = 0; c < PCH; c++) {
                    const bool ok = pc[c] >= 0;
                    const u32 cc = ok ? (u32)pc[c] : 0u;
                    const u32 tw = cc >> (5 * LEVELS);
                    bool hit = ok && tw < (u32)topw;
                    u32 x = top[hit ? tw : 0];
                    int r = (int)(hit ? tw : 0);
                    if (LEVELS >= 2) {
                        const u32 b = (cc >> (5 * (LEVELS - 1))) & 31;
                        hit = hit && ((x >> b) & 1u);
                        r = topPre[r] + __popc(x & ((1u << b) - 1u));
                        r = hit ? r : 0;
                        if (LEVELS >= 3) {
                            x = SB[r];
                            const u32 b1 = (cc >> 5) & 31;
                            hit = hit && ((x >> b1) & 1u);
                            r = preB[r] + __popc(x & ((1u << b1) - 1u));
                            r = hit ? r : 0;
                        }
                        x = SA[r];
                    }
                    const u32 b0 = cc & 31;
                    hit = hit && ((x >> b0) & 1u);
                    if constexpr (COUNT) {
                        // a hit adds one to its column's counter; the kept bits follow from the counters (step 3)
                        if (hit) atomicAdd(&ccnt[pre0[r] + __popc(x & ((1u << b0) - 1u))], 1u);
                    } else {
                        // only the hits touch K0: parking the misses (the vast majority of a sparse
                        // masked product) on one spare word serialises them as same-address atomics
                        if (hit) atomicOr(&K0[r], 1u << b0);
                    }
                }
                wave_lds_fence();
            }
        }

        // ---- 3. emit the kept bits in rank order; clear everything for the next row ------
        constexpr int W0 = (LEVELS == 1) ? TW : CHUNKS;
        if constexpr (COUNT) {
            // the mask row's columns in rank order, each with its counter: the non-zero ones are emitted with their counts
            // (columns staged in L0w, counts in K0), at the same offsets in tmp and vals
            u32 m[W0], wv[W0];
#pragma unroll
            for (int k = 0; k < W0; k++) {
                m[k] = L0[lane * W0 + k];
                wv[k] = (LEVELS == 1) ? (u32)(lane * W0 + k) : L0w[lane * W0 + k];
            }
            const int c0 = pre0[lane * W0];                        // the lane's words own the counters c0, c0 + 1, ...
            clear_blocked<W0>(L0, lane);
            if (LEVELS >= 2) clear_blocked<TW>(top, lane);
            if (LEVELS >= 3) clear_blocked<CHUNKS>(SB, lane);
            int nmask = 0;
#pragma unroll
            for (int k = 0; k < W0; k++) nmask += __popc(m[k]);
            int mine = 0;
            for (int t = 0; t < nmask; t++) mine += ccnt[c0 + t] != 0u ? 1 : 0;
            const int inc = wave_incl_scan(mine);
            const int running = wave_bcast(inc, 63);
            wave_lds_fence();
            {
                int pos = inc - mine, c = c0;
#pragma unroll
                for (int k = 0; k < W0; k++) {
                    u32 mk = m[k];
                    const u32 base = wv[k] << 5;
                    while (mk) {
                        const u32 v = ccnt[c++];
                        if (v) {
                            L0w[stage_swz(pos)] = base | (u32)__builtin_ctz(mk);
                            K0[stage_swz(pos)] = v;
                            pos++;
                        }
                        mk &= mk - 1u;
                    }
                }
            }
            wave_lds_fence();
            int *vout = vals + (out - tmp);
            for (int t = lane; t < running; t += 64) {
                __builtin_nontemporal_store((int)L0w[stage_swz(t)], out + t);
                __builtin_nontemporal_store((int)K0[stage_swz(t)], vout + t);
            }
            if (lane == 0) cnt[i - row_begin] = running;
            wave_lds_fence();
            continue;
        }
        u32 m[W0], wv[W0];
#pragma unroll
        for (int k = 0; k < W0; k++) {
            m[k] = K0[lane * W0 + k];
            wv[k] = (LEVELS == 1) ? (u32)(lane * W0 + k) : L0w[lane * W0 + k];
        }
        clear_blocked<W0>(K0, lane);
        clear_blocked<W0>(L0, lane);
        if (LEVELS >= 2) clear_blocked<TW>(top, lane);
        if (LEVELS >= 3) clear_blocked<CHUNKS>(SB, lane);
        int mine = 0;
#pragma unroll
        for (int k = 0; k < W0; k++) mine += __popc(m[k]);
        const int inc = wave_incl_scan(mine);
        const int running = wave_bcast(inc, 63);
        wave_lds_fence();
        {
            int pos = inc - mine;
#pragma unroll
            for (int k = 0; k < W0; k++) {
                u32 mk = m[k];
                const u32 base = wv[k] << 5;
                while (mk) {
                    L0w[stage_swz(pos)] = base | (u32)__builtin_ctz(mk);
                    pos++;
                    mk &= mk - 1u;
                }
            }
        }
        wave_lds_fence();
        for (int t = lane; t < running; t += 64) __builtin_nontemporal_store((int)L0w[stage_swz(t)], out + t);   // streamed, as in wave_rows.inc
        if (lane == 0) cnt[i - row_begin] = running;
        wave_lds_fence();
    }
