// wave_rows_body.inc -- the body of the one-wave kernels, included inside k_wave_rows, k_wave_rows_excl and k_wave_rows_acc
// (wave_rows.inc).  The including kernel provides the template parameters LEVELS, CHUNKS, TWP, the arguments ab, Bcol, rec,
// recpre, row_ptr, nrows, rpw, row_begin, tmp, cnt, err, Frow, Fcol, cols, and the constants COUNT (symbolic twin), EXCL
// (complemented-mask twin: F's columns are dropped from each staged row before it is stored, drop_mask_cols) and ACC
// (accumulate twin: the row of D -- passed as Frow / Fcol -- is one more source of the gather, read from Fcol; its columns
// outside [0, cols) lose their valid bit).  A text body and not a
// __forceinline__ function: with a function the compiler schedules the existing instances differently (1-2 more VGPRs on
// half of them); included, k_wave_rows compiles to the same code as before the twin existed.
// The gather's load and the sweeps' product test are macros the including kernel defines (BSP_WAVE_GATHER(c, g),
// BSP_WAVE_OK(x, c)), so that k_wave_rows and k_wave_rows_excl see the very same tokens as before the accumulate twin
// (written as `(x) && (!ACC || ...)`, the test changed their schedule); they are undefined at the end.
    using Cfg = WaveCfg<LEVELS, CHUNKS, TWP>;
    constexpr int TOPW = Cfg::TOPW, WAVES = Cfg::WAVES, SW = Cfg::SW, SLOTS = Cfg::SLOTS, FULL = Cfg::FULL;
    // separate objects: no false LDS dependencies between the arrays of one sweep
    __shared__ __attribute__((aligned(16))) u32 s_top[WAVES][TOPW];
    __shared__ __attribute__((aligned(16))) unsigned short s_topPre[WAVES][TOPW];
    __shared__ __attribute__((aligned(16))) u64 s_starts[WAVES][CHUNKS];
    __shared__ __attribute__((aligned(16))) u32 s_L0w[WAVES][SLOTS];       // also the gather's delta[] and the emit staging
    __shared__ __attribute__((aligned(16))) u32 s_SA[WAVES][LEVELS >= 2 ? SLOTS : 4];
    __shared__ __attribute__((aligned(16))) u32 s_SB[WAVES][LEVELS >= 3 ? SLOTS : 4];
    __shared__ __attribute__((aligned(16))) unsigned short s_preB[WAVES][LEVELS >= 3 ? SLOTS : 8];
    __shared__ __attribute__((aligned(16))) unsigned short s_preA[WAVES][LEVELS >= 4 ? SLOTS : 8];

    const int lane = lane_id();
    // product slot of this lane inside a 64-product chunk: bit-reversed, so that neighbouring
    // lanes hold products of different B rows -- their ranks are then spread over the LDS banks
    // instead of marching through the slot arrays at a near-constant stride
    const int plane = (int)(__brev((unsigned)lane) >> 26);
    const int wave_in_wg = threadIdx.x >> 6;
    const long long wave_global = (long long)blockIdx.x * WAVES + wave_in_wg;
    const long long k0 = wave_global * rpw;                        // rpw <= Cfg::RPW <= 16 rows per wave
    if (k0 >= nrows) return;                                       // wave-uniform; no barriers used
    const int nmine = (nrows - k0 < rpw) ? (int)(nrows - k0) : rpw;

    // this wave's row records: one coalesced round trip for 16 rows
    int r_row = 0, r_a0 = 0, r_alen = 0;
    long long r_pre = 0;
    if (lane < nmine) {
        const RowRec q = rec[k0 + lane];
        r_row = q.row;
        r_a0 = q.a0;
        r_alen = q.alen;
        // numeric pass after an exact symbolic pass: the row goes to its final place in C.col_idx
        // (`tmp` is C.col_idx then); otherwise to its upper-bound offset in the workspace
        if (!COUNT) r_pre = row_ptr ? row_ptr[q.row - row_begin] : recpre[k0 + lane];
    }

    u32 *top = s_top[wave_in_wg];
    unsigned short *topPre = s_topPre[wave_in_wg];
    u64 *starts = s_starts[wave_in_wg];
    u32 *L0w = s_L0w[wave_in_wg];
    int *delta = reinterpret_cast<int *>(s_L0w[wave_in_wg]);      // dead before L0w lives
    u32 *SA = s_SA[wave_in_wg];
    u32 *SB = s_SB[wave_in_wg];
    unsigned short *preA = s_preA[wave_in_wg];
    unsigned short *preB = s_preB[wave_in_wg];

    // zero the structures that must be all-zero at the start of a row (kept so by every row)
    constexpr int TW = TOPW / 64;                                  // top words per lane
    clear_blocked<TW>(top, lane);
    if (lane < CHUNKS) starts[lane] = 0ull;
    if (LEVELS >= 2) clear_blocked<SW>(SA, lane);
    if (LEVELS >= 3) clear_blocked<SW>(SB, lane);
    wave_lds_fence();

    // prefetch of the first row's B-row extents
    int2 ab_next = make_int2(0, 0);
    {
        const int a0 = wave_bcast(r_a0, 0), alen = wave_bcast(r_alen, 0);
        if (lane < alen) ab_next = load_extent(ab + a0 + lane);
    }
    // CHUNKS stores through an EMPTY descriptor (all dropped by the range check): they put the same
    // number of younger vmcnt events behind the first prefetch as every later prefetch has, so
    // the wait at the top of the row loop is vmcnt(CHUNKS) on both the entry and the back edge
    if (!COUNT) store_row<CHUNKS, false>(tmp, 0, L0w, lane);

    int my_cnt = 0;
    for (int kk = 0; kk < nmine; kk++) {
        const int a0 = wave_bcast(r_a0, kk);
        const int alen = wave_bcast(r_alen, kk);
        const u32 pre_lo = (u32)wave_bcast((int)(u32)r_pre, kk);
        const u32 pre_hi = (u32)wave_bcast((int)(u32)((unsigned long long)r_pre >> 32), kk);
        int *out = tmp + (long long)(((u64)pre_hi << 32) | pre_lo);
        int f0 = 0, mlen = 0;                                      // EXCL: F's row, ACC: D's row (absolute row id)
        if constexpr (EXCL || ACC) {
            const int i = wave_bcast(r_row, kk);
            f0 = Frow[i];
            mlen = Frow[i + 1] - f0;
        }

        // ---- gather plan: product offsets of the selected B rows ------------------------
        int F = 0, nsrc = 0;
        for (int ab0 = 0; ab0 < alen; ab0 += 64) {                 // usually one trip
            int2 e = ab_next;
            if (ab0 > 0) {
                e = make_int2(0, 0);
                if (ab0 + lane < alen) e = load_extent(ab + a0 + ab0 + lane);
            }
            const int bs = e.x, len = e.y;
            const int inc = wave_incl_scan(len);
            const int excl = F + inc - len;
            const u64 bal = __ballot(len > 0);
            // (a row always fits its class -- bin_of sized it from these very extents -- so the bound below only
            // trips when an operand was rewritten under the library; then the row is cut off, not LDS overrun)
            if (len > 0 && (unsigned)excl < (unsigned)Cfg::CAP) {
                const int sidx = nsrc + __popcll(bal & mask_lt(lane));
                delta[sidx] = bs - excl;                           // B address = delta + product index
                atomicOr(&starts[excl >> 6], 1ull << (excl & 63));
            }
            F += wave_bcast(inc, 63);
            nsrc += __popcll(bal);
        }
        // ACC: D's row is the last source, products F_B .. F_B + |D_i| (class and capacity were sized by F_B + |D_i|)
        const int nsrcB = nsrc;
        if constexpr (ACC) {
            if (mlen > 0) {
                if ((unsigned)F < (unsigned)Cfg::CAP && lane == 0) {
                    delta[nsrc] = f0 - F;                          // D address = delta + product index
                    atomicOr(&starts[F >> 6], 1ull << (F & 63));
                }
                F += mlen;
                nsrc += 1;
            }
        }
        if (F > Cfg::CAP || F < 0) {                               // wave-uniform, never taken on consistent operands
            if (lane == 0) atomicOr(err, kErrCapacity);
            F = F < 0 ? 0 : Cfg::CAP;
        }
        wave_lds_fence();
        // starts words -> registers (lane c holds word c), then cleared for the next row
        u64 sw = 0ull;
        if (lane < CHUNKS) { sw = starts[lane]; starts[lane] = 0ull; }
        const int sinc = wave_incl_scan(__popcll(sw));
        const int sbefore = sinc - __popcll(sw);

        // ---- gather B.col_idx: all lanes busy, products kept in registers ---------------
        // The loads of all chunks are issued back to back and nothing consumes them here: lanes
        // past the end of the row load Bcol[0] and are masked later by their product index, so
        // the compiler has no reason to wait between the gathers.
        int col[CHUNKS];
        int rank[CHUNKS];
        int gaddr[CHUNKS];
        bool dsrc[CHUNKS];                                         // ACC: the product is one of D's row (tail lanes: source 0's kind)
                                                                   // until sweep 1, then: one of D's row outside [0, cols)
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            {
                const int p = c * 64 + plane;
                const u64 M = wave_bcast64(sw, c);
                const int before = wave_bcast(sbefore, c);
                int s = before + __popcll(M & mask_le(plane)) - 1;
                s = (c < FULL || p < F) ? s : 0;
                if constexpr (ACC) dsrc[c] = s == nsrcB;
                // unconditional LDS read (tail lanes read source 0 and load its first column): a
                // select on the loaded value makes the compiler wait after every single read
                gaddr[c] = delta[s];                               // consumed in the next loop: the
            }                                                      // LDS reads of all chunks overlap
        }
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            {
                const int p = c * 64 + plane;
                const int g = gaddr[c] + ((c < FULL || p < F) ? p : 0);
                col[c] = BSP_WAVE_GATHER(c, g);
            }
        }
        // prefetch the next row's extents: in flight while this row is accumulated
        ab_next = make_int2(0, 0);
        if (kk + 1 < nmine) {
            const int na0 = wave_bcast(r_a0, kk + 1), nalen = wave_bcast(r_alen, kk + 1);
            if (lane < nalen) ab_next = load_extent(ab + na0 + lane);
        }
        wave_lds_fence();   // delta (aliases L0w) is dead from here on

        bool row_counted = false;   // wave-uniform: the hash filter has settled |C_i|
        int running = 0;            // |C_i|
        if constexpr (COUNT && LEVELS >= 2 && CHUNKS <= 16) {       // (beyond 16 chunks the per-chunk masks spill: the sweeps stay)
            constexpr int HB = wr_floor_log2(32 * SLOTS);          // bits of the hash bitmap (SA, all zero between rows)
            u32 *hb = SA;
            bool amb[CHUNKS];
            u64 am[CHUNKS];
            int namb = 0;
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
                const bool ok = c < FULL || c * 64 + plane < F;
                const u32 cc = (u32)col[c];
                const u32 h = (cc ^ (cc >> HB) ^ (2 * HB < 32 ? cc >> ((2 * HB) & 31) : 0u)) & ((1u << HB) - 1u);
                u32 old = 0u;
                if (ok) old = atomicOr(&hb[h >> 5], 1u << (h & 31));
                amb[c] = ok && ((old >> (h & 31)) & 1u);
            }
            wave_lds_fence();
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
                am[c] = __ballot(amb[c]);
                namb += __popcll(am[c]);
            }
            clear_blocked<SW>(hb, lane);                           // SA is all zero again, whichever way the row goes
            wave_lds_fence();
            if (namb <= kMaxAmbiguous) {
                int dups = 0;
                if (namb > 0) {
#pragma unroll
                    for (int c = 0; c < CHUNKS; c++) {
                        u64 m = am[c];
                        while (m) {                                // (wave-uniform: m is a ballot)
                            const int l = (int)__builtin_ctzll(m);
                            m &= m - 1ull;
                            const u32 x = (u32)__builtin_amdgcn_readlane(col[c], l);
                            u64 hit = 0ull;                        // equal products that settle it: not ambiguous, or ambiguous and earlier
#pragma unroll
                            for (int c2 = 0; c2 < CHUNKS; c2++) {
                                const bool ok2 = c2 < FULL || c2 * 64 + plane < F;
                                const u64 e = __ballot(ok2 && (u32)col[c2] == x);
                                hit |= e & ~am[c2];
                                if (c2 < c) hit |= e & am[c2];
                                if (c2 == c) hit |= e & am[c2] & mask_lt(l);
                            }
                            dups += hit != 0ull ? 1 : 0;
                        }
                    }
                }
                running = F - dups;
                row_counted = true;
            }
        }
        if (!row_counted) {
        // ---- sweep 1: top bitmap, addressed directly by the high digits -----------------
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            {
                if constexpr (ACC) dsrc[c] = dsrc[c] && (u32)col[c] >= (u32)cols;   // from here on: a column of D that is dropped
                const bool ok = BSP_WAVE_OK(c < FULL || c * 64 + plane < F, c);
                const u32 cc = ok ? (u32)col[c] : 0u;
                col[c] = (int)cc;                                  // tail lanes: column 0, never OR-ed
                const u32 tw = cc >> (5 * LEVELS);
                // tail lanes are masked off: parking them on one spare word instead makes up to 63
                // same-address atomics, which the LDS serialises (measured: -12 % kernel time)
                if (ok) atomicOr(&top[tw], 1u << ((cc >> (5 * (LEVELS - 1))) & 31));
                rank[c] = (int)tw;
            }
        }
        wave_lds_fence();

        u32 *S0;                     // level-0 slots (32-column masks) of this row
        int nslots0 = 0;             // how many of them the row uses (LEVELS >= 2)
        if (LEVELS == 1) {
            S0 = top;
        } else {
            // number of slots of the level below the one just scanned; after the last scan it is
            // the number of level-0 slots of the row
            nslots0 = scan_blocked<TW>(top, topPre, lane);         // ranks of the level LEVELS-2 slots
            wave_lds_fence();
            const u32 *P = top;
            const unsigned short *Ppre = topPre;
            u32 *Pmut = top;
            bool parent_is_top = true;
#pragma unroll
            for (int lev = LEVELS - 2; lev >= 0; lev--) {
                // as many level-0 slots as products: every product sits alone in its 32-column slot
                // (wave-uniform; nslots0 counts the slots of level `lev` here)
                const bool sparse = lev == 0 && nslots0 == F;
                // level `lev` slot buffers alternate: lev even -> SA/preA, lev odd -> SB/preB
                u32 *S = (lev & 1) ? SB : SA;
                unsigned short *Spre = (lev & 1) ? preB : preA;
                u32 px[CHUNKS];
                int ppre[CHUNKS];
#pragma unroll
                for (int c = 0; c < CHUNKS; c++)                   // all parent reads first ...
                    {
                        px[c] = P[rank[c]];
                        ppre[c] = Ppre[rank[c]];
                    }
#pragma unroll
                for (int c = 0; c < CHUNKS; c++)                   // ... then all the ORs
                    {
                        const bool ok = BSP_WAVE_OK(c < FULL || c * 64 + plane < F, c);
                        const u32 cc = (u32)col[c];
                        const u32 b = (cc >> (5 * (lev + 1))) & 31;
                        const int r2 = ppre[c] + __popc(__builtin_amdgcn_ubfe(px[c], 0u, b));   // bits below b
                        const u32 bit = 1u << ((cc >> (5 * lev)) & 31);
                        if (ok) {                                  // tail lanes: no LDS traffic at all
                            if (lev == 0) {
                                // a sparse row -- known since the scan of the level above -- never reads
                                // its masks: only the column beside the mask is kept
                                if (!sparse) atomicOr(&S[r2], bit);
                                if (!COUNT) L0w[r2] = cc;          // any product of the slot: same cc >> 5
                            } else {
                                atomicOr(&S[r2], bit);
                            }
                        }
                        rank[c] = r2;
                    }
                wave_lds_fence();
                if (parent_is_top) clear_blocked<TW>(Pmut, lane);  // parent level is consumed
                else clear_blocked<SW>(Pmut, lane);
                parent_is_top = false;
                if (lev > 0) {
                    nslots0 = scan_blocked<SW>(S, Spre, lane);
                    P = S;
                    Pmut = S;
                    Ppre = Spre;
                }
                wave_lds_fence();
            }
            S0 = SA;                                               // level 0 is even
        }

        // ---- emit: lane l expands its own W consecutive level-0 slots (ascending columns) into
        // the LDS staging row at the rank given by one wave scan, then the wave streams the
        // staged row to memory fully coalesced.
        constexpr int W0 = (LEVELS == 1) ? TW : SW;
        if (LEVELS >= 2 && nslots0 == F) {
            // Sparse row (the common case when cols >> F_i): every level-0 slot holds ONE column,
            // so slot index = output position and L0w already is the sorted row.
            running = nslots0;                                     // (the masks were never written)
            if constexpr (EXCL)
                if (running > 0 && mlen > 0) running = drop_mask_cols<CHUNKS, false>(L0w, running, top, Fcol, f0, mlen, lane);
            if (!COUNT) store_row<CHUNKS, false>(out, running, L0w, lane);
        } else if (COUNT) {
            u32 m[W0];
#pragma unroll
            for (int k = 0; k < W0; k++) m[k] = S0[lane * W0 + k];
            clear_blocked<W0>(S0, lane);
            int mine = 0;
#pragma unroll
            for (int k = 0; k < W0; k++) mine += __popc(m[k]);
            running = wave_bcast(wave_incl_scan(mine), 63);
        } else {
            u32 m[W0], wv[W0];
#pragma unroll
            for (int k = 0; k < W0; k++) {
                m[k] = S0[lane * W0 + k];
                wv[k] = (LEVELS == 1) ? (u32)(lane * W0 + k) : (L0w[lane * W0 + k] >> 5);
            }
            clear_blocked<W0>(S0, lane);
            int mine = 0;
#pragma unroll
            for (int k = 0; k < W0; k++) mine += __popc(m[k]);
            const int inc = wave_incl_scan(mine);
            running = wave_bcast(inc, 63);
            wave_lds_fence();                                      // L0w reads are done: reuse it as staging
            {
                u32 *stage = L0w;
                int pos = inc - mine;
#pragma unroll
                for (int k = 0; k < W0; k++) {
                    u32 mk = m[k];
                    const u32 base = wv[k] << 5;
                    while (mk) {
                        stage[stage_swz(pos)] = base | (u32)__builtin_ctz(mk);
                        pos++;
                        mk &= mk - 1u;
                    }
                }
            }
            wave_lds_fence();
            if constexpr (EXCL)
                if (running > 0 && mlen > 0) running = drop_mask_cols<CHUNKS, true>(L0w, running, top, Fcol, f0, mlen, lane);
            store_row<CHUNKS, true>(out, running, L0w, lane);
        }
        }   // !row_counted
        my_cnt = (lane == kk) ? running : my_cnt;                  // lane kk keeps |C_i| of row kk
        wave_lds_fence();
    }
    if (cnt && lane < nmine) cnt[r_row - row_begin] = my_cnt;
#undef BSP_WAVE_GATHER
#undef BSP_WAVE_OK
