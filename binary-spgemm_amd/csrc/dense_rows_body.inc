// dense_rows_body.inc -- the body of the windowed heavy-row kernels, included inside k_dense_rows, k_dense_rows_excl and
// k_dense_rows_acc (dense_rows.hip), which provide kDenseThreads, the arguments, MASKED (keep F's columns: two bitmaps) and
// MODE (MaskMode::Drop: clear F's columns from each window; MaskMode::Insert: set the columns of D's row -- passed as
// Frow / Fcol -- that lie in [0, cols) in each window).  A text body and not a __forceinline__ function, so that
// k_dense_rows compiles to the same code as before its twin existed (see wave_rows_body.inc).
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

