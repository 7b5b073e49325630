// rank_rows_body.inc -- the body of the rank-class kernels, included inside k_rank_rows, k_rank_rows_excl and k_rank_rows_acc
// (dense_rows.hip), which provide kSpans (false: the column range is one span, the common case: one pass, its quads kept in
// registers), the arguments, DROP (clear F's columns from each span's slots before the read-out) and INS (set the columns of
// D's row -- passed as Frow / Fcol -- that lie in [0, cols) and in the span: its top bits after sweep 1, its slots after sweep 2).  A text body, so that k_rank_rows
// compiles to the same code as before its twin existed (see wave_rows_body.inc).
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

