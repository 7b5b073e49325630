// wave_rows.hip -- dispatcher of the one-wave-per-row kernels (the kernel: wave_rows.inc, built once per (LEVELS, mode)
// pair).  Picks the number of 5-bit levels from B's column count; launch_class picks the kernel family of a class.
#include "kernels.hpp"

namespace bsp {

template <int LEVELS, MaskMode MODE>
void launch_wave_levels(int bin, const int2 *ab, const int *Bcol, int cols, int topw, const RowRec *rec,
                        const long long *recpre, const long long *row_ptr, int nrows, int row_begin, int *tmp, int *cnt,
                        unsigned *err, const int *Frow, const int *Fcol, hipStream_t s, bool count, int shared_max);
#define BSP_WAVE_EXTERN1(L, M) \
    extern template void launch_wave_levels<L, MaskMode::M>(int, const int2 *, const int *, int, int, const RowRec *, \
        const long long *, const long long *, int, int, int *, int *, unsigned *, const int *, const int *, hipStream_t, bool, int);
#define BSP_WAVE_EXTERN(L) BSP_WAVE_EXTERN1(L, None) BSP_WAVE_EXTERN1(L, Drop) BSP_WAVE_EXTERN1(L, Insert)
BSP_WAVE_EXTERN(1) BSP_WAVE_EXTERN(2) BSP_WAVE_EXTERN(3) BSP_WAVE_EXTERN(4) BSP_WAVE_EXTERN(5)
#undef BSP_WAVE_EXTERN
#undef BSP_WAVE_EXTERN1

// words of the directly addressed top bitmap: ceil(cols / 32^levels) <= kWaveTopWords
static int wave_top_words(int levels, int cols)
{
    const long long span = 1ll << (5 * levels);
    return (int)(((long long)cols + span - 1) / span);
}

// shared_max of class `bin` (k_wave_rows: a row with up to that many products more than level-0 slots is emitted without
// its masks) for a value of BSPGEMM_OPT_SHARED_SLOTS.  The automatic table is per class and measured ("few
// shared slots"; profiles/r07_shared_slots_*): every loser costs a pass over the row's chunks, the masks it saves cost the
// same whatever their number.  Up to 4 chunks: 4 -- n = 2^18 uniform (every row 256 products, 4 shared slots on average) is
// level up to 4 and 1.5 % of its numeric phase slower from 5 on.  5 .. 8 chunks: 8 -- the bench matrix still gains from 4 to
// 8 (numeric phase 3.25 -> 3.23 ms) and is level above.  10, 12 chunks: 4, as the chunks per loser double -- 8 is within
// their run-to-run spread.  14, 16 chunks: 8 -- at 4, 18 % and 37 % of the bench matrix's rows of these classes still build
// their masks, at 8 under 2 %; measured per class on one stream, 0.165 -> 0.161 ms and 0.078 -> 0.075 ms, level from 8 to 16
// (profiles/large_classes_per_class.log).  Above 16 chunks the path is not compiled: it gains 3 % in the class of 20 chunks
// (1.2 % of the products) and loses from 24 chunks on.
int wave_shared_max(int bin, int shared_slots)
{
    static_assert(kWaveBins == 16, "one entry per capacity class");
    //                                          chunks: -  1  2  3  4  5  6  7  8 10 12 14 16 20 24 28 32
    static const int auto_max[kWaveBins + 1] = {0, 4, 4, 4, 4, 8, 8, 8, 8, 4, 4, 8, 8, 0, 0, 0, 0};
    if (bin < 1 || bin > kWaveBins || kWaveChunks[bin] > 16) return 0;       // (no such path above 16 chunks)
    if (shared_slots < 0) return auto_max[bin];
    return shared_slots > kSharedSlotsMax ? kSharedSlotsMax : shared_slots;
}

hipError_t launch_wave_rows(int bin, int levels, const int2 *ab, const int *Bcol, int cols,
                            const RowRec *rec, const long long *recpre, const long long *row_ptr, int nrows, int row_begin,
                            int *tmp, int *cnt, unsigned *err, MaskMode mode, const int *Frow, const int *Fcol, hipStream_t s,
                            bool count_only, int shared_slots)
{
    if (mode == MaskMode::Keep || mode == MaskMode::Count || (count_only && mode != MaskMode::None)) return hipErrorInvalidValue;
    if (nrows <= 0) return hipSuccess;
#define BSP_WAVE_ROW(M) {launch_wave_levels<1, MaskMode::M>, launch_wave_levels<2, MaskMode::M>, launch_wave_levels<3, MaskMode::M>, \
                         launch_wave_levels<4, MaskMode::M>, launch_wave_levels<5, MaskMode::M>}
    static const decltype(&launch_wave_levels<1, MaskMode::None>) by_levels[3][5] = {BSP_WAVE_ROW(None), BSP_WAVE_ROW(Drop),
                                                                                      BSP_WAVE_ROW(Insert)};
#undef BSP_WAVE_ROW
    const int m = mode == MaskMode::Drop ? 1 : (mode == MaskMode::Insert ? 2 : 0);
    by_levels[m][(levels < 5 ? levels : 5) - 1](bin, ab, Bcol, cols, wave_top_words(levels, cols), rec, recpre, row_ptr, nrows,
                                                row_begin, tmp, cnt, err, Frow, Fcol, s, count_only,
                                                count_only ? 0 : wave_shared_max(bin, shared_slots));
    return hipSuccess;
}

hipError_t launch_class(int bin, const int2 *ab, const int *Bcol, long long nnzB, int cols, const RowRec *rec,
                        const long long *recpre, int nrows, int row_begin, int *tmp, int *cnt, unsigned *err, MaskMode mode,
                        const int *Frow, const int *Fcol, hipStream_t s, bool count_only, int *vals, int shared_slots)
{
    if (bin > kWaveBins)
        return launch_dense_rows(bin, ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, mode, Frow, Fcol, s, vals);
    if (mode != MaskMode::Keep && mode != MaskMode::Count)   // (the count pass emits nothing: no output offsets, no workspace)
        return launch_wave_rows(bin, wave_levels_for_cols(cols), ab, Bcol, cols, rec, count_only ? nullptr : recpre, nullptr,
                                nrows, row_begin, count_only ? nullptr : tmp, cnt, err, mode, Frow, Fcol, s, count_only,
                                shared_slots);
    if (!wave_masked_supported(cols))
        return launch_dense_rows(bin, ab, Bcol, nnzB, cols, rec, recpre, nrows, row_begin, tmp, cnt, mode, Frow, Fcol, s, vals);
    launch_wave_masked(bin, ab, Bcol, cols, Frow, Fcol, rec, recpre, nrows, row_begin, tmp, cnt,
                       mode == MaskMode::Count ? vals : nullptr, s);
    return hipSuccess;
}

}  // namespace bsp
