// early_dest.hpp -- the early destination of the int32 drop-ins (dropin.hip): a malloc'ed block sized by an upper bound of
// nnz(C), which a helper thread faults in and pins IN PLACE piece by piece while the caller uploads and multiplies, so that
// the download can follow it piece by piece as DMA into the caller's own memory.  Host only: no HIP header, no HIP call;
// pinning and unpinning are two function pointers (none: nothing is pinned).  The object owns the block, the helper, the
// per-piece pin flags and everything the two threads share.
//
// THE INVARIANT: no piece is unpinned and the block is not freed while a copy into it can be in flight.  The object cannot
// see the caller's stream, so the caller drains it before release(), drop() or destruction.
#pragma once
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>

extern "C" void bspgemm_par_prefault(void *p, size_t bytes);      // first touch on all host threads (host/par_copy.c)

namespace bsp {

// transparent huge pages for the 2 MiB-aligned interior of [p, p + bytes) (no effect where THP is off)
static inline void advise_huge_pages(void *p, size_t bytes)
{
    const uintptr_t m = ((uintptr_t)2 << 20) - 1;
    const uintptr_t lo = (reinterpret_cast<uintptr_t>(p) + m) & ~m, hi = (reinterpret_cast<uintptr_t>(p) + bytes) & ~m;
    if (hi > lo) madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_HUGEPAGE);
}

class EarlyDest {
public:
    using PinFn = bool (*)(void *p, size_t bytes);      // true: [p, p + bytes) is pinned now
    using UnpinFn = void (*)(void *p);                  // p: what PinFn was given
    const size_t piece;
    // Pieces of 128 MiB: first touch (the kernel zeroes the pages), then the pin; zeroing, pinning and the DMA that follows
    // them overlap instead of adding up (zeroing + pinning 5.3 GB take about as long as moving it over the link).
    explicit EarlyDest(PinFn pin = nullptr, UnpinFn unpin = nullptr, size_t piece_bytes = (size_t)128 << 20)
        : piece(piece_bytes), pin_(unpin ? pin : nullptr), unpin_(unpin) {}
    ~EarlyDest() { drop(); }

    // Spawns the helper: malloc of `bytes` (> 0), huge-page advice, then per piece first touch, pin, publish.  Once.
    void start(size_t bytes)
    {
        bytes_ = bytes;
        pinned_.assign((bytes + piece - 1) / piece, 0);
        exited_ = false;
        helper_ = std::thread([this] { run(); });
    }
    // The block, once it exists; NULL if its malloc failed or start() was never called.
    int *block()
    {
        while (!block_ && !exited_) usleep(50);
        return block_;
    }
    // true once piece k is faulted in (pinned or not); false if the helper ended without getting there
    bool wait_piece(size_t k)
    {
        while (ready_ <= k && !exited_) usleep(50);
        return ready_ > k;
    }
    // The helper ends after its current piece (pieces beyond nnz(C) are not needed); joined here.  Idempotent.
    void stop()
    {
        stop_ = true;
        if (helper_.joinable()) helper_.join();
    }
    // Hands the block over: the helper stopped, every pinned piece unpinned once, and what the bound overshot given back
    // (in place: the block only shrinks) when that is more than 2^20 ints.  The object forgets the block; NULL if there is none.
    int *release(size_t keep_bytes)
    {
        stop();                                         // (pinned_ was the helper's until here)
        int *p = block_.exchange(nullptr);
        for (size_t k = 0; k < pinned_.size(); k++)
            if (pinned_[k]) { unpin_(reinterpret_cast<char *>(p) + k * piece); pinned_[k] = 0; }
        if (p && bytes_ > keep_bytes && (bytes_ - keep_bytes) / sizeof(int) > ((size_t)1 << 20))
            if (void *shrunk = realloc(p, keep_bytes ? keep_bytes : sizeof(int))) p = static_cast<int *>(shrunk);
        return p;
    }
    // What the destructor does: stop, unpin, free.  Idempotent.
    void drop() { free(release(bytes_)); }

private:
    void run()
    {
        char *base = static_cast<char *>(malloc(bytes_));
        block_ = reinterpret_cast<int *>(base);
        if (base) advise_huge_pages(base, bytes_);
        for (size_t k = 0; base && k < pinned_.size() && !stop_; k++) {
            const size_t off = k * piece, len = (bytes_ - off < piece) ? bytes_ - off : piece;
            bspgemm_par_prefault(base + off, len);
            if (pin_ && pin_(base + off, len)) pinned_[k] = 1;
            ready_ = k + 1;
        }
        exited_ = true;
    }

    const PinFn pin_;
    const UnpinFn unpin_;
    size_t bytes_ = 0;
    std::vector<char> pinned_;                          // per piece: pinned by the helper, not yet unpinned
    std::thread helper_;
    // what the two threads share (sequentially consistent: a handful of accesses per 128 MiB piece)
    std::atomic<int *> block_{nullptr};
    std::atomic<size_t> ready_{0};                      // pieces faulted in so far
    std::atomic<bool> stop_{false}, exited_{true};      // exited_: no helper is running
};

}   // namespace bsp
