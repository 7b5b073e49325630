// early_dest_main.cpp -- csrc/early_dest.hpp on the CPU, built twice by oracle/Makefile (asan): under
// -fsanitize=address,undefined and under -fsanitize=thread; run by tests/test_host_c.py.  No HIP, no OpenMP: the pin hooks
// are counting stubs and the first touch is a plain loop.  Pieces of 64 KiB.  Any failed check or sanitizer report ends
// the program with a non-zero status.
#include "../binary-spgemm_amd/csrc/early_dest.hpp"

#include <cstdio>

extern "C" void bspgemm_par_prefault(void *p, size_t bytes)
{
    volatile char *c = static_cast<volatile char *>(p);
    for (size_t i = 0; i < bytes; i += 4096) c[i] = 0;
    if (bytes) c[bytes - 1] = 0;
}

static std::atomic<int> g_pins{0}, g_unpins{0}, g_asked{0};
static bool pin_all(void *, size_t) { g_pins++; return true; }
static bool pin_every_second(void *, size_t) { if (g_asked++ % 2) return false; g_pins++; return true; }
static void unpin(void *) { g_unpins++; }
static void reset() { g_pins = g_unpins = g_asked = 0; }

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

constexpr size_t kPiece = (size_t)64 << 10;
static unsigned char pattern(size_t i) { return (unsigned char)(i * 131 + (i >> 16) + 7); }

// the consumer of dropin.hip's download: follows wait_piece and writes into each piece as it arrives
static void fill_behind_helper(bsp::EarlyDest &e, size_t bytes)
{
    unsigned char *b = reinterpret_cast<unsigned char *>(e.block());
    CHECK(b);
    for (size_t k = 0, off = 0; off < bytes; k++, off += kPiece) {
        CHECK(e.wait_piece(k));
        for (size_t i = off; i < bytes && i < off + kPiece; i++) b[i] = pattern(i);
    }
}

int main()
{
    {   // 1. five pieces and 123 bytes, consumed piece by piece, released with less than the whole
        reset();
        const size_t bytes = 5 * kPiece + 123, keep = 3 * kPiece + 17;
        bsp::EarlyDest e(pin_all, unpin, kPiece);
        e.start(bytes);
        fill_behind_helper(e, bytes);
        unsigned char *b = reinterpret_cast<unsigned char *>(e.release(keep));
        CHECK(b && g_pins == 6 && g_unpins == 6);
        for (size_t i = 0; i < keep; i++) CHECK(b[i] == pattern(i));
        CHECK(!e.block() && !e.release(0));             // forgotten
        free(b);
        // ... and an overshoot above 2^20 ints is given back: the block shrinks to `keep`, its content stays
        reset();
        const size_t big = ((size_t)5 << 20) + 123, keep2 = kPiece + 5;
        bsp::EarlyDest g(pin_all, unpin, kPiece);
        g.start(big);
        fill_behind_helper(g, keep2);
        b = reinterpret_cast<unsigned char *>(g.release(keep2));
        CHECK(b && g_pins == g_unpins && g_pins >= 2);
        for (size_t i = 0; i < keep2; i++) CHECK(b[i] == pattern(i));
        free(b);                                        // (AddressSanitizer: the block has keep2 bytes now)
    }
    {   // 2. eight pieces, stopped after piece 1, then destroyed: the leak check sees the block freed
        reset();
        {
            bsp::EarlyDest e(pin_all, unpin, kPiece);
            e.start(8 * kPiece);
            CHECK(e.wait_piece(1));
            e.stop();
            e.stop();                                   // idempotent
            CHECK(g_pins >= 2 && g_pins <= 8 && g_unpins == 0);
            if (g_pins < 8) CHECK(!e.wait_piece(7));    // a piece that will not come does not block
        }
        CHECK(g_pins == g_unpins && g_pins <= 8);
    }
    {   // 3. every second pin refused: the pieces still arrive, only the pinned ones are unpinned
        reset();
        bsp::EarlyDest e(pin_every_second, unpin, kPiece);
        e.start(6 * kPiece);
        for (size_t k = 0; k < 6; k++) CHECK(e.wait_piece(k));
        free(e.release(6 * kPiece));
        CHECK(g_asked == 6 && g_pins == 3 && g_unpins == 3);
    }
    {   // 4. no hooks: nothing is pinned or unpinned
        reset();
        bsp::EarlyDest e(nullptr, nullptr, kPiece);
        e.start(3 * kPiece + 1);
        fill_behind_helper(e, 3 * kPiece + 1);
        free(e.release(3 * kPiece + 1));
        CHECK(g_pins == 0 && g_unpins == 0);
    }
    {   // 5. destroyed without start; started and destroyed at once
        reset();
        {
            bsp::EarlyDest e(pin_all, unpin, kPiece);
            CHECK(!e.block() && !e.wait_piece(0));
        }
        {
            bsp::EarlyDest e(pin_all, unpin, kPiece);
            e.start(8 * kPiece);
        }
        CHECK(g_pins == g_unpins);
    }
    {   // 6. release(0): a block that free takes
        reset();
        bsp::EarlyDest e(pin_all, unpin, kPiece);
        e.start(2 * kPiece);
        int *p = e.release(0);
        CHECK(p && g_pins == g_unpins);
        free(p);
    }
    printf("early_dest ok\n");
    return 0;
}
