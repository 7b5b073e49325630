// ws_layout_main.cpp -- csrc/ws_layout.hpp (the cursor that lays an entry point's arrays out in the context's int
// workspace) on the CPU under -fsanitize=address,undefined (oracle/Makefile, target asan; run by tests/test_host_c.py).
// Every sequence is sized with a NULL base, placed over a heap block of EXACTLY the reported size and written byte by
// byte: the sanitizer is the check that the total suffices.  A failed check or a report ends with a non-zero status.
#include "../binary-spgemm_amd/csrc/ws_layout.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "ws_layout: %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

struct Pair { int x, y; };                       // int2-like
struct Rec24 { uint64_t a, b; int c, d; };       // a 24-byte record
static_assert(sizeof(Pair) == 8 && sizeof(Rec24) == 24, "the element sizes the cases are about");

struct Slot { size_t off, bytes; };              // where an array came out: bytes from the base, and its length

// one array of element type `type` (0 .. 4) with `count` entries from the cursor
static Slot take_one(WsCursor &c, int type, size_t count)
{
    char *p = nullptr;
    size_t size = 0;
    switch (type) {
    case 0: { int *q; c.take(q, count); p = (char *)q; size = sizeof(int); break; }
    case 1: { unsigned char *q; c.take(q, count); p = (char *)q; size = 1; break; }
    case 2: { Pair *q; c.take(q, count); p = (char *)q; size = sizeof(Pair); break; }
    case 3: { uint64_t *q; c.take(q, count); p = (char *)q; size = sizeof(uint64_t); break; }
    default: { Rec24 *q; c.take(q, count); p = (char *)q; size = sizeof(Rec24); break; }
    }
    CHECK((p == nullptr) == (c.base == nullptr));
    // placed: the offset is read off the pointer; sized: off the cursor, which has just added the array's ints
    const size_t ints = (count * size + 3) / 4;
    return Slot{p ? (size_t)(p - reinterpret_cast<char *>(c.base)) : (c.at - ints) * sizeof(int), count * size};
}

static size_t walk(int *base, size_t start, const std::vector<int> &types, const std::vector<size_t> &counts, std::vector<Slot> *out)
{
    WsCursor c(base, start);
    out->clear();
    for (size_t i = 0; i < types.size(); i++) out->push_back(take_one(c, types[i], counts[i]));
    return c.ints();
}

static long sequences = 0;

static void check_sequence(size_t start, const std::vector<int> &types, const std::vector<size_t> &counts)
{
    std::vector<Slot> sized, placed, moved;
    const size_t total = walk(nullptr, start, types, counts, &sized);
    size_t end = start * sizeof(int);
    for (const Slot &a : sized) {
        CHECK(a.off % 16 == 0);                                  // every start on a 16-byte boundary of the workspace
        CHECK(a.off >= end);                                     // disjoint and ascending
        end = a.off + a.bytes;
    }
    CHECK(total * sizeof(int) >= end);                           // the total covers the end of the last array
    CHECK(total * sizeof(int) < end + sizeof(int));              // ... and no more than the int it ends in
    // placing over a block of exactly the reported size, then over a second one: the same offsets from either base
    int *blk[2] = {static_cast<int *>(malloc(total * sizeof(int))), static_cast<int *>(malloc(total * sizeof(int)))};
    CHECK((blk[0] && blk[1]) || total == 0);
    CHECK(walk(blk[0], start, types, counts, &placed) == total);
    CHECK(walk(blk[1], start, types, counts, &moved) == total);
    for (size_t i = 0; i < sized.size(); i++) {
        CHECK(placed[i].off == sized[i].off && moved[i].off == sized[i].off);
        if (total == 0) continue;                                // (a NULL block: nothing to write)
        for (int b = 0; b < 2; b++) memset(reinterpret_cast<char *>(blk[b]) + sized[i].off, 0xA5 + (int)i, sized[i].bytes);
    }
    // the pointers themselves, through the typed interface
    if (total > 0) {
        WsCursor c(blk[1], start);
        uint64_t *q = nullptr;
        c.take(q, 1);
        CHECK(reinterpret_cast<char *>(q) == reinterpret_cast<char *>(blk[1]) + ws_pad4(start) * sizeof(int));
    }
    free(blk[0]);
    free(blk[1]);
    sequences++;
}

// the layouts of three entry points before the cursor, as plain arithmetic, against the cursor's totals
static void check_parity(size_t n)
{
    const size_t n4 = (n + 3) & ~(size_t)3;
    struct Flags16 { int w[4]; } *flags;                         // the counter blocks of the colouring and the peeling
    struct Counters96 { uint64_t w[9]; int v[6]; } *cnt;          // PageRank's
    int *a, *b, *c, *d;
    uint64_t *k, *r, *c0, *c1, *acc;
    Pair *chunk;
    // colouring: the counters, key (64-bit), cnt and the two lists
    CHECK(WsCursor(nullptr).take(flags, 1).take(k, n4).take(a, n4).take(b, n4).take(c, n4).ints() == 4 + 5 * n4);
    // core numbers: the counters, deg and the two lists
    CHECK(WsCursor(nullptr).take(flags, 1).take(a, n4).take(b, n4).take(c, n4).ints() == 4 + 3 * n4);
    // PageRank under PULL, for a graph of 5 n entries: the counters, r, c[2], acc (64-bit), four class lists, the chunk records
    const size_t chunk_cap = n + (5 * n) / 4096 + 1;
    const size_t o_r = sizeof(Counters96) / sizeof(int), o_c = o_r + 2 * n4, o_acc = o_c + 4 * n4, o_list = o_acc + 2 * n4;
    const size_t o_chunk = o_list + 4 * n4, own_ints = o_chunk + 2 * chunk_cap;
    CHECK(WsCursor(nullptr).take(cnt, 1).take(r, n4).take(c0, n4).take(c1, n4).take(acc, n4).take(d, 4 * n4).take(chunk, chunk_cap).ints() ==
          own_ints);
}

int main()
{
    const size_t counts[] = {0, 1, 3, 4, 5, 70};
    for (size_t start : {(size_t)0, (size_t)5}) {
        // every ordered pair of (type, count) x (type, count), and behind it one of every type at a third count
        for (int t0 = 0; t0 < 5; t0++)
            for (size_t c0 : counts)
                for (int t1 = 0; t1 < 5; t1++)
                    for (size_t c1 : counts)
                        for (size_t c2 : counts)
                            check_sequence(start, {t0, t1, 0, 1, 2, 3, 4}, {c0, c1, c2, c2, c2, c2, c2});
        check_sequence(start, {}, {});
        for (int t = 0; t < 5; t++)
            for (size_t c : counts) check_sequence(start, {t}, {c});
    }
    // an array that a call does not have: NULL, no ints, and what follows stays where it would be without it
    {
        int blk[16];
        int *x = blk, *y = nullptr, *z = nullptr;
        WsCursor c(blk);
        c.take(y, 3).take_if(false, x, 70).take(z, 1);
        CHECK(x == nullptr && y == blk && z == blk + 4 && c.ints() == 5 && c.aligned() == 8);
    }
    for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)70}) check_parity(n);
    printf("ws_layout ok: %ld sequences\n", sequences);
    return 0;
}
