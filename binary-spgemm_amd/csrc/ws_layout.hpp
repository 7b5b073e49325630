// ws_layout.hpp -- the layout of an entry point's arrays in the context's int workspace (ctx->tmp), stated ONCE: the
// same list of take() calls sizes the workspace (base NULL: what to ask ensure_tmp for) and places the typed pointers
// (base = ctx->tmp AS IT IS NOW: after anything that may have moved the workspace the list is walked again).  Every array
// starts on a 16-byte boundary of the workspace.  Host-only, no HIP header: a stand-alone program compiles it with plain g++
// and walks it under the sanitizers (tests/test_host_c.py).
#pragma once
#include <cstddef>

// n rounded up to a multiple of 4: an int array of that many entries ends on a 16-byte boundary
static inline size_t ws_pad4(size_t n) { return (n + 3) & ~(size_t)3; }

struct WsCursor {
    int *base;                          // NULL: the sizing pass, every pointer comes out NULL
    size_t at;                          // int offset of the end of the last array (start: where the layout begins)
    explicit WsCursor(int *tmp, size_t start = 0) : base(tmp), at(start) {}
    // the next array: `count` entries of T from the next 16-byte boundary
    template <class T> WsCursor &take(T *&p, size_t count)
    {
        at = ws_pad4(at);
        p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += (count * sizeof(T) + sizeof(int) - 1) / sizeof(int);
        return *this;
    }
    // an array that only some calls have: NULL and no ints where it is not wanted
    template <class T> WsCursor &take_if(bool wanted, T *&p, size_t count)
    {
        if (wanted) return take(p, count);
        p = nullptr;
        return *this;
    }
    size_t aligned() { return at = ws_pad4(at); }   // where the next array starts (a flag_scratch_carve behind the list)
    size_t ints() const { return at; }              // ints of the workspace up to the end of the last array
};
