// The scratch carver, in a form the host compiler takes too (tests/test_scratch_carve.py runs it with g++ under ASan / UBSan).
// A layout is written once, as the takes it makes; run on a null base it sizes the buffer (`used`), run on the buffer it
// hands out the pointers - the byte count and the pointers cannot disagree.  carve_scratch (sit_internal.h) does both
// runs over the context's scratch buffer.
#pragma once

#include <stdint.h>

struct Carve {
    char *base;                                                  // aligned to the largest `align` asked for (hipMalloc: 256)
    int64_t used;
    // n elements from the next multiple of `align` (a power of two, 16 or more) on; a piece is a multiple of 16 bytes.
    // n <= 0: no bytes (the pointer is the next take's)
    template <class T> T *take(int64_t n, int64_t align = 16)
    {
        used = (used + align - 1) & ~(align - 1);
        T *p = base ? (T *)(base + used) : nullptr;
        used += ((n > 0 ? n : 0) * (int64_t)sizeof(T) + 15) & ~(int64_t)15;
        return p;
    }
};
