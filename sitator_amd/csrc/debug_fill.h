// SITATOR_DEBUG_FILL=<two hex digits>, in a form the host compiler takes too (tests/test_debug_fill.py).  With the knob set
// the library fills device memory with that byte before it uses it (sit_internal.h: sit_debug_fill), so that a kernel
// which reads a piece nobody wrote meets the fill instead of whatever the last user left.  "ff" is NaN as a float and -1
// as an integer (and the cleared state of several tables); "7b" is a finite 1e286 / 1e36 and a large positive integer.
#pragma once

#include <stdlib.h>

// the byte of the text of the knob, -1 where it is not exactly two hexadecimal digits (no prefix, no sign, no blanks)
static inline int debug_fill_parse(const char *s)
{
    if (!s || !s[0] || !s[1] || s[2]) return -1;
    int v = 0;
    for (int i = 0; i < 2; i++) {
        const char ch = s[i];
        int d;
        if (ch >= '0' && ch <= '9') d = ch - '0';
        else if (ch >= 'a' && ch <= 'f') d = ch - 'a' + 10;
        else if (ch >= 'A' && ch <= 'F') d = ch - 'A' + 10;
        else return -1;
        v = v * 16 + d;
    }
    return v;
}

// read at each use (a test switches it between calls); -1: off
static inline int debug_fill_byte(void) { return debug_fill_parse(getenv("SITATOR_DEBUG_FILL")); }
