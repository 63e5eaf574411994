"""CPU-only: the scratch carver (sitator_amd/csrc/scratch_carve.h) compiled with the host compiler into a stand-alone program
under ASan / UBSan.  A layout is run on a null base to size the buffer and then on a heap buffer of EXACTLY that size, so a
take that hands out one byte too many is a heap overflow the sanitizer reports.  (The layouts of the label scans and of the
grouping run over the same carver in test_label_scan.py and test_group_ref.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv: "self" or "random <seed> <layouts>".  Exit 0: every check held; 3: one did not (stderr says which).
PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include "scratch_carve.h"

struct E72 { char b[72]; };
struct E16 { char b[16]; };

static char *g_base;
static int64_t g_used;

static void fail(const char *what, int layout) { fprintf(stderr, "%s (layout %d)\n", what, layout); exit(3); }

// sized on a null base, then carved over exactly `used` bytes on a 64-byte boundary (what the largest alignment asks of a base)
template <class Lay> static void carve(Lay lay)
{
    Carve size = {nullptr, 0};
    lay(size);
    g_used = size.used;
    void *p = nullptr;
    if (posix_memalign(&p, 64, (size_t)g_used)) exit(2);
    g_base = (char *)p;
    Carve cv = {g_base, 0};
    lay(cv);
    if (cv.used != size.used) fail("sizing and carving pass disagree", -1);
}

static void self_test()
{
    int64_t *a; int32_t *b; char *c; double *d;
    carve([&](Carve &cv) { a = cv.take<int64_t>(3); b = cv.take<int32_t>(0); c = cv.take<char>(1); d = cv.take<double>(2); });
    if (g_used != 64 || (char *)a != g_base || (char *)b != (char *)c || (char *)a + 32 != c || c + 16 != (char *)d) fail("carver", -1);
    a[0] = a[2] = 1; c[0] = 2; d[0] = d[1] = 3.0;       // n = 0 took no bytes: nothing is written through b
    free(g_base);
    // a piece on a 64-byte boundary: the gap before it belongs to nobody, the piece itself is still a multiple of 16
    carve([&](Carve &cv) { c = cv.take<char>(1); d = cv.take<double>(1, 64); a = cv.take<int64_t>(1); });
    if (g_used != 96 || c != g_base || (char *)d != g_base + 64 || (char *)a != g_base + 80) fail("carver, 64-byte piece", -1);
    c[0] = 1; d[0] = 2.0; a[0] = 3;
    free(g_base);
}

struct Take { int size; int64_t n, align; char *p; };

static char *take_of(Carve &cv, const Take &t)
{
    switch (t.size) {
    case 1: return (char *)cv.take<char>(t.n, t.align);
    case 4: return (char *)cv.take<int32_t>(t.n, t.align);
    case 8: return (char *)cv.take<double>(t.n, t.align);
    case 16: return (char *)cv.take<E16>(t.n, t.align);
    default: return (char *)cv.take<E72>(t.n, t.align);
    }
}

static void random_layouts(unsigned seed, int layouts)
{
    std::mt19937 rng(seed);
    const int sizes[5] = {1, 4, 8, 16, 72};
    const int64_t counts[8] = {0, 1, 3, 5, 7, 64, 257, 1000};
    for (int l = 0; l < layouts; l++) {
        Take t[12];
        const int nt = 1 + (int)(rng() % 12);
        for (int i = 0; i < nt; i++) t[i] = {sizes[rng() % 5], counts[rng() % 8], (rng() & 1) ? 64 : 16, nullptr};
        carve([&](Carve &cv) { for (int i = 0; i < nt; i++) t[i].p = take_of(cv, t[i]); });
        char *end = g_base;                                 // the end of the last piece with bytes
        for (int i = 0; i < nt; i++) {
            const int64_t bytes = t[i].n * t[i].size;
            if ((size_t)t[i].p & (size_t)(t[i].align - 1)) fail("a piece is not aligned as asked", l);
            if (t[i].p < end) fail("pieces out of order or overlapping", l);
            if (t[i].p + bytes > g_base + g_used) fail("a piece ends beyond `used`", l);
            if (t[i].n == 0 && i + 1 < nt) {
                // no bytes: the next take starts where this one does - at the next boundary of its own alignment from there,
                // which is this very address unless it asks for 64 where this one asked for 16
                char *next = (char *)(((size_t)t[i].p + (size_t)(t[i + 1].align - 1)) & ~(size_t)(t[i + 1].align - 1));
                if (t[i + 1].p != next) fail("a zero-count take took bytes", l);
                if (t[i + 1].align <= t[i].align && t[i + 1].p != t[i].p) fail("a zero-count take does not share its address", l);
            }
            if (bytes) { memset(t[i].p, 0x5a + i, (size_t)bytes); end = t[i].p + bytes; }   // every byte, under ASan
        }
        // (the memsets did not run into each other: every piece still holds its own pattern)
        for (int i = 0; i < nt; i++)
            for (int64_t b = 0; b < t[i].n * t[i].size; b++)
                if (t[i].p[b] != (char)(0x5a + i)) fail("pieces share bytes", l);
        free(g_base);
    }
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "self")) { self_test(); return 0; }
    if (argc == 4 && !strcmp(argv[1], "random")) { random_layouts((unsigned)atoi(argv[2]), atoi(argv[3])); return 0; }
    return 2;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("scratch_carve")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])
    return exe


def test_carver_self_test(probe):
    """16-byte rounding, the n <= 0 rule, and a piece on a 64-byte boundary, at known offsets."""
    subprocess.run([probe, "self"], check=True)


def test_random_layouts_are_aligned_ordered_disjoint_and_writable(probe):
    """1000 seeded layouts of 1 to 12 takes: elements of 1, 4, 8, 16 and 72 bytes, counts 0, 1, 3, 5, 7, 64, 257, 1000,
    alignment 16 or 64 per take, over a heap buffer of exactly `used` bytes.  Every piece is aligned as asked, the pieces are
    in order and disjoint, the last ends within `used`, a zero-count take shares its address with the next take (which
    then moves on to its own boundary if it asks for a larger alignment), and every byte of every piece is written."""
    subprocess.run([probe, "random", "20261", "1000"], check=True)
