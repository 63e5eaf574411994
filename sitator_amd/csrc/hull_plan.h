// The plan of k_group_hull (hull.hip) in a form the host compiler takes too (tests/test_hull_predicates.py drives it with
// g++ under ASan / UBSan): capacities, the LDS layout of a workgroup, the statuses, and the bookkeeping of the wrap - the
// list of open directed edges and the counts that decide whether a hull closed.  The geometry is in hull_predicates.h.
//
// The wrap.  A facet (u, v, w) has the directed edges u->v, v->w, w->u; the facet on the other side of an edge has its
// reverse.  The list holds the directed edges still WANTED: after the first facet (a, b, c) these are b->a, c->b, a->c.
// A step takes the last entry u->v off the list, the pivot about (u, v) gives w, and of the new facet's other two edges
// v->w and w->u each is either on the list already (some earlier facet wanted it: the entry leaves) or its reverse is put
// on.  The hull closed when the list is empty.  Every wanted edge was then met by exactly one facet; a directed edge that
// two facets have, which only wrong signs produce, leaves more facets than F = 2 V - 4 (Euler: V - E + F = 2 with
// E = 3 F / 2) and is reported as HS_OPEN.
//
// Capacities.  HP_FACET_CAP = 2048 facets.  Measured on clouds of 20 000 points: 112 facets (Gaussian), 250 (uniform in a
// cube); the test suite's shell of 600 points has 1196.  2048 is the next power of two above that shell and 8 times the
// largest count of a real-shaped cloud.  A step adds one facet, so HP_FACET_CAP also bounds the steps of a site: the kernel
// ends after at most HP_FACET_CAP pivots of at most `len` tests per lane each, whatever the predicates answer.  The wanted
// edges are the boundary of the facets found so far; a triangulated disc of f facets has at most f + 2 boundary edges, so
// HP_OPEN_CAP = HP_FACET_CAP + 2 never binds before the facet capacity does on a valid hull.  Appending is checked anyway.
//
// LDS per workgroup: the list (HP_OPEN_CAP x 2 x 4 bytes = 16 400), one candidate per wave (HP_WAVES x 32) and a few
// words: HP_LDS_BYTES below, about 16.2 KiB.  Of the 160 KiB of a gfx950 CU that allows 9 workgroups = 36 waves where the
// CU holds 32 at most: the list does not lower the occupancy the registers allow.
#pragma once

#include <stdint.h>

#define HP_BLOCK 256                                   // threads of a workgroup: one workgroup per site
#define HP_WAVE 64
#define HP_WAVES (HP_BLOCK / HP_WAVE)
#define HP_FACET_CAP 2048
#define HP_OPEN_CAP (HP_FACET_CAP + 2)
#define HP_MAX_POINTS 0xFFFFFFFEll                     // site-local indices are 32-bit words, 0xFFFFFFFF is "none"
#define HP_LDS_BYTES (HP_OPEN_CAP * 8 + HP_WAVES * 32 + 64)

// how a site ended
#define HS_CLOSED 0                                    // every wanted edge met, V - E + F = 2: the volume is a hull's
#define HS_FEW 1                                       // fewer than 4 points
#define HS_UNCERTAIN 2                                 // an uncertain predicate was met (or no candidate was left)
#define HS_CAPACITY 3                                  // facet or open-edge capacity exceeded
#define HS_OPEN 4                                      // the list ran empty but the counts are not a closed surface's

#ifdef __HIPCC__
#define HW_HD __host__ __device__
#else
#define HW_HD
#endif

struct HullEdge {
    uint32_t from, to;
};

// the state one thread keeps for a site
struct HullWrap {
    HullEdge *open;                                    // [HP_OPEN_CAP]
    int n_open;
    int n_facets, n_vertices;
    int overflow;
};

HW_HD inline void hw_init(HullWrap &w, HullEdge *open)
{
    w.open = open; w.n_open = 0; w.n_facets = 0; w.n_vertices = 0; w.overflow = 0;
}

HW_HD inline void hw_want(HullWrap &w, uint32_t from, uint32_t to)
{
    if (w.n_open >= HP_OPEN_CAP) { w.overflow = 1; return; }
    w.open[w.n_open].from = from; w.open[w.n_open].to = to;
    w.n_open++;
}

// the first position of the directed edge in list[lo, hi), -1: not there
HW_HD inline int hw_find(const HullEdge *list, int lo, int hi, uint32_t from, uint32_t to)
{
    for (int k = lo; k < hi; k++)
        if (list[k].from == from && list[k].to == to) return k;
    return -1;
}

// the first facet (a, b, c)
HW_HD inline void hw_first(HullWrap &w, uint32_t a, uint32_t b, uint32_t c)
{
    w.n_facets = 1;
    hw_want(w, b, a); hw_want(w, c, b); hw_want(w, a, c);
}

// the entry a step works on: the last one, taken off the list (n_open > 0)
HW_HD inline HullEdge hw_take(HullWrap &w)
{
    w.n_open--;
    return w.open[w.n_open];
}

// The facet (e.from, e.to, third) joins.  p1, p2: the first positions of e.to->third and third->e.from in the list as
// hw_take left it (-1: not there).  The larger position leaves first (its place goes to the last entry, which lies
// behind both), so the smaller one still names its edge; then the reverses of the edges not found are wanted, in this
// order.
HW_HD inline void hw_join(HullWrap &w, HullEdge e, uint32_t third, int p1, int p2)
{
    w.n_facets++;
    const int hi = p1 > p2 ? p1 : p2, lo = p1 > p2 ? p2 : p1;
    if (hi >= 0) { w.n_open--; w.open[hi] = w.open[w.n_open]; }
    if (lo >= 0) { w.n_open--; w.open[lo] = w.open[w.n_open]; }
    if (p1 < 0) hw_want(w, third, e.to);
    if (p2 < 0) hw_want(w, e.from, third);
}

// the status of a site whose list ran empty
HW_HD inline int hw_closed_status(const HullWrap &w)
{
    const int F = w.n_facets, V = w.n_vertices;
    return (F % 2 == 0 && V - 3 * (F / 2) + F == 2) ? HS_CLOSED : HS_OPEN;
}
