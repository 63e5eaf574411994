// The decisions of the gift-wrapping convex hull of hull.hip (k_group_hull), in a form the host compiler takes too
// (tests/test_hull_predicates.py runs them with g++ under ASan / UBSan): the orientation test with its certificate, the
// selection rule of a pivot, the first-facet rule.  Must be compiled without contraction (-ffp-contract=off): the error
// bound below is the bound of exactly this sequence of roundings.
//
// orient3d.  D = det [a - q; b - q; c - q] = -(q - a) . ((b - a) x (c - a)), evaluated in double in the operation order of
// Shewchuk's orient3d ("Adaptive Precision Floating-Point Arithmetic and Fast Robust Geometric Predicates", 1997, stage A):
// three differences per point, six products, three differences of products, three products, two sums.  His bound A for
// that sequence: |computed - exact| <= (7 + 56 eps) eps * permanent, eps = 2^-53, where the permanent is the same
// expression with every term replaced by its magnitude (computed in double as well; the 56 eps cover its own roundings).
// Underflow is not covered: coordinates here are Angstrom of the order 1..100.
//
// A test answers HP_POS (q lies strictly on the side the normal (b - a) x (c - a) points to: D < -bound), HP_NEG (strictly
// on the other side: D > bound) or HP_UNCERTAIN (|D| <= bound, which includes an exact 0, and anything with a NaN).  A
// certified answer is the sign of the exact determinant; nothing is ever decided from an uncertain one.
//
// Facets (a, b, c) are kept with their normal pointing out of the hull: no point is HP_POS.  The volume term of a facet
// against the hull's first vertex p0 is D(a, b, c, p0) / 6 >= 0.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define HP_HD __host__ __device__
#else
#define HP_HD
#endif

#define HP_POS 1
#define HP_NEG (-1)
#define HP_UNCERTAIN 0

#define HP_NONE 0xFFFFFFFFu                            // no point (an empty candidate)
#define HP_EPS 1.1102230246251565e-16                  // 2^-53
#define HP_BOUND_A ((7.0 + 56.0 * HP_EPS) * HP_EPS)

// D and its permanent
HP_HD inline double hp_det(const double a[3], const double b[3], const double c[3], const double q[3], double *permanent)
{
    const double adx = a[0] - q[0], bdx = b[0] - q[0], cdx = c[0] - q[0];
    const double ady = a[1] - q[1], bdy = b[1] - q[1], cdy = c[1] - q[1];
    const double adz = a[2] - q[2], bdz = b[2] - q[2], cdz = c[2] - q[2];
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy;
    const double cdxady = cdx * ady, adxcdy = adx * cdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady;
    const double det = adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy) + cdz * (adxbdy - bdxady);
    *permanent = (fabs(bdxcdy) + fabs(cdxbdy)) * fabs(adz) + (fabs(cdxady) + fabs(adxcdy)) * fabs(bdz)
                 + (fabs(adxbdy) + fabs(bdxady)) * fabs(cdz);
    return det;
}

HP_HD inline int hp_orient3d(const double a[3], const double b[3], const double c[3], const double q[3])
{
    double permanent;
    const double det = hp_det(a, b, c, q, &permanent);
    const double bound = HP_BOUND_A * permanent;
    if (det > bound) return HP_NEG;
    if (-det > bound) return HP_POS;
    return HP_UNCERTAIN;                               // |det| <= bound, or a NaN
}

// the same point (callers skip it instead of testing it: its determinant is an exact 0 by construction, not by geometry)
HP_HD inline bool hp_same(const double p[3], const double q[3]) { return p[0] == q[0] && p[1] == q[1] && p[2] == q[2]; }

// lexicographic order of the coordinates, exact
HP_HD inline bool hp_lex_less(const double p[3], const double q[3])
{
    if (p[0] != q[0]) return p[0] < q[0];
    if (p[1] != q[1]) return p[1] < q[1];
    return p[2] < q[2];
}

// A candidate of a reduction: a point of the site (its index i, HP_NONE: none yet, and its coordinates), and whether an
// uncertain test was met on the way to it.  The flag is sticky: it survives every later merge.
struct HpCand {
    uint32_t i;
    int uncertain;
    double p[3];
};

HP_HD inline HpCand hp_none()
{
    HpCand c;
    c.i = HP_NONE; c.uncertain = 0; c.p[0] = c.p[1] = c.p[2] = 0.0;
    return c;
}

HP_HD inline HpCand hp_point(uint32_t i, const double p[3])
{
    HpCand c;
    c.i = i; c.uncertain = 0; c.p[0] = p[0]; c.p[1] = p[1]; c.p[2] = p[2];
    return c;
}

// The first vertex: the lexicographically least point, of equal points the one of lowest index.
HP_HD inline HpCand hp_pick_least(const HpCand &c, const HpCand &q)
{
    if (q.i == HP_NONE) return c;
    if (c.i == HP_NONE) return q;
    if (hp_same(c.p, q.p)) return q.i < c.i ? q : c;
    return hp_lex_less(q.p, c.p) ? q : c;
}

// The selection rule of a pivot about the directed edge (a, b): of two candidates the one the other is not HP_POS of, so
// that the winner w of a whole site leaves no point on the positive side of (a, b, w).  Of equal points the lower index
// stays: a vertex has one name.  Both arguments are points other than a and b (the caller skips those).  About a hull
// edge all points lie in a wedge of less than 180 degrees, on which "q is HP_POS of (a, b, c)" is a strict total order of
// the directions: with certified signs the winner does not depend on the order of the merges.
HP_HD inline HpCand hp_pick(const double a[3], const double b[3], const HpCand &c, const HpCand &q)
{
    HpCand r = c;
    if (q.i == HP_NONE) return r;
    if (c.i == HP_NONE) r = q;
    else if (hp_same(c.p, q.p)) { if (q.i < c.i) r = q; }
    else {
        const int s = hp_orient3d(a, b, c.p, q.p);
        if (s == HP_POS) r = q;
        else if (s == HP_UNCERTAIN) r.uncertain = 1;
    }
    r.uncertain |= c.uncertain | q.uncertain;
    return r;
}

// First facet.  a = hp_pick_least over the site.  b = the pivot about the virtual edge (a, a + (0, 1, 0)): a is the least
// point, so every other point lies in the half space x >= a.x and the plane through that edge can be turned until no
// point is on its positive side.  (Points exactly above or below a in the plane x = a.x give an exact 0: uncertain.)
// c = the pivot about (a, b): by the selection rule no point is HP_POS of (a, b, c), the facet looks outwards as it is.
HP_HD inline void hp_virtual_second(const double a[3], double v[3])
{
    v[0] = a[0]; v[1] = a[1] + 1.0; v[2] = a[2];
}
