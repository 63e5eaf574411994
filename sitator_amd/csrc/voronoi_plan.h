// Every decision of VoronoiSiteGenerator (the periodic Voronoi nodes of the static lattice), written once for the kernels of
// voronoi.hip and for the host compiler (tests/test_voronoi_plan.py drives it with g++ under ASan / UBSan).  Compile without
// contraction (-ffp-contract=off): the error bounds below are the bounds of exactly these sequences of roundings.
//
// The contract.  Atoms are taken with all their periodic images.  A NODE is a sphere (c, r) with no atom image closer to c
// than r - tau and at least four atom images, not coplanar, within [r - tau, r + tau] of c; its vertices are the static
// indices of all atom images in that shell.  One degenerate sphere (8 atoms about the centre of a simple-cubic cube) is one
// node with all of its atoms.
//
// Coordinates.  Everything about atom i is computed in coordinates relative to p_i: a neighbour is q = (p_s + T(m)) - p_i,
// formed as -((p_i - p_s) - T(m)) with T(m) as in barrier_plan.h, so the magnitudes that enter the bounds are those of the
// search radius R, not of the cell.
//
// The sphere of a quadruple (i, a, b, c), u its centre relative to p_i:  2 q_k . u = |q_k|^2 for k = a, b, c, solved by
// Cramer's rule:
//     D = det [q_a; q_b; q_c]                        hp_det(q_a, q_b, q_c, 0): the differences with 0 are exact
//     w_k = (x x + y y) + z z
//     N = (w_a (q_b x q_c) + w_b (q_c x q_a)) + w_c (q_a x q_b),   every cross component a difference of two products
//     u = N / (2 D),   r = sqrt((u0 u0 + u1 u1) + u2 u2),   c = p_i + u.
// It is considered only when hp_orient3d certifies a non-zero sign (|D| > HP_BOUND_A * permanent) and
// |D| >= VP_SHAPE_MIN * permanent; rho = permanent / |D| is the shape number of the quadruple.
//
// Forward error of u (eps = 2^-53, hats: computed values, P_x: N_x with every term replaced by its magnitude).
//   w_k: three products and two sums of non-negative terms, relative error <= 3 eps.  A cross component C: each product eps,
//   the difference eps: |dC| <= 2 eps (|y z'| + |z y'|).  A product w C: eps more, so |d(w C)| <= 6 eps w pC.  The two sums: eps
//   of a partial sum each, <= 2 eps P_x.  Together |dN_x| <= 8 eps P_x (1 + O(eps)).
//   D: |dD| <= HP_BOUND_A * permanent = (7 + 56 eps) eps * permanent (hull_predicates.h).
//   u^ - u = dN / (2 D^) + u (D - D^) / D^ and one rounding of the quotient (2 D^ is exact):
//       |du_x| <= 8 eps P_x / |2 D^| + |u_x| 7 eps rho + eps |u_x|.
//   The header evaluates  e_x = eps (12 P_x / |2 D^| + (8 rho + 2) |u^_x|):  the constants 12, 8, 2 over 8, 7, 1 cover the
//   O(eps) factors, the roundings of P_x, rho and e_x themselves and |u_x| <= |u^_x| + e_x for every rho the shape floor admits.
//   ec = sqrt(e0^2 + e1^2 + e2^2) bounds |u^ - u|.  In terms of rho: P_x / |2 D^| = rho P_x / (2 permanent), so
//   ec <= eps rho (12 P / (2 permanent) + 10 |u|): the error is rho times a length of the order of the quadruple's size.
//   r^: the norm of u^ has relative error <= 3 eps, so |r^ - r| <= ec + 3 eps r^.
//   A neighbour's distance d^ = |q - u^|: three differences (eps each), the norm (3 eps): |d^ - d| <= ec + 4 eps d^.
//   A comparison of d with r -/+ tau therefore errs by at most  slack = 2 ec + 8 eps (d^ + r^ + tau)  (the 8 covers 3 + 4 and
//   the rounding of r^ -/+ tau).
//
// VP_SHAPE_MIN.  For the default tau = 1e-6 A, relative coordinates up to L = 64 A and quadruples whose magnitude centre
// P / (2 permanent) stays below 8 L (the atoms of a quadruple of a crystal are comparable in every coordinate; where they are
// not, e is large and the tests below answer uncertain - the floor is a filter, the certificate is e), the centre is good to
// tau / 16 when  eps rho (12 * 8 L + 10 L) <= tau / 16,  rho <= 6.25e-8 / (1.11e-16 * 106 * 64) = 8.3e4.  The floor is the next
// power of two below 1 / 8.3e4: VP_SHAPE_MIN = 2^-17.  Flatter quadruples are skipped; a degenerate node is still found from its
// other quadruples.  For a smaller tau or larger coordinates nothing changes but the number of uncertain answers.
//
// Membership of a neighbour at distance d: inside (d < r - tau), on (|d - r| <= tau), outside (d > r + tau), each certified
// against `slack`; a comparison within slack of its threshold answers VM_UNCERTAIN and nothing is decided from it.
//
// Completeness of atom i at search radius R (its neighbours: all atom images within R).
//   (a) Every open octant about p_i (all three coordinates of q non-zero, by sign) holds a neighbour.  Then the cell clipped by
//       the neighbours is bounded: a direction v of an unbounded clipped cell has v . q <= 0 for every neighbour q (the cell
//       contains the ray p_i + t v, so each bisector half space does).  Take the octant of v's signs (a zero of v taken as +):
//       its neighbour q has v_k q_k >= 0 for every k, and > 0 where v_k != 0 because no q_k is 0.  v is not 0, so v . q > 0:
//       a contradiction.
//   (b) No sphere through p_i that is empty of the neighbours has r > R / 2.  The vertices of the bounded clipped cell are
//       centres of such spheres, so the clipped cell lies within R / 2 of p_i; an atom beyond R has its bisector plane
//       beyond R / 2 and cannot cut it: the clipped cell is the cell, and every atom on a sphere of radius <= R / 2 through
//       p_i lies within R.  A sphere with r <= R / 2 empty of the R-neighbours is empty of all atoms.
//   r <= R / 2 is certified (r^ + its bound <= R / 2); anything else counts as far.  Spheres of skipped (flat) quadruples are not
//   looked at: that is not certified.
// Per-atom status: VS_OK; VS_GROW ((a) or (b) failed: run again at the plan's next R); VS_UNCERTAIN (a near sphere with no
// neighbour certified inside met an uncertain answer); VS_CAPACITY (neighbours, records, members, or R beyond the caps).
//
// Records.  An empty near sphere found from (i, a, b, c) with members M (the neighbours on it, a, b, c among them) is written
// once: only by the atom of lowest static index among its members (an own image counts as i), and only from the first triple
// of M, in enumeration order, that passes the shape floor.  Both rules drop copies the merge would unite anyway and keep the
// first record of every node where it was.  Enumeration order: atoms ascending; triples a < b < c of the neighbour list
// lexicographic; the list ordered by (squared distance, static index, image m0, m1, m2).  The kernel compacts by prefix sums in
// that order: nothing depends on arrival, two calls return the same bytes.
//
// Merge (host, vp_merge).  Two records are one node when their wrapped centres are within mu = 16 tau under the minimum image;
// the relation is closed transitively.  A node takes the place and the centre of its first record, its vertices are the union.
// A pair of centres between mu and 4 mu apart makes the clustering ambiguous: VS_UNCERTAIN for the call.  Pairs are found over
// a periodic grid of bins at least 4 mu high; 8 mu must stay below the smallest height of the cell.
//
// LDS of the sphere kernel: the neighbours' relative positions and static indices, VP_LDS_BYTES (7 KiB of the 160 KiB of a
// gfx950 CU): occupancy is bounded by registers, not LDS.  One workgroup of VP_BLOCK threads per atom.
#pragma once

#include <math.h>
#include <stdint.h>

#include "hull_predicates.h"
#include "barrier_plan.h"

#define VP_HD HP_HD

#define VP_BLOCK 256                                   // threads of a workgroup: one workgroup per atom
#define VP_NBR_CAP 256                                 // neighbours of an atom (one per thread in the sort)
#define VP_REC_CAP 128                                 // records of an atom
#define VP_MEMBER_CAP 32                               // atom images on one sphere, the atom itself included
#define VP_PAIR_FOUND 2                                // records one pair (a, b) can give: a triangle lies on two empty spheres
#define VP_R0_FACTOR 2.125                             // first R = this * (volume / atoms)^(1/3): past the 4th shell of SC, BCC and FCC
#define VP_GROWTH 1.3                                  // R of round k + 1 = R of round k * this
#define VP_MAX_ROUNDS 12
#define VP_SHAPE_MIN (1.0 / 131072.0)                  // 2^-17
#define VP_MU_FACTOR 16.0                              // mu = this * tau
#define VP_LDS_BYTES (VP_NBR_CAP * (3 * 8 + 4) + 64)

#define VS_OK 0
#define VS_GROW 1
#define VS_UNCERTAIN 2
#define VS_CAPACITY 3

#define VM_UNCERTAIN 0
#define VM_INSIDE 1
#define VM_ON 2
#define VM_OUTSIDE 3

#define VC_SKIP 0                                      // flat or uncertain orientation: not considered
#define VC_REJECT 1                                    // a neighbour is certified inside
#define VC_FAR 2                                       // no neighbour certified inside, r not certified <= R / 2
#define VC_DUP 3                                       // an empty near sphere another triple or atom records
#define VC_RECORD 4
#define VC_UNCERTAIN 5
#define VC_CAPACITY 6                                  // more than VP_MEMBER_CAP atom images on the sphere

struct VpSphere {
    double u[3];                                       // centre relative to the atom
    double r;
    double ec;                                         // bound of |u^ - u|
    double rho;                                        // permanent / |D|
};

struct VpRecord {
    double c[3];                                       // p_i + u, not wrapped
    double r;
    int32_t n;                                         // members, the atom itself first
    int32_t atom;
    int32_t m[VP_MEMBER_CAP];                          // static indices
};

// |D| certified non-zero and above the shape floor
VP_HD inline bool vp_shape_ok(const double qa[3], const double qb[3], const double qc[3], double *det, double *permanent)
{
    const double o[3] = {0.0, 0.0, 0.0};
    *det = hp_det(qa, qb, qc, o, permanent);
    if (!(fabs(*det) > HP_BOUND_A * *permanent)) return false;     // uncertain sign, an exact 0, a NaN
    return fabs(*det) >= VP_SHAPE_MIN * *permanent;
}

VP_HD inline bool vp_sphere(const double qa[3], const double qb[3], const double qc[3], VpSphere &s)
{
    double det, permanent;
    if (!vp_shape_ok(qa, qb, qc, &det, &permanent)) return false;
    const double wa = (qa[0] * qa[0] + qa[1] * qa[1]) + qa[2] * qa[2];
    const double wb = (qb[0] * qb[0] + qb[1] * qb[1]) + qb[2] * qb[2];
    const double wc = (qc[0] * qc[0] + qc[1] * qc[1]) + qc[2] * qc[2];
    const double den = 2.0 * det, aden = fabs(den);
    s.rho = permanent / fabs(det);
    double e2 = 0.0;
    for (int x = 0; x < 3; x++) {
        const int y = (x + 1) % 3, z = (x + 2) % 3;
        const double bc1 = qb[y] * qc[z], bc2 = qb[z] * qc[y];
        const double ca1 = qc[y] * qa[z], ca2 = qc[z] * qa[y];
        const double ab1 = qa[y] * qb[z], ab2 = qa[z] * qb[y];
        const double N = (wa * (bc1 - bc2) + wb * (ca1 - ca2)) + wc * (ab1 - ab2);
        const double P = (wa * (fabs(bc1) + fabs(bc2)) + wb * (fabs(ca1) + fabs(ca2))) + wc * (fabs(ab1) + fabs(ab2));
        s.u[x] = N / den;
        const double e = HP_EPS * (12.0 * (P / aden) + (8.0 * s.rho + 2.0) * fabs(s.u[x]));
        e2 += e * e;
    }
    s.r = sqrt((s.u[0] * s.u[0] + s.u[1] * s.u[1]) + s.u[2] * s.u[2]);
    s.ec = sqrt(e2) * (1.0 + 8.0 * HP_EPS);
    return s.r < INFINITY && s.ec < INFINITY;
}

VP_HD inline double vp_distance(const double q[3], const VpSphere &s)
{
    const double d0 = q[0] - s.u[0], d1 = q[1] - s.u[1], d2 = q[2] - s.u[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

VP_HD inline double vp_slack(double d, const VpSphere &s, double tau) { return 2.0 * s.ec + 8.0 * HP_EPS * ((d + s.r) + tau); }

// inside / on / outside for a distance d, certified against slack; anything else (a NaN too) is uncertain
VP_HD inline int vp_classify(double d, double r, double tau, double slack)
{
    if (d < (r - tau) - slack) return VM_INSIDE;
    if (d > (r + tau) + slack) return VM_OUTSIDE;
    if (fabs(d - r) <= tau - slack) return VM_ON;
    return VM_UNCERTAIN;
}

// r certified <= R / 2
VP_HD inline bool vp_near(const VpSphere &s, double R) { return (s.r + s.ec) + 4.0 * HP_EPS * s.r <= 0.5 * R; }

// the open octant of q: bit 0 x < 0, bit 1 y < 0, bit 2 z < 0; -1 on a coordinate plane (or a NaN)
VP_HD inline int vp_octant(const double q[3])
{
    int o = 0;
    for (int k = 0; k < 3; k++) {
        if (q[k] < 0.0) o |= 1 << k;
        else if (!(q[k] > 0.0)) return -1;
    }
    return o;
}

// One triple (a < b < c) of the neighbour list q[n][3] / sid[n] of atom `self` at p: what becomes of its sphere.  out (may be
// null) is written for VC_RECORD.
VP_HD inline int vp_candidate(const double *q, const int32_t *sid, int n, int32_t self, const double p[3], int a, int b, int c,
                              double R, double tau, VpRecord *out)
{
    VpSphere s;
    if (!vp_sphere(q + 3 * a, q + 3 * b, q + 3 * c, s)) return VC_SKIP;
    int members[VP_MEMBER_CAP];
    int nm = 0, uncertain = 0, overflow = 0;
    for (int k = 0; k < n; k++) {
        int ans = VM_ON;                                             // a, b, c: on by construction
        if (k != a && k != b && k != c) {
            const double d = vp_distance(q + 3 * k, s);
            ans = vp_classify(d, s.r, tau, vp_slack(d, s, tau));
        }
        if (ans == VM_INSIDE) return VC_REJECT;
        if (ans == VM_UNCERTAIN) uncertain = 1;
        else if (ans == VM_ON) {
            if (nm < VP_MEMBER_CAP - 1) members[nm++] = k;
            else overflow = 1;
        }
    }
    if (!vp_near(s, R)) return VC_FAR;
    if (uncertain) return VC_UNCERTAIN;
    if (overflow) return VC_CAPACITY;
    for (int j = 0; j < nm; j++)
        if (sid[members[j]] < self) return VC_DUP;                   // the member of lowest static index records it
    for (int x = 0; x < nm; x++)                                     // the first triple of the members that passes the floor
        for (int y = x + 1; y < nm; y++)
            for (int z = y + 1; z < nm; z++) {
                const int ma = members[x], mb = members[y], mc = members[z];
                if (ma == a && mb == b && mc == c) goto first;
                double det, permanent;
                if (vp_shape_ok(q + 3 * ma, q + 3 * mb, q + 3 * mc, &det, &permanent)) return VC_DUP;
            }
first:
    if (out) {
        for (int k = 0; k < 3; k++) out->c[k] = p[k] + s.u[k];
        out->r = s.r;
        out->n = nm + 1;
        out->atom = self;
        out->m[0] = self;
        for (int j = 0; j < nm; j++) out->m[1 + j] = sid[members[j]];
        for (int j = nm + 1; j < VP_MEMBER_CAP; j++) out->m[j] = -1;
    }
    return VC_RECORD;
}

// the key of the neighbour order: (squared distance, static index, m0, m1, m2)
struct VpKey {
    double d2;
    int32_t s, m[3];
};

VP_HD inline bool vp_key_less(const VpKey &x, const VpKey &y)
{
    if (x.d2 != y.d2) return x.d2 < y.d2;
    if (x.s != y.s) return x.s < y.s;
    if (x.m[0] != y.m[0]) return x.m[0] < y.m[0];
    if (x.m[1] != y.m[1]) return x.m[1] < y.m[1];
    return x.m[2] < y.m[2];
}

// the image of atom s by m relative to atom i: q = -((p_i - p_s) - T(m)), and its squared length
template <class P> VP_HD inline double vp_relative(const P &c, const double pi[3], const double ps[3], int m0, int m1, int m2, double q[3])
{
    const double t0 = ((double)m0 * c.cm[0] + (double)m1 * c.cm[1]) + (double)m2 * c.cm[2];
    const double t1 = ((double)m0 * c.cm[3] + (double)m1 * c.cm[4]) + (double)m2 * c.cm[5];
    const double t2 = ((double)m0 * c.cm[6] + (double)m1 * c.cm[7]) + (double)m2 * c.cm[8];
    const double d0 = (pi[0] - ps[0]) - t0, d1 = (pi[1] - ps[1]) - t1, d2 = (pi[2] - ps[2]) - t2;
    q[0] = -d0; q[1] = -d1; q[2] = -d2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// |det| of the cell
template <class P> VP_HD inline double vp_volume(const P &c)
{
    const double d = c.cm[0] * (c.cm[4] * c.cm[8] - c.cm[5] * c.cm[7]) - c.cm[1] * (c.cm[3] * c.cm[8] - c.cm[5] * c.cm[6])
                     + c.cm[2] * (c.cm[3] * c.cm[7] - c.cm[4] * c.cm[6]);
    return fabs(d);
}

// the search radius of round k (0: from the atom density)
VP_HD inline double vp_radius(double volume, int64_t S, int round)
{
    double R = VP_R0_FACTOR * cbrt(volume / (double)S);
    for (int k = 0; k < round; k++) R *= VP_GROWTH;
    return R;
}

// the status of an atom from what its round found
VP_HD inline int vp_status(int nbr_over_cap, int capacity, int octants, int n_far, int uncertain)
{
    if (nbr_over_cap || capacity) return VS_CAPACITY;
    if (octants != 0xFF || n_far > 0) return VS_GROW;
    if (uncertain) return VS_UNCERTAIN;
    return VS_OK;
}

#include <vector>

// Records [n] with wrapped centres w[n][3] into nodes: node[k] = the node of record k, numbered in the order of their first
// records; first[j] = the first record of node j.  Returns VS_OK, VS_UNCERTAIN (a pair of centres between mu and 4 mu apart) or
// VS_CAPACITY (8 mu is not below the smallest height of the cell: the bins cannot tell the images apart).
template <class P> inline int vp_merge(const P &c, const double *w, int64_t n, double mu, std::vector<int64_t> &node, std::vector<int64_t> &first)
{
    node.assign((size_t)n, -1);
    first.clear();
    if (n == 0) return VS_OK;
    int G[3];
    double hmin = INFINITY;
    for (int a = 0; a < 3; a++) {
        const double h = 1.0 / sqrt((c.ci[3 * a] * c.ci[3 * a] + c.ci[3 * a + 1] * c.ci[3 * a + 1]) + c.ci[3 * a + 2] * c.ci[3 * a + 2]);
        if (h < hmin) hmin = h;
        const double g = floor(h / (4.0 * mu));
        G[a] = g >= 64.0 ? 64 : (g >= 1.0 ? (int)g : 1);
    }
    if (!(8.0 * mu < hmin)) return VS_CAPACITY;
    std::vector<double> f((size_t)(3 * n));
    std::vector<int64_t> bin((size_t)n), start((size_t)(G[0] * G[1] * G[2]) + 1, 0), order((size_t)n), parent((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        double b[3];
        cp_to_cell(c, w + 3 * k, b);
        int g[3];
        for (int a = 0; a < 3; a++) {
            b[a] -= floor(b[a]);
            f[(size_t)(3 * k + a)] = b[a];
            g[a] = (int)(b[a] * (double)G[a]);
            if (g[a] >= G[a]) g[a] = G[a] - 1;
            if (g[a] < 0) g[a] = 0;
        }
        bin[(size_t)k] = ((int64_t)g[0] * G[1] + g[1]) * G[2] + g[2];
        start[(size_t)bin[(size_t)k] + 1]++;
        parent[(size_t)k] = k;
    }
    for (size_t b = 1; b < start.size(); b++) start[b] += start[b - 1];
    {
        std::vector<int64_t> cur(start.begin(), start.end() - 1);
        for (int64_t k = 0; k < n; k++) order[(size_t)cur[(size_t)bin[(size_t)k]]++] = k;       // ascending inside a bin
    }
    auto find = [&](int64_t x) {
        while (parent[(size_t)x] != x) { parent[(size_t)x] = parent[(size_t)parent[(size_t)x]]; x = parent[(size_t)x]; }
        return x;
    };
    int ambiguous = 0;
    for (int64_t k = 0; k < n; k++) {
        const int64_t bk = bin[(size_t)k];
        const int g[3] = {(int)(bk / ((int64_t)G[1] * G[2])), (int)(bk / G[2] % G[1]), (int)(bk % G[2])};
        int nb[3][3], nn[3];
        for (int a = 0; a < 3; a++) {                                // the distinct bins of {g - 1, g, g + 1} mod G
            nn[a] = 0;
            for (int o = -1; o <= 1; o++) {
                const int v = ((g[a] + o) % G[a] + G[a]) % G[a];
                bool seen = false;
                for (int j = 0; j < nn[a]; j++) seen = seen || nb[a][j] == v;
                if (!seen) nb[a][nn[a]++] = v;
            }
        }
        for (int i0 = 0; i0 < nn[0]; i0++)
            for (int i1 = 0; i1 < nn[1]; i1++)
                for (int i2 = 0; i2 < nn[2]; i2++) {
                    const int64_t b = ((int64_t)nb[0][i0] * G[1] + nb[1][i1]) * G[2] + nb[2][i2];
                    for (int64_t e = start[(size_t)b]; e < start[(size_t)b + 1]; e++) {
                        const int64_t j = order[(size_t)e];
                        if (j >= k) break;
                        double df[3], d[3];
                        for (int a = 0; a < 3; a++) {
                            df[a] = f[(size_t)(3 * k + a)] - f[(size_t)(3 * j + a)];
                            df[a] -= nearbyint(df[a]);
                        }
                        cp_to_real(c, df, d);
                        const double dist = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                        if (dist <= mu) {
                            const int64_t rk = find(k), rj = find(j);
                            if (rk < rj) parent[(size_t)rj] = rk;
                            else if (rj < rk) parent[(size_t)rk] = rj;
                        } else if (dist <= 4.0 * mu) ambiguous = 1;
                    }
                }
    }
    for (int64_t k = 0; k < n; k++) {
        const int64_t r = find(k);                                   // the lowest record of the class: r <= k
        if (r == k) { node[(size_t)k] = (int64_t)first.size(); first.push_back(k); }
        else node[(size_t)k] = node[(size_t)r];
    }
    return ambiguous ? VS_UNCERTAIN : VS_OK;
}
