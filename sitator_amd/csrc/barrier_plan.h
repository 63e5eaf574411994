// Every decision of MergeSitesByBarrier's energy evaluation (network/MergeSitesByBarrier.py:103-125 with a truncated and shifted
// 12-6 potential as the calculator), written once for the kernels of barrier.hip and for the host compiler
// (tests/test_barrier_plan.py drives it with g++ under ASan / UBSan).  Compile without contraction (-ffp-contract=off): the pair
// term, the driven point and the squared distance are compared bit for bit with tests/barrier_ref.py.
//
// What is summed.  The energy of ONE mobile atom at x in a frozen lattice of S atoms under periodic boundaries,
//     E(x) = sum over atoms s and integer triples m with d2 <= rc2 of phi_s(d2),
//     d = (x - s) - T(m),  T(m)[k] = (m0 cell[0][k] + m1 cell[1][k]) + m2 cell[2][k],  d2 = (d0 d0 + d1 d1) + d2 d2,
//     s6 = (sig2 / d2)^3 as (q q) q,  phi = (eps4 s6)(s6 - 1) - e0,  eps4 = 4 eps,  sig2 = sigma sigma,  e0 = the same at d2 = rc rc.
// No root, no pow.  d2 = 0 gives q = inf and phi = +inf, never NaN.  Every (s, m) is a term of its own, so d2 and the cutoff
// test are the same bits whoever enumerates the triples; only the order of the sum differs between two complete enumerations.
//
// Which triples.  frac(d) = g - m with g = ci (x) - ci (s), and |d| >= |g_a - m_a| h_a for every axis a, h_a the perpendicular
// height of the cell along a.  So a term within rc has |g_a - m_a| <= q_a = rc / h_a on every axis.  g_a is brought into the
// cell, r = g_a - floor(g_a) in [0, 1], and m_a = floor(g_a) + t: then -q_a <= t <= 1 + q_a, which |t| <= n_a = floor(q_a) + 1
// covers whatever the cell's shape, wherever x and s lie.  The plan holds n_a (with q_a widened by BP_SLACK before the floor,
// for the rounding of q_a itself); per atom the kernel walks the t with |r - t| <= q_a + slack only, clamped to the plan's range,
// which bounds every loop.  The slack (1e-9 cell units, scaled by 1 + |g_a|) is far above the rounding of g_a for the inputs
// the entry point admits (|crystal coordinate| <= BP_MAX_FRAC) and admits only triples whose d2 the cutoff test then refuses.
//
// The order of the sum (barrier.hip): the atoms in tiles of BP_TILE, inside a tile lane l of a wave takes the atoms l, l + 64,
// ... in turn and for each its triples with m0 outermost and m2 innermost, ascending; the 64 lane sums meet in a butterfly
// (xor 32, 16, ..., 1); the tile sums are added in tile order.  Nothing depends on arrival.
//
// LDS per workgroup: one tile of BP_TILE records of BP_REC doubles (36 864 bytes) and the path of the pair: BP_LDS_BYTES, of the
// 160 KiB of a gfx950 CU.  Four workgroups (16 waves) of a CU fit.  A record's stride of 72 bytes keeps the 32 lanes of a
// half wave on 32 distinct bank pairs.
#pragma once

#include <stdint.h>

#include "clamp_point.h"

#define BP_HD CP_HD

#define BP_BLOCK 256                                   // threads of a workgroup: one workgroup per candidate pair
#define BP_WAVE 64
#define BP_WAVES (BP_BLOCK / BP_WAVE)
#define BP_TILE 512                                    // static atoms staged at once
#define BP_REC 9                                       // doubles of a staged atom: pos[3], crystal[3], eps4, sig2, e0
#define BP_LDS_BYTES (BP_TILE * BP_REC * 8 + 48)       // the tile and the path of the pair
#define BP_MAX_SITES 16384
#define BP_MAX_RANGE 256                               // translations per axis and sign the plan admits (rc / h_a below 255)
#define BP_MAX_FRAC 1048576.0                          // |crystal coordinate| of an atom or a centre the entry point admits
#define BP_SLACK 1e-9

struct BarrierPlan {
    int n[3];                                          // |t_a| <= n[a]
    double q[3];                                       // rc / h_a, h_a the perpendicular height along cell vector a
    double rc2;
};

// The plan of a cell given as cm = cell.T (row-major, cm[3 k + j] = cell[j][k]) and a cutoff.  h_a = |det| / |a_b x a_c|.
// false: a degenerate cell, rc not positive, or more than BP_MAX_RANGE translations along an axis.
template <class P> BP_HD inline bool bp_plan(const P &c, double rc, BarrierPlan &pl)
{
    double a[3][3];
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) a[j][k] = c.cm[3 * k + j];
    double cr[3][3];                                   // cr[a] = a_b x a_c, (a, b, c) cyclic
    for (int i = 0; i < 3; i++) {
        const int b = (i + 1) % 3, d = (i + 2) % 3;
        cr[i][0] = a[b][1] * a[d][2] - a[b][2] * a[d][1];
        cr[i][1] = a[b][2] * a[d][0] - a[b][0] * a[d][2];
        cr[i][2] = a[b][0] * a[d][1] - a[b][1] * a[d][0];
    }
    const double det = a[0][0] * cr[0][0] + a[0][1] * cr[0][1] + a[0][2] * cr[0][2];
    pl.rc2 = rc * rc;
    if (!(rc > 0.0) || !(fabs(det) > 0.0) || !(pl.rc2 < INFINITY)) return false;
    for (int i = 0; i < 3; i++) {
        const double area = sqrt(cr[i][0] * cr[i][0] + cr[i][1] * cr[i][1] + cr[i][2] * cr[i][2]);
        pl.q[i] = rc / (fabs(det) / area);
        if (!(pl.q[i] < (double)(BP_MAX_RANGE - 1))) return false;
        pl.n[i] = (int)floor(pl.q[i] * (1.0 + BP_SLACK) + BP_SLACK) + 1;
    }
    return true;
}

// The integers m of one axis with |g - m| <= q (and a slack): [*lo, *hi], at most 2 n + 1 of them; empty for a g beyond
// BP_MAX_FRAC cells (the entry point refuses such input).
BP_HD inline void bp_axis_range(double g, double q, int n, int *lo, int *hi)
{
    *lo = 1; *hi = 0;
    if (!(fabs(g) <= 4.0 * BP_MAX_FRAC)) return;
    const double base = floor(g), r = g - base;
    const double w = q + BP_SLACK * (1.0 + fabs(g));
    double tl = ceil(r - w), th = floor(r + w);
    if (tl < (double)-n) tl = (double)-n;
    if (th > (double)n) th = (double)n;
    *lo = (int)base + (int)tl;
    *hi = (int)base + (int)th;
}

// the unshifted 12-6 term at squared distance d2
BP_HD inline double bp_lj(double d2, double sig2, double eps4)
{
    const double q = sig2 / d2;
    const double s6 = (q * q) * q;
    return (eps4 * s6) * (s6 - 1.0);
}

BP_HD inline double bp_phi(double d2, double sig2, double eps4, double e0) { return bp_lj(d2, sig2, eps4) - e0; }

// the record of a static atom: rec[0..2] position as given, [3..5] its crystal coordinates (not wrapped), [6] 4 eps,
// [7] sigma^2, [8] e0
template <class P> BP_HD inline void bp_atom(const P &c, const double pos[3], double eps, double sigma, double rc, double rec[BP_REC])
{
    for (int k = 0; k < 3; k++) rec[k] = pos[k];
    cp_to_cell(c, pos, rec + 3);
    rec[6] = 4.0 * eps;
    rec[7] = sigma * sigma;
    rec[8] = bp_lj(rc * rc, rec[7], rec[6]);
}

// MergeSitesByBarrier.py:110-112: positions[-1] = vector; *= coeff; += pos[i] - the product first, then the sum
BP_HD inline void bp_driven(const double from[3], const double vector[3], double coeff, double x[3])
{
    for (int k = 0; k < 3; k++) {
        const double scaled = vector[k] * coeff;
        x[k] = scaled + from[k];
    }
}

// what the atom of `rec` and all its periodic images contribute at x (fx: the crystal coordinates of x, not wrapped)
template <class P> BP_HD inline double bp_atom_energy(const P &c, const BarrierPlan &pl, const double *rec, const double x[3],
                                                     const double fx[3])
{
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {                      // most atoms of a large cell leave at the first axis
        bp_axis_range(fx[a] - rec[3 + a], pl.q[a], pl.n[a], &lo[a], &hi[a]);
        if (lo[a] > hi[a]) return 0.0;
    }
    const double b0 = x[0] - rec[0], b1 = x[1] - rec[1], b2 = x[2] - rec[2];
    double e = 0.0;
    for (int m0 = lo[0]; m0 <= hi[0]; m0++)
        for (int m1 = lo[1]; m1 <= hi[1]; m1++)
            for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                const double t0 = ((double)m0 * c.cm[0] + (double)m1 * c.cm[1]) + (double)m2 * c.cm[2];
                const double t1 = ((double)m0 * c.cm[3] + (double)m1 * c.cm[4]) + (double)m2 * c.cm[5];
                const double t2 = ((double)m0 * c.cm[6] + (double)m1 * c.cm[7]) + (double)m2 * c.cm[8];
                const double d0 = b0 - t0, d1 = b1 - t1, d2 = b2 - t2;
                const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                if (dd <= pl.rc2) e += bp_phi(dd, rec[7], rec[6], rec[8]);
            }
    return e;
}

// MergeSitesByBarrier.py:116-125 on the n image energies of a pair: v[0] the first maximum (np.argmax) is neither end,
// v[1] forward barrier <= threshold, v[2] backward barrier <= threshold (a comparison with NaN, inf - inf, is false)
BP_HD inline void bp_verdict(const double *e, int n, double threshold, uint8_t v[3])
{
    int k = 0;
    for (int i = 1; i < n; i++)
        if (e[i] > e[k]) k = i;
    const double forward = e[k] - e[0], backward = e[k] - e[n - 1];
    v[0] = (uint8_t)(k != 0 && k != n - 1);
    v[1] = (uint8_t)(forward <= threshold);
    v[2] = (uint8_t)(backward <= threshold);
}
