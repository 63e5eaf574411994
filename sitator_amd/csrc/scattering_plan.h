// Every decision of the intermediate scattering function (scattering.hip), in ONE place: the reduction of a fractional
// coordinate, the hand-written sine and cosine of 2 pi f, the power step and the term of an atom for a q vector, the blocks
// of a lag's origins (series_plan.h counts them), the order of every sum, the q batch, the frame window and the lags of a
// launch under a workspace cap, the tile of power tables and its LDS bytes, the validation, and - sc_layout(), the one place
// that names them - the pieces of a call's device buffer.  Host and device arithmetic only: no HIP call, no context, no side
// effect (tests/test_scattering_plan.py compiles it with g++ under ASan / UBSan).  No fma and no library sine, cosine or
// exponential: every product and every sum below is one rounded float64 operation (-ffp-contract=off), which numpy repeats
// bit for bit (tests/scattering_ref.py).
//
// Definitions.  Cell rows c_0..c_2, ci = inverse(cell^T), q = 2 pi (h ci[0] + k ci[1] + l ci[2]):
//   phase     s_a = (ci[a][0] x + ci[a][1] y) + ci[a][2] z (msd_frac), f_a = s_a - nearbyint(s_a): NaN where s_a is not finite
//   E_a       (cos 2 pi f_a, sin 2 pi f_a) by sc_sincos2pi; P_0 = 1 (NaN where E is), P_m = E P_{m-1}, a negative index: the conjugate
//   term      (P^0_h P^1_k) P^2_l, each product by sc_cmul
//   rho_q(t)  the terms of a selection added one after the other in selection order, from +0
//   coherent  C(tau, q) = sum_t rho^b_q(t + tau) conj(rho^a_q(t)) over the origins t = 0, s, 2 s, .. while t + tau <= F - 1
//   self      S(tau, q) = sum_t sum_i term(d), d_a = f_a(t + tau) - f_a(t), d_a -= nearbyint(d_a); tau = 0: origins x n_a + 0i
//   order     origins are taken in blocks of SC_BLOCK by number; coherent: the products of a block are added by the tree of
//             sc_tree (origins beyond the last count as +0); self: the terms of a block are added one after the other, origin by
//             origin and within an origin in selection order, from +0; the blocks are added one after the other from +0
#pragma once
#include <math.h>
#include <stdint.h>

#include "scratch_carve.h"
#include "series_plan.h"

#define SC_THREADS 256                            // threads of a workgroup of every kernel: four waves
#define SC_MAX_H 32                               // the largest |h|, |k|, |l|
#define SC_MAX_Q ((int64_t)1 << 16)               // q vectors of a call
#define SC_MAX_QBATCH ((int64_t)1 << 15)          // q vectors held at once: grid.y of k_sc_coherent
#define SC_MAX_ATOMS ((int64_t)1 << 20)           // atoms of a list, as sit_vanhove
#define SC_MAX_F ((int64_t)1 << 29)               // as sit_msd
#define SC_BLOCK 128                              // origins of a block: one partial sum per (lag, block, q)
#define SC_QTILE SC_THREADS                       // q vectors of a workgroup of k_sc_density / k_sc_self: one per thread
#define SC_TILE_MAX 64                            // (frame, atom) entries whose power tables a workgroup stages at once
#define SC_TILE_LDS 24576                         // bytes the tables of a tile may take: six workgroups on a CU's 160 KB
#define SC_LAG_TILE 8                             // lags of a workgroup of k_sc_coherent
#define SC_RUN 32                                 // frames of a workgroup of k_sc_density
#define SC_MAX_LAGS_LAUNCH 65535                  // grid.z of k_sc_self
#define SC_MAX_FRAC ((int64_t)1 << 36)            // (frame, column) elements of one k_series_frac launch: 2^28 workgroups

// ---- the phase ----------------------------------------------------------------------------------------------------------

// s less the nearest whole number, ties to even: exact, in [-1/2, 1/2]; NaN where s is not finite (inf - inf, NaN - NaN)
MSD_HD double sc_reduce(double s) { return s - nearbyint(s); }

// the correctly rounded doubles of pi^n / n!: even n = 0, 2, .., 18 and odd n = 1, 3, .., 17.  The first term left out is
// (pi / 4)^20 / 20! = 3.3e-21 for the cosine and (pi / 4)^19 / 19! = 8.3e-20 for the sine at |r| = 1/4: both below 2^-60
#define SC_COS_TERMS 10
#define SC_SIN_TERMS 9
#define SC_COS_COEFFS {0x1.0000000000000p+0, 0x1.3bd3cc9be45dep+2, 0x1.03c1f081b5ac4p+2, 0x1.55d3c7e3cbffap+0, 0x1.e1f506891babbp-3, \
                       0x1.a6d1f2a204a8cp-6, 0x1.f9d38a3763cc3p-10, 0x1.b6e24f44b128fp-14, 0x1.20c62c2f2d7f5p-18, 0x1.2a0c591af8314p-23}
#define SC_SIN_COEFFS {0x1.921fb54442d18p+1, 0x1.4abbce625be53p+2, 0x1.466bc6775aae2p+1, 0x1.32d2cce62bd86p-1, 0x1.50783487ee782p-4, \
                       0x1.e3074fde8871fp-8, 0x1.e8f434d018d63p-12, 0x1.6fadb9f155744p-16, 0x1.aaec32af93359p-21}

// (cos 2 pi f, sin 2 pi f) for |f| <= 1; NaN in both for anything else, a NaN included.  g = 2 f, k = nearbyint(2 g),
// r = g - k / 2 are exact and |r| <= 1/4: the angle is pi r + k pi / 2.  cos(pi r) and sin(pi r) / r are alternating series in
// z = r^2, by Horner from the last coefficient: p = a_last; p = a_n - z p.  k mod 4 swaps and signs.
MSD_HD void sc_sincos2pi(double f, double *c, double *s)
{
    if (!(fabs(f) <= 1.0)) { *c = NAN; *s = NAN; return; }
    const double ac[SC_COS_TERMS] = SC_COS_COEFFS, as[SC_SIN_TERMS] = SC_SIN_COEFFS;
    const double g = 2.0 * f, k = nearbyint(2.0 * g), r = g - k * 0.5, z = r * r;
    double pc = ac[SC_COS_TERMS - 1], ps = as[SC_SIN_TERMS - 1];
    for (int n = SC_COS_TERMS - 2; n >= 0; n--) pc = ac[n] - z * pc;
    for (int n = SC_SIN_TERMS - 2; n >= 0; n--) ps = as[n] - z * ps;
    ps = r * ps;
    switch ((int)k & 3) {                                         // k is a whole number in [-4, 4]
    case 0: *c = pc; *s = ps; break;
    case 1: *c = -ps; *s = pc; break;
    case 2: *c = -pc; *s = -ps; break;
    default: *c = ps; *s = -pc; break;
    }
}

// (ar + i ai) (br + i bi): four products, one subtraction, one addition
MSD_HD void sc_cmul(double ar, double ai, double br, double bi, double *re, double *im)
{
    *re = ar * br - ai * bi;
    *im = ar * bi + ai * br;
}

// P_0 .. P_H of E = (c, s) as (re, im) pairs: P_m = E P_{m-1}, re = c pr - s pi, im = c pi + s pr.  P_0 = 1, or NaN where E is
// NaN: a coordinate that is not finite reaches every q vector, (0, 0, 0) included
MSD_HD void sc_powers(double c, double s, int H, double *tab)
{
    double pr = c == c ? 1.0 : NAN, pi = 0.0;
    tab[0] = pr; tab[1] = pi;
    for (int m = 1; m <= H; m++) {
        double re, im;
        sc_cmul(c, s, pr, pi, &re, &im);
        pr = re; pi = im;
        tab[2 * m] = pr; tab[2 * m + 1] = pi;
    }
}

// the term of (h, k, l) from the three tables of an atom: t0 / t1 / t2 hold P_0 .. of axis 0 / 1 / 2
MSD_HD void sc_term(const double *t0, const double *t1, const double *t2, int h, int k, int l, double *re, double *im)
{
    const int ah = h < 0 ? -h : h, ak = k < 0 ? -k : k, al = l < 0 ? -l : l;
    const double a_re = t0[2 * ah], a_im = h < 0 ? -t0[2 * ah + 1] : t0[2 * ah + 1];
    const double b_re = t1[2 * ak], b_im = k < 0 ? -t1[2 * ak + 1] : t1[2 * ak + 1];
    const double c_re = t2[2 * al], c_im = l < 0 ? -t2[2 * al + 1] : t2[2 * al + 1];
    double m_re, m_im;
    sc_cmul(a_re, a_im, b_re, b_im, &m_re, &m_im);
    sc_cmul(m_re, m_im, c_re, c_im, re, im);
}

// one coordinate of the displacement of the self part
MSD_HD double sc_delta(double f_later, double f_origin) { const double d = f_later - f_origin; return d - nearbyint(d); }

// one product of the coherent part: b conj(a)
MSD_HD void sc_cross(double ar, double ai, double br, double bi, double *re, double *im)
{
    *re = br * ar + bi * ai;
    *im = bi * ar - br * ai;
}

// ---- blocks of origins (series_origins of series_plan.h), the tree ----------------------------------------------------------

// the names the probe of tests/test_scattering_plan.py asks for; the library calls the shared ones
inline int64_t sc_origins(int64_t F, int64_t tau, int64_t stride) { return series_origins(F, tau, stride); }
inline int64_t sc_first_outside(const int64_t *list, int64_t n, int64_t lo, int64_t hi) { return series_first_outside(list, n, lo, hi); }
MSD_HD int64_t sc_blocks(int64_t n_origins) { return (n_origins + SC_BLOCK - 1) / SC_BLOCK; }

// the sum of the SC_BLOCK values of a block in place: steps d = SC_BLOCK / 2, .., 2, 1: v[j] <- v[j] + v[j + d] for j < d; the
// sum is v[0].  The kernel runs the same steps with one thread per j.
inline double sc_tree(double *v)
{
    for (int d = SC_BLOCK / 2; d >= 1; d >>= 1)
        for (int j = 0; j < d; j++) v[j] = v[j] + v[j + d];
    return v[0];
}

// ---- the validation of the q list ---------------------------------------------------------------------------------------

// the largest |index| of every axis into H[3]; false for an index beyond SC_MAX_H
inline bool sc_hmax(const int64_t *q_int, int64_t n_q, int64_t *H)
{
    H[0] = H[1] = H[2] = 0;
    for (int64_t i = 0; i < 3 * n_q; i++) {
        const int64_t v = q_int[i];
        if (v < -SC_MAX_H || v > SC_MAX_H) return false;
        const int64_t a = v < 0 ? -v : v;
        if (a > H[i % 3]) H[i % 3] = a;
    }
    return true;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------
struct ScPlanIn {
    int64_t F, n_a, n_b, n_q, n_lags, stride;
    int64_t H[3];                                 // the largest |index| of every axis (sc_hmax)
    bool same, want_self, want_coherent;
    int64_t workspace_bytes;                      // the caller's cap, 0: the default
};

struct ScPlan {
    int64_t n_sel;                                // selections whose density modes are held: 1 with `same`, else 2
    int64_t n_cols;                               // columns of a frame of fractional coordinates: n_a, or n_a + n_b
    int64_t row;                                  // (re, im) pairs of the three tables of an entry: H0 + H1 + H2 + 3
    int64_t tile;                                 // entries of a tile of tables
    int64_t lds_bytes;
    int64_t n_blocks;                             // blocks of origins at lag 0: the most of any lag
    int64_t q_batch, n_q_batches;                 // q vectors held at once
    int64_t window;                               // frames whose fractional coordinates are held at once (coherent part)
    int64_t lags_per_launch;                      // lags whose block partials are held at once
    int64_t workspace;                            // bytes of the work area
    const char *err;                              // null, or why there is no launch
};

struct ScPieces {
    int64_t *atoms, *lags; int32_t *q;            // [n_a + n_b], [n_lags], [n_q][3]
    double *self_sums, *coherent_sums;            // [n_lags][n_q][2]
    int64_t head;                                 // the work area begins here
    double *frac;                                 // [window][3][n_cols]: f, reduced
    double *rho;                                  // [n_sel][q_batch][F][2]
    double *partial;                              // [lags_per_launch][n_blocks][q_batch][2]
};

inline ScPieces sc_layout(Carve &cv, const ScPlan &p, const ScPlanIn &in)
{
    const int64_t table = in.n_lags * in.n_q * 2;
    ScPieces w;
    w.atoms = cv.take<int64_t>(in.n_a + in.n_b, 256);
    w.lags = cv.take<int64_t>(in.n_lags, 256);
    w.q = cv.take<int32_t>(in.n_q * 3, 256);
    w.self_sums = cv.take<double>(in.want_self ? table : 0, 256);
    w.coherent_sums = cv.take<double>(in.want_coherent ? table : 0, 256);
    cv.take<char>(0, 256);
    w.head = cv.used;
    w.frac = cv.take<double>(in.want_coherent ? p.window * 3 * p.n_cols : 0, 256);
    w.rho = cv.take<double>(in.want_coherent ? p.n_sel * p.q_batch * in.F * 2 : 0, 256);
    w.partial = cv.take<double>(p.lags_per_launch * p.n_blocks * p.q_batch * 2, 256);
    cv.take<char>(0, 256);
    return w;
}

// bytes of LDS of a workgroup: the tables of a tile (k_sc_density, k_sc_self) or the products of a lag tile (k_sc_coherent)
inline int64_t sc_lds_bytes(int64_t row, int64_t tile)
{
    const int64_t tables = tile * row * 16, tree = (int64_t)SC_LAG_TILE * SC_BLOCK * 16;
    return tables > tree ? tables : tree;
}

inline ScPlan sc_plan(const ScPlanIn &in, int64_t default_workspace)
{
    ScPlan p = ScPlan();
    if (in.F < 1 || in.F > SC_MAX_F) { p.err = "1 to 2^29 frames are needed"; return p; }
    if (in.n_lags < 1) { p.err = "an empty lag list"; return p; }
    if (in.stride < 1) { p.err = "origin_stride is below 1"; return p; }
    if (in.n_q < 1 || in.n_q > SC_MAX_Q) { p.err = "1 to 2^16 q vectors are needed"; return p; }
    for (int a = 0; a < 3; a++)
        if (in.H[a] < 0 || in.H[a] > SC_MAX_H) { p.err = "an index of a q vector is beyond 32"; return p; }
    if (in.n_a < 1 || in.n_b < 1 || in.n_a > SC_MAX_ATOMS || in.n_b > SC_MAX_ATOMS) { p.err = "a list holds no atom or more than 2^20"; return p; }
    if (in.same && in.n_a != in.n_b) { p.err = "one selection in two lists of different lengths"; return p; }
    if (!in.want_self && !in.want_coherent) { p.err = "neither part is asked for"; return p; }
    if (in.workspace_bytes < 0) { p.err = "a negative workspace cap"; return p; }
    const int64_t cap = in.workspace_bytes > 0 ? in.workspace_bytes : default_workspace;
    p.n_sel = in.same ? 1 : 2;
    p.n_cols = in.same ? in.n_a : in.n_a + in.n_b;
    p.row = in.H[0] + in.H[1] + in.H[2] + 3;
    p.tile = SC_TILE_LDS / (p.row * 16);
    if (p.tile > SC_TILE_MAX) p.tile = SC_TILE_MAX;
    p.lds_bytes = sc_lds_bytes(p.row, p.tile);
    p.n_blocks = sc_blocks(series_origins(in.F, 0, in.stride));
    // what one q vector, one lag of it and one frame take; the four pieces of the work area start on 256 bytes
    const int64_t q_series = in.want_coherent ? p.n_sel * in.F * 16 : 0, q_lag = p.n_blocks * 16;
    const int64_t frame = in.want_coherent ? 3 * p.n_cols * 8 : 0, slack = 1024;
    if (cap < slack + q_series + q_lag + frame) {
        p.err = in.want_coherent ? "the workspace cap is below one q vector's series and one frame's coordinates"
                                 : "the workspace cap is below one q vector's block sums";
        return p;
    }
    const int64_t avail = cap - slack;
    // the frames first, on at most a quarter of the cap and what one q vector leaves; then the q vectors; then the lags of a launch
    p.window = frame ? in.F : 0;
    if (frame) {
        const int64_t beside_q = (avail - q_series - q_lag) / frame;          // at least 1
        if (p.window > beside_q) p.window = beside_q;
        if (p.window * frame > avail / 4) { p.window = avail / 4 / frame; if (p.window < 1) p.window = 1; }
        if (p.window > SC_MAX_FRAC / p.n_cols) p.window = SC_MAX_FRAC / p.n_cols;
    }
    int64_t left = avail - p.window * frame;
    p.q_batch = left / (q_series + q_lag);
    if (p.q_batch > in.n_q) p.q_batch = in.n_q;
    if (p.q_batch > SC_MAX_QBATCH) p.q_batch = SC_MAX_QBATCH;
    p.n_q_batches = (in.n_q + p.q_batch - 1) / p.q_batch;
    left -= p.q_batch * q_series;
    p.lags_per_launch = left / (p.q_batch * q_lag);
    if (p.lags_per_launch > in.n_lags) p.lags_per_launch = in.n_lags;
    if (p.lags_per_launch > SC_MAX_LAGS_LAUNCH) p.lags_per_launch = SC_MAX_LAGS_LAUNCH;
    Carve cv = {nullptr, 0};
    const ScPieces w = sc_layout(cv, p, in);
    p.workspace = cv.used - w.head;
    return p;
}
