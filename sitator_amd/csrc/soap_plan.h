// Every decision and every per-point formula of the SOAP site descriptors (site_descriptors/SOAP.py, whose engines - QUIP, DScribe -
// are external programs), written once for the kernels of soap.hip and for the host compiler (tests/test_soap_ref.py drives it
// with g++ under ASan / UBSan).  The descriptor is the GTO construction of Himanen et al., Comput. Phys. Commun. 247 (2020)
// 106949, fixed in DESIGN.md section 17; agreement with an installation of DScribe or QUIP is not claimed.
//
// What is computed for a centre x, per environment species Z, with a = 1 / (2 sigma^2):
//     c_Z,nlm = sum over images i of species Z with |p_i| <= cutoff, p_i = r_i - x, of
//               w(|p_i|) sum_n' beta[l][n][n'] K[l][n'] exp(-gam[l][n'] |p_i|^2) R_lm(p_i),
//     K = pi^(3/2) a^l (alpha + a)^-(l + 3/2),  gam = alpha a / (alpha + a)                      (sp_prim_consts, sp_primitive),
//     R_lm = |p|^l Y_lm(p / |p|) the real orthonormal solid harmonic, a polynomial in p          (sp_solid_harmonics),
//     p[Z1, Z2, n, n', l] = pi sqrt(8 / (2 l + 1)) sum_m c_Z1,nlm c_Z2,n'lm, m ascending         (sp_contract).
// Nothing divides by |p|: a centre on an atom is an ordinary input.  alpha[l][n] and beta[l][n][n'] come from the caller.
//
// Which images: the translation ranges of barrier_plan.h (bp_plan, bp_axis_range), complete for any cell shape.
//
// The order of every sum (soap.hip): the neighbour list of a centre is in (atom, m0, m1, m2) order, ascending; every coefficient
// adds its neighbours in list order; the contraction runs over m ascending.  Nothing depends on arrival.
//
// Capacities: l_max <= SP_MAX_L, n_max <= SP_MAX_N, species <= SP_MAX_SPECIES; a workgroup of SP_BLOCK threads stages SP_NBR_CAP
// neighbours at a time (longer lists go round again) - sp_lds_doubles has the bytes.
//
// The bucket plan of SOAPDescriptorAverages (SOAP.py:258-320) in integers: sp_bucket_*.
#pragma once

#include <stdint.h>

#include "barrier_plan.h"

#define SP_HD CP_HD

#define SP_BLOCK 256                                   // threads of a workgroup: one workgroup per environment
#define SP_WAVE 64
#define SP_NBR_CAP 32                                  // neighbours staged at once
#define SP_MAX_L 8
#define SP_MAX_N 8
#define SP_MAX_SPECIES 4
#define SP_MAX_L2 ((SP_MAX_L + 1) * (SP_MAX_L + 1))
#define SP_MAX_OWN ((SP_MAX_SPECIES * SP_MAX_N * SP_MAX_L2 + SP_BLOCK - 1) / SP_BLOCK)   // coefficients a lane accumulates
#define SP_NBR_REC 4                                   // doubles of a staged neighbour: p[3], w

#define SP_PI 3.14159265358979323846

struct SoapShape {
    int n_species, n_max, l_max;
    int L2;                                            // (l_max + 1)^2 harmonics
    int NR;                                            // n_max (l_max + 1) radial values of a neighbour
    int n_coef;                                        // n_species n_max L2
};

// false: beyond a capacity (what: 1 l_max, 2 n_max, 3 species)
SP_HD inline bool sp_shape(int n_species, int n_max, int l_max, SoapShape &s, int *what)
{
    *what = 0;
    if (l_max < 0 || l_max > SP_MAX_L) { *what = 1; return false; }
    if (n_max < 1 || n_max > SP_MAX_N) { *what = 2; return false; }
    if (n_species < 1 || n_species > SP_MAX_SPECIES) { *what = 3; return false; }
    s.n_species = n_species; s.n_max = n_max; s.l_max = l_max;
    s.L2 = (l_max + 1) * (l_max + 1);
    s.NR = n_max * (l_max + 1);
    s.n_coef = n_species * n_max * s.L2;
    return true;
}

// LDS of a workgroup in doubles: neighbours | harmonics | radial values | coefficients | K, gam | beta | species of the
// neighbours and the scan words (as int32, 2 per double)
SP_HD inline int sp_lds_doubles(const SoapShape &s)
{
    const int tab = (s.l_max + 1) * s.n_max;
    return SP_NBR_CAP * (SP_NBR_REC + s.L2 + s.NR) + s.n_coef + 2 * tab + tab * s.n_max + (SP_NBR_CAP + 16) / 2;
}

// features of the power spectrum: species pairs outermost in the order of the environment list (crossover: all Z1 <= Z2, else
// Z1 = Z2), then n, then n' (n' >= n when Z1 = Z2, all n' when Z1 < Z2), then l
SP_HD inline int64_t sp_n_dim(int n_species, int n_max, int l_max, int crossover)
{
    const int64_t same = (int64_t)n_max * (n_max + 1) / 2 * (l_max + 1), cross = (int64_t)n_max * n_max * (l_max + 1);
    return n_species * same + (crossover ? (int64_t)n_species * (n_species - 1) / 2 * cross : 0);
}

// the feature table: feat[3 f] = the row of c of (Z1, n), feat[3 f + 1] = of (Z2, n') (a row: Z n_max + n), feat[3 f + 2] = l
inline int64_t sp_feature_table(int n_species, int n_max, int l_max, int crossover, int32_t *feat)
{
    int64_t f = 0;
    for (int z1 = 0; z1 < n_species; z1++)
        for (int z2 = z1; z2 < (crossover ? n_species : z1 + 1); z2++)
            for (int n = 0; n < n_max; n++)
                for (int m = (z1 == z2 ? n : 0); m < n_max; m++)
                    for (int l = 0; l <= l_max; l++, f++)
                        if (feat) { feat[3 * f] = z1 * n_max + n; feat[3 * f + 1] = z2 * n_max + m; feat[3 * f + 2] = l; }
    return f;
}

// K and gam of a primitive r^l exp(-alpha r^2) against a Gaussian of exponent a
inline void sp_prim_consts(double a, double alpha, int l, double *K, double *gam)
{
    const double s = alpha + a;
    *K = pow(SP_PI, 1.5) * pow(a, (double)l) * pow(s, -((double)l + 1.5));
    *gam = alpha * a / s;
}

SP_HD inline double sp_primitive(double K, double gam, double d2) { return K * exp(-gam * d2); }

// the switch: 1 up to cutoff - t, 0.5 (1 + cos(pi (d - cutoff + t) / t)) beyond; t <= 0: the hard cut
SP_HD inline double sp_switch(double d, double cutoff, double t)
{
    if (!(t > 0.0) || d <= cutoff - t) return 1.0;
    return 0.5 * (1.0 + cos(SP_PI * (d - cutoff + t) / t));
}

// norm[l l + l + m] = sqrt((2 l + 1) / (4 pi) (l - |m|)! / (l + |m|)!), times sqrt(2) for m != 0
inline void sp_harmonic_norms(int l_max, double *norm)
{
    for (int l = 0; l <= l_max; l++)
        for (int m = 0; m <= l; m++) {
            double ratio = 1.0;
            for (int k = l - m + 1; k <= l + m; k++) ratio /= (double)k;
            const double v = sqrt((2.0 * l + 1.0) / (4.0 * SP_PI) * ratio) * (m ? sqrt(2.0) : 1.0);
            norm[l * l + l + m] = v;
            norm[l * l + l - m] = v;
        }
}

// out[l l + l + m] = |p|^l Y_lm(p / |p|), real orthonormal, no Condon-Shortley phase, m > 0: cos, m < 0: sin.  With
// (x + i y)^m = C_m + i S_m and Q_l^m the polynomial |p|^(l - m) d^m P_l / d u^m at u = z / |p|:
//     Q_m^m = (2 m - 1)!!,  Q_(m+1)^m = (2 m + 1) z Q_m^m,  (l - m) Q_l^m = (2 l - 1) z Q_(l-1)^m - (l + m - 1) |p|^2 Q_(l-2)^m.
SP_HD inline void sp_solid_harmonics(double x, double y, double z, int l_max, const double *norm, double *out)
{
    const double r2 = (x * x + y * y) + z * z;
    double cm = 1.0, sm = 0.0, qmm = 1.0;
    for (int m = 0; m <= l_max; m++) {
        if (m) {
            const double c2 = x * cm - y * sm, s2 = x * sm + y * cm;
            cm = c2; sm = s2;
            qmm *= (double)(2 * m - 1);
        }
        double q2 = 0.0, q1 = qmm;                     // Q_(l-2)^m, Q_(l-1)^m
        for (int l = m; l <= l_max; l++) {
            double q;
            if (l == m) q = qmm;
            else {
                q = ((double)(2 * l - 1) * z * q1 - (double)(l + m - 1) * r2 * q2) / (double)(l - m);
                q2 = q1; q1 = q;
            }
            const int at = l * l + l;
            out[at + m] = norm[at + m] * q * cm;
            if (m) out[at - m] = norm[at - m] * q * sm;
        }
    }
}

// one feature from the rows ca, cb of the coefficients (each L2 long): the sum over m ascending
SP_HD inline double sp_contract(const double *ca, const double *cb, int l)
{
    double s = 0.0;
    for (int k = l * l; k <= l * l + 2 * l; k++) s += ca[k] * cb[k];
    return SP_PI * sqrt(8.0 / (2.0 * l + 1.0)) * s;
}

// ---- the bucket plan of SOAPDescriptorAverages --------------------------------------------------------------------------------
// labels[F, M] (-1: unassigned; every label in [-1, K)), the strided frames f with f % stepsize == 0.

// SOAP.py:263-266: counts[s] = strided frames in which site s holds at least one ion.  stamp[K]: scratch.
inline void sp_bucket_counts(const int64_t *labels, int64_t F, int64_t M, int64_t K, int64_t stepsize, int64_t *counts, int64_t *stamp)
{
    for (int64_t s = 0; s < K; s++) { counts[s] = 0; stamp[s] = -1; }
    for (int64_t f = 0; f < F; f += stepsize)
        for (int64_t m = 0; m < M; m++) {
            const int64_t s = labels[f * M + m];
            if (s >= 0 && stamp[s] != f) { stamp[s] = f; counts[s]++; }
        }
}

// :268-276: the averaging asked for, or floor(mean(counts) / avg_descriptors_per_site); 0 becomes 1 (*was_zero)
inline int64_t sp_bucket_averaging(const int64_t *counts, int64_t K, int64_t averaging, int64_t avg_descriptors_per_site, int *was_zero)
{
    *was_zero = 0;
    if (averaging <= 0) {
        int64_t sum = 0;
        for (int64_t s = 0; s < K; s++) sum += counts[s];
        averaging = (int64_t)floor(((double)sum / (double)K) / (double)avg_descriptors_per_site);
    }
    if (averaging == 0) { *was_zero = 1; averaging = 1; }
    return averaging;
}

// :278-292: rows per site, vectors per row, first row.  Returns the number of rows.
inline int64_t sp_bucket_rows(const int64_t *counts, int64_t K, int64_t averaging, int64_t *nr_of_descs, int64_t *averagings, int64_t *first_row)
{
    int64_t rows = 0;
    for (int64_t s = 0; s < K; s++) {
        const int64_t nr = counts[s] / averaging;
        averagings[s] = nr == 0 ? counts[s] : averaging;
        nr_of_descs[s] = nr > 1 ? nr : 1;
        first_row[s] = rows;
        rows += nr_of_descs[s];
    }
    return rows;
}

// :297-315: the contributors in frame order, inside a frame in ion order.  Of several ions on one site in one frame the last in
// ion order contributes (numpy's fancy +=); the k-th frame of a site goes to row first_row + k / averagings while that is one of
// the site's rows.  entry[i] = frame * M + ion, row[i], site[i]; any of them may be NULL (a counting call).  seen[K], stamp[K],
// last[K]: scratch.
inline int64_t sp_bucket_contributors(const int64_t *labels, int64_t F, int64_t M, int64_t K, int64_t stepsize, const int64_t *nr_of_descs,
                                      const int64_t *averagings, const int64_t *first_row, int64_t *seen, int64_t *stamp, int64_t *last,
                                      int64_t *entry, int64_t *row, int64_t *site)
{
    int64_t n = 0;
    for (int64_t s = 0; s < K; s++) { seen[s] = 0; stamp[s] = -1; last[s] = -1; }
    for (int64_t f = 0; f < F; f += stepsize) {
        for (int64_t m = 0; m < M; m++) {
            const int64_t s = labels[f * M + m];
            if (s >= 0) { stamp[s] = f; last[s] = m; }
        }
        for (int64_t m = 0; m < M; m++) {
            const int64_t s = labels[f * M + m];
            if (s < 0 || stamp[s] != f || last[s] != m) continue;
            const int64_t k = seen[s]++;
            if (k / averagings[s] >= nr_of_descs[s]) continue;
            if (entry) entry[n] = f * M + m;
            if (row) row[n] = first_row[s] + k / averagings[s];
            if (site) site[n] = s;
            n++;
        }
    }
    return n;
}
