// The decisions of the landmark pruning tables (candidates.hip) in a form the host compiler takes too
// (tests/test_candidates_plan.py runs them with g++ under ASan / UBSan against tests/candidates_ref.py): the periodic
// distance tests, the bound of a (landmark, vertex), the box of bins a landmark's workgroup walks, the test of one
// (bin, landmark) pair, its critical vertex, the grid and the covering radius of a bin, the per-bin sort - and
// cand_build_host, which builds a whole table serially from the same functions.  The kernels of candidates.hip call
// these functions; both sides must be compiled without contraction (-ffp-contract=off): the device table and the
// host table are compared integer for integer.
//
// cm = cell.T (columns are the cell vectors), ci = inverse(cm), both row-major, as in Pbc (sit_internal.h).
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define CAND_HD __host__ __device__
#define CAND_HD_INLINE __host__ __device__ __forceinline__
#else
#define CAND_HD
#define CAND_HD_INLINE inline
#endif

#define CAND_MAX_GRID 192                    // bins per axis
#define CAND_MAX_BINS 1500000                // bins in all: the largest axis is thinned by 3/4 while there are more
#define CAND_PACK_BITS 24                    // scatter pass: landmark | critical vertex << 24 while D < 2^24

struct CandArgs {
    double cm[9], ci[9], h[3];
    const double *ref_static;
    const int32_t *verts;      // [D, Vp], -1 padded
    const double *vcd;         // [D, Vp]
    int64_t D, Vp, nb;
    int G[3];
    double rz, displacement, rb;
    int32_t *cnt;              // [nb + 1] counts, then offsets
    int32_t *cursor;           // [nb]
    int32_t *list;             // scatter pass: landmark | critical vertex << 24 (split off after the sort)
};

CAND_HD_INLINE void cand_matvec(const double *m, const double *v, double *o)
{
    o[0] = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
    o[1] = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
    o[2] = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
}

// images searched per axis for a distance of at most T: the fractional difference is reduced to [-0.5, 0.5], a lattice
// plane of axis i is h[i] away from the next
CAND_HD_INLINE int cand_images(const CandArgs &a, int i, double T) { return (int)floor(T / a.h[i] + 0.5); }

// exact periodic distance test: is min_L |d + L| <= T ?
CAND_HD inline bool cand_within_periodic(const CandArgs &a, const double *d, double T)
{
    double f[3];
    cand_matvec(a.ci, d, f);
    int n[3];
    for (int i = 0; i < 3; i++) { f[i] -= floor(f[i] + 0.5); n[i] = cand_images(a, i, T); }
    const double T2 = T * T;
    for (int ia = -n[0]; ia <= n[0]; ia++)
        for (int ib = -n[1]; ib <= n[1]; ib++)
            for (int ig = -n[2]; ig <= n[2]; ig++) {
                const double ff[3] = {f[0] + ia, f[1] + ib, f[2] + ig};
                double r[3];
                cand_matvec(a.cm, ff, r);
                if (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] <= T2) return true;
            }
    return false;
}

// squared periodic distance min_L |d + L|^2, searched over the images that can be closer than T
CAND_HD inline double cand_periodic_dist2(const CandArgs &a, const double *d, double T)
{
    double f[3];
    cand_matvec(a.ci, d, f);
    int n[3];
    for (int i = 0; i < 3; i++) { f[i] -= floor(f[i] + 0.5); n[i] = cand_images(a, i, T); }
    double best = 1e300;
    for (int ia = -n[0]; ia <= n[0]; ia++)
        for (int ib = -n[1]; ib <= n[1]; ib++)
            for (int ig = -n[2]; ig <= n[2]; ig++) {
                const double ff[3] = {f[0] + ia, f[1] + ib, f[2] + ig};
                double r[3];
                cand_matvec(a.cm, ff, r);
                const double r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
                best = r2 < best ? r2 : best;
            }
    return best;
}

// how far the centre of a listed bin may be from vertex h of landmark k (the right-hand side of candidates.hip's bound)
CAND_HD_INLINE double cand_bound_of(const CandArgs &a, int64_t k, int64_t h)
{
    return a.rz * a.vcd[k * a.Vp + h] * (1.0 + 1e-9) + a.displacement * (1.0 + 1e-9) + a.rb + 1e-9;
}

// The bins one landmark's workgroup walks: its real vertices (the row ends at the first -1), the tightest of them,
// and per axis the bins [lo, lo + cnt) (mod G) whose centre can be within that vertex's bound of it.
struct CandBox {
    int64_t nv;
    int best;                  // the tightest vertex, -1: the landmark has none (every bin is walked)
    double tbest;
    int lo[3], cnt[3];
};

CAND_HD inline CandBox cand_box(const CandArgs &a, int64_t k)
{
    CandBox b;
    b.nv = 0; b.best = -1; b.tbest = 0.0;
    for (int64_t h = 0; h < a.Vp; h++) {
        if (a.verts[k * a.Vp + h] < 0) break;
        const double t = cand_bound_of(a, k, h);
        if (b.best < 0 || t < b.tbest) { b.best = (int)h; b.tbest = t; }
        b.nv++;
    }
    for (int i = 0; i < 3; i++) { b.lo[i] = 0; b.cnt[i] = a.G[i]; }
    if (b.nv > 0) {
        // bins whose centre can be within tbest of the tightest vertex
        const double *rv = a.ref_static + 3 * a.verts[k * a.Vp + b.best];
        double f0[3];
        cand_matvec(a.ci, rv, f0);
        for (int i = 0; i < 3; i++) {
            const double w = b.tbest / a.h[i];
            const double x0 = (f0[i] - w) * a.G[i] - 0.5, x1 = (f0[i] + w) * a.G[i] - 0.5;
            const int64_t ia = (int64_t)ceil(x0 - 1e-9), ib = (int64_t)floor(x1 + 1e-9);
            const int64_t n = ib - ia + 1;
            if (n >= a.G[i]) { b.lo[i] = 0; b.cnt[i] = a.G[i]; }
            else if (n <= 0) { b.lo[i] = 0; b.cnt[i] = 0; }
            else { b.lo[i] = (int)(((ia % a.G[i]) + a.G[i]) % a.G[i]); b.cnt[i] = (int)n; }
        }
    }
    return b;
}

CAND_HD_INLINE int64_t cand_box_bins(const CandBox &b) { return (int64_t)b.cnt[0] * b.cnt[1] * b.cnt[2]; }

// bin q of the box (z fastest): its coordinates on the grid, its centre cb, its index
CAND_HD_INLINE int64_t cand_box_bin(const CandArgs &a, const CandBox &b, int64_t q, double cb[3])
{
    const int iz = (int)(q % b.cnt[2]);
    const int64_t q2 = q / b.cnt[2];
    const int iy = (int)(q2 % b.cnt[1]), ix = (int)(q2 / b.cnt[1]);
    const int bx = (b.lo[0] + ix) % a.G[0], by = (b.lo[1] + iy) % a.G[1], bz = (b.lo[2] + iz) % a.G[2];
    const double fc[3] = {(bx + 0.5) / a.G[0], (by + 0.5) / a.G[1], (bz + 0.5) / a.G[2]};
    cand_matvec(a.cm, fc, cb);
    return ((int64_t)bx * a.G[1] + by) * a.G[2] + bz;
}

// is landmark k (nv real vertices) listed for the bin with centre cb: every vertex within its bound of the centre
CAND_HD inline bool cand_pair_listed(const CandArgs &a, int64_t k, int64_t nv, const double cb[3])
{
    bool ok = true;
    for (int64_t h = 0; h < nv && ok; h++) {
        const double *p = a.ref_static + 3 * a.verts[k * a.Vp + h];
        const double d[3] = {p[0] - cb[0], p[1] - cb[1], p[2] - cb[2]};
        ok = cand_within_periodic(a, d, cand_bound_of(a, k, h));
    }
    return ok;
}

// the CRITICAL vertex of (bin, landmark): the one with the least room between the bin centre's distance and its bound -
// the vertex most likely to put an ion of this bin beyond the cut-off (fill3.hip tests it first).  Any choice is
// correct; this one is the cheapest on average.  It travels in the top byte of the list entry, so there is none (0)
// once landmark ids need those bits.
CAND_HD inline int cand_critical_vertex(const CandArgs &a, int64_t k, int64_t nv, const double cb[3])
{
    int crit = 0;
    double room = 1e300;
    if (a.D < (1LL << CAND_PACK_BITS))
        for (int64_t h = 0; h < nv; h++) {
            const double *p = a.ref_static + 3 * a.verts[k * a.Vp + h];
            const double d[3] = {p[0] - cb[0], p[1] - cb[1], p[2] - cb[2]};
            const double bd = cand_bound_of(a, k, h);
            const double m = bd - sqrt(cand_periodic_dist2(a, d, bd));
            if (m < room) { room = m; crit = (int)h; }
        }
    return crit;
}

CAND_HD_INLINE int32_t cand_pack(int64_t k, int crit) { return (int32_t)k | (crit << CAND_PACK_BITS); }

// one bin's list after the scatter pass: ascending landmark (the scatter order is arbitrary), then the critical vertex
// moves to its own array
CAND_HD inline void cand_sort_bin(int32_t *l, unsigned char *cr, int n, int packed)
{
    const int32_t km = packed ? 0xffffff : 0x7fffffff;
    for (int i = 1; i < n; i++) {
        const int32_t v = l[i];
        int j = i - 1;
        while (j >= 0 && (l[j] & km) > (v & km)) { l[j + 1] = l[j]; j--; }
        l[j + 1] = v;
    }
    for (int i = 0; i < n; i++) {
        cr[i] = packed ? (unsigned char)((unsigned)l[i] >> CAND_PACK_BITS) : (unsigned char)0;
        l[i] &= km;
    }
}

// ---- the grid (host side of sit_build_candidates) ----------------------------------------------------------------

// perpendicular heights h[] of the cell, bins per axis G[] of about bin_target Angstrom (at most CAND_MAX_GRID per
// axis and CAND_MAX_BINS in all) and the covering radius of a bin: half its longest body diagonal, plus 1e-6 that also
// absorbs the rounding of the device-side bin index
inline void cand_grid(const double cm[9], const double ci[9], double bin_target, double h[3], int G[3], double *rb_out)
{
    double len[3];
    for (int i = 0; i < 3; i++) {
        const double *r = ci + 3 * i;
        h[i] = 1.0 / sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        len[i] = sqrt(cm[i] * cm[i] + cm[3 + i] * cm[3 + i] + cm[6 + i] * cm[6 + i]);
    }
    for (int i = 0; i < 3; i++) {
        G[i] = (int)lround(len[i] / bin_target);
        G[i] = G[i] < CAND_MAX_GRID ? G[i] : CAND_MAX_GRID;
        G[i] = G[i] > 1 ? G[i] : 1;
    }
    while ((int64_t)G[0] * G[1] * G[2] > CAND_MAX_BINS) {
        const int m = (G[0] >= G[1] && G[0] >= G[2]) ? 0 : (G[1] >= G[2] ? 1 : 2);
        G[m] = G[m] * 3 / 4;
    }
    double rb = 0;
    for (int sa = -1; sa <= 1; sa += 2)
        for (int sb = -1; sb <= 1; sb += 2) {
            const double f[3] = {1.0 / G[0], sa * 1.0 / G[1], sb * 1.0 / G[2]};
            double r[3];
            for (int i = 0; i < 3; i++) r[i] = cm[3 * i] * f[0] + cm[3 * i + 1] * f[1] + cm[3 * i + 2] * f[2];
            const double half = 0.5 * sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            rb = rb > half ? rb : half;
        }
    *rb_out = rb + 1e-6;
}

// cm, ci, h, G, nb, rb, displacement of `a` for a table with bins of about bin_target (the basis fields stay)
inline void cand_setup(CandArgs &a, const double cm[9], const double ci[9], double displacement, double bin_target)
{
    for (int i = 0; i < 9; i++) { a.cm[i] = cm[i]; a.ci[i] = ci[i]; }
    cand_grid(a.cm, a.ci, bin_target, a.h, a.G, &a.rb);
    a.nb = (int64_t)a.G[0] * a.G[1] * a.G[2];
    a.displacement = displacement;
}

// ---- a whole table, serially: what k_cand_pass<false>, k_cand_scan, k_cand_pass<true> and k_cand_sort leave behind ----

struct CandTable {
    std::vector<int32_t> off;            // [nb + 1]
    std::vector<int32_t> list;           // [total] ascending landmarks of every bin
    std::vector<unsigned char> crit;     // [total]
    int64_t W, total;                    // widest bin (1 for an empty table), entries
};

// `a` as cand_setup left it, with the basis (ref_static, verts, vcd, D, Vp, rz) filled in; cnt / cursor / list are set here
inline void cand_build_host(CandArgs a, CandTable &t)
{
    t.off.assign((size_t)(a.nb + 1), 0);
    std::vector<int32_t> cursor((size_t)a.nb, 0);
    a.cnt = t.off.data(); a.cursor = cursor.data(); a.list = nullptr;
    // count
    for (int64_t k = 0; k < a.D; k++) {
        const CandBox box = cand_box(a, k);
        const int64_t n = cand_box_bins(box);
        for (int64_t q = 0; q < n; q++) {
            double cb[3];
            const int64_t b = cand_box_bin(a, box, q, cb);
            if (cand_pair_listed(a, k, box.nv, cb)) a.cnt[b + 1]++;
        }
    }
    // exclusive scan of cnt[1..nb] in place, and the widest bin
    int64_t acc = 0;
    int w = 0;
    for (int64_t b = 1; b <= a.nb; b++) { w = a.cnt[b] > w ? a.cnt[b] : w; acc += a.cnt[b]; a.cnt[b] = (int32_t)acc; }
    t.total = acc;
    t.W = w > 0 ? w : 1;
    t.list.assign((size_t)acc, 0);
    t.crit.assign((size_t)acc, 0);
    a.list = t.list.data();
    // scatter, landmarks in DESCENDING order (the device's order is arbitrary): the sort below has work to do
    for (int64_t k = a.D - 1; k >= 0; k--) {
        const CandBox box = cand_box(a, k);
        const int64_t n = cand_box_bins(box);
        for (int64_t q = 0; q < n; q++) {
            double cb[3];
            const int64_t b = cand_box_bin(a, box, q, cb);
            if (!cand_pair_listed(a, k, box.nv, cb)) continue;
            a.list[a.cnt[b] + a.cursor[b]++] = cand_pack(k, cand_critical_vertex(a, k, box.nv, cb));
        }
    }
    const int packed = a.D < (1LL << CAND_PACK_BITS) ? 1 : 0;
    for (int64_t b = 0; b < a.nb; b++)
        cand_sort_bin(t.list.data() + a.cnt[b], t.crit.data() + a.cnt[b], a.cnt[b + 1] - a.cnt[b], packed);
}
