// Every decision of EnergyLandscape: the energy of ONE probe ion at the centre of every voxel of a periodic
// grid, in the frozen lattice of S static atoms under the truncated and shifted 12-6 potential of barrier_plan.h - written once for
// the kernels of landscape.hip and for the host compiler (tests/test_landscape_plan.py drives it with g++ under ASan / UBSan).
// Compile without contraction (-ffp-contract=off): everything is compared bit for bit with tests/landscape_ref.py.
//
// Voxel centre.  Voxel (i0, i1, i2) of the grid (n0, n1, n2), flat index v = (i0 n1 + i1) n2 + i2:
//     f_a = ((double)i_a + 0.5) / (double)n_a,    x_k = (f0 cell[0][k] + f1 cell[1][k]) + f2 cell[2][k].
// The crystal coordinates of x are f itself: no inverse is needed on the voxel's side.
//
// Term.  That of barrier_plan.h for a static atom s and an integer triple m: b = x - s, T(m) as there, d = b - T,
// dd = (d0 d0 + d1 d1) + d2 d2, counted where dd <= rc2, value bp_phi(dd, sig2, eps4, e0).  dd = 0 gives +inf, never NaN.  A term is
// the same bits whoever evaluates it.  The pair term enters the loops as a type (LpLJ) so that another potential can follow.
//
// Sum.  E(v) is the flat sequential float64 sum, from 0.0, of the counted terms in ascending (s, m0, m1, m2): no sub-sum per atom, no
// tree, no atomics.  A term that fails the cutoff test adds nothing, so two complete enumerations in that order - whatever else they
// walk over - give the same bytes.  Both kernel forms and the Python loop of the restatement are such enumerations.
//
// Form 1, direct.  A thread per voxel walks, for every atom in turn, the triples of bp_axis_range at its own crystal coordinate
// (lp_atom_add): complete by the argument of barrier_plan.h.
//
// Form 2, tiled.  A workgroup of LP_BLOCK threads owns a tile of LP_TILE0 x LP_TILE1 x LP_TILE2 voxels (partial at the upper edges
// of the grid), thread x the voxel (x / 64, x / 8 % 8, x % 8) of it: neighbouring lanes are neighbours along the last axis.  The
// workgroup first lists every (s, m) that can lie within rc of ANY voxel centre of the tile, then every thread runs the list for
// its own voxel: two subtractions per coordinate, the squared distance, the cutoff test, the pair term - no floor, no range.
//
// Why the list misses nothing.  Let the tile hold the voxels o_a <= i_a < o_a + c_a.  Its voxel centres have crystal coordinates
// between (o_a + 0.5) / n_a and (o_a + c_a - 0.5) / n_a: within e_a = (c_a - 1) / (2 n_a) of fc_a = (o_a + c_a / 2) / n_a.  By
// barrier_plan.h a term within rc of the voxel at f has |g_a - m_a| <= q_a = rc / h_a on every axis, g = f - ci(s), whatever the
// cell's shape, since |d| >= |g_a - m_a| h_a.  With gc = fc - ci(s), |gc_a - g_a| <= e_a, hence |gc_a - m_a| <= q_a + e_a: the
// integers bp_axis_range finds at gc_a for the widened q_a + e_a, with its own slack (1e-9 cell units and more, against roundings
// of 1e-16 in f, fc and e and of 1e-10 in ci(s)), clamped to |t| <= floor(q_a + e_a) + 1, which covers -(q_a + e_a) <= t <=
// 1 + q_a + e_a.  What the list holds beyond that is harmless: the cutoff test of each term decides.
//
// Chunks.  The list is generated in ascending (s, m0, m1, m2) - atoms in batches of LP_BLOCK, thread t the atom t of the batch, an
// exclusive prefix sum of the threads' counts gives every entry its place - and consumed in chunks of LP_CHUNK records of LDS:
// the chunk is run by every thread as soon as it is full, and once more at the end.  Consecutive chunks of an ordered list leave
// the order of the sum untouched.  lp_tile_serial is the same schedule on the host.
//
// LDS.  Tiled: LP_CHUNK records of LP_REC doubles (32 256 bytes) and the four wave sums of the prefix: LP_LDS_TILED = 32 288 bytes
// of the 160 KiB of a gfx950 CU - four workgroups (16 waves) of a CU fit, as many as the direct form's BP_TILE records of
// barrier_plan.h (36 864 bytes) admit.  Every lane of a wave reads the same record (a broadcast: no bank conflict whatever the
// stride); the records are written LP_REC doubles apart, 72 bytes, which keeps the 32 lanes of a half wave on distinct bank pairs.
//
// Limits.  n_a in [1, 1024] and V <= 2^27, those of sit_percolation_*: a result can always be handed on.
#pragma once

#include <stdint.h>

#include "barrier_plan.h"

#define LP_HD BP_HD

#define LP_BLOCK 256                                   // threads of a workgroup: one per voxel of a tile
#define LP_TILE0 4
#define LP_TILE1 8
#define LP_TILE2 8
#define LP_REC 9                                       // doubles of a list record: s[3], T(m)[3], eps4, sig2, e0
#define LP_CHUNK 448                                   // records of LDS a chunk of the list holds
#define LP_LDS_TILED (LP_CHUNK * LP_REC * 8 + 32)
#define LP_LDS_DIRECT (BP_TILE * BP_REC * 8)
#define LP_MAX_GRID 1024
#define LP_MAX_VOXELS ((int64_t)1 << 27)
#define LP_FORM_DIRECT 1
#define LP_FORM_TILED 2
#define LP_PLAN_WORDS 16

static_assert(LP_TILE0 * LP_TILE1 * LP_TILE2 == LP_BLOCK, "a thread per voxel of a tile");

// The form 0 resolves to: the tiled form where rc is shorter than every perpendicular height of the cell (q_a < 1 on every axis),
// else the direct form.  Measured: on the 512-atom C2 host, q_a <= 0.38, the tiled kernel takes 0.52 ms
// against 3.46 ms (rc = 6 A) and 1.02 ms against 6.55 ms (rc = 12 A) - there the direct form spends its time finding out, atom by
// atom, that nothing is in reach; on the 4 A cell with 5 atoms and q_a about 2.2, where every atom has images in reach of every voxel
// and a list can drop none, the direct kernel takes 0.25 ms against 0.34 ms.  Between the two regimes nothing was measured.
LP_HD inline int lp_form(int form, const BarrierPlan &bp)
{
    if (form) return form;
    return bp.q[0] < 1.0 && bp.q[1] < 1.0 && bp.q[2] < 1.0 ? LP_FORM_TILED : LP_FORM_DIRECT;
}

// the 12-6 pair term on the parameters of a record, par = (eps4, sig2, e0)
struct LpLJ {
    static LP_HD inline double phi(double dd, const double *par) { return bp_phi(dd, par[1], par[0], par[2]); }
};

struct LandscapePlan {
    const char *err;                                   // null, or what is wrong with the arguments
    BarrierPlan bp;
    int64_t n[3], V, tiles[3], n_tiles;
    int form;                                          // the form taken
    int wide[3];                                       // |t_a| of the list of a full tile
};

LP_HD inline int lp_tile_edge(int a) { return a == 0 ? LP_TILE0 : a == 1 ? LP_TILE1 : LP_TILE2; }

// |t_a| the widened range of a tile of half-extent `half` is clamped to
LP_HD inline int lp_wide(double q, double half)
{
    const double qw = q + half;
    return (int)floor(qw * (1.0 + BP_SLACK) + BP_SLACK) + 1;
}

template <class P> LP_HD inline LandscapePlan lp_plan(const P &c, double rc, const int64_t *grid3, int form)
{
    LandscapePlan p;
    p.err = nullptr;
    p.V = 1; p.n_tiles = 1; p.form = 0;
    for (int a = 0; a < 3; a++) { p.n[a] = grid3[a]; p.tiles[a] = 0; p.wide[a] = 0; }
    for (int a = 0; a < 3; a++)
        if (grid3[a] < 1 || grid3[a] > LP_MAX_GRID) { p.err = "an axis of the grid holds 1 to 1024 voxels"; p.V = 0; p.n_tiles = 0; return p; }
    for (int a = 0; a < 3; a++) {
        p.V *= p.n[a];
        p.tiles[a] = (p.n[a] + lp_tile_edge(a) - 1) / lp_tile_edge(a);
        p.n_tiles *= p.tiles[a];
    }
    if (p.V > LP_MAX_VOXELS) { p.err = "more than 2^27 voxels"; return p; }
    if (form < 0 || form > 2) { p.err = "form is 0, 1 or 2"; return p; }
    if (!bp_plan(c, rc, p.bp)) { p.err = "degenerate cell, or rc not positive or beyond 255 perpendicular heights of the cell"; return p; }
    p.form = lp_form(form, p.bp);
    for (int a = 0; a < 3; a++) {
        const int64_t cnt = p.n[a] < lp_tile_edge(a) ? p.n[a] : lp_tile_edge(a);
        p.wide[a] = lp_wide(p.bp.q[a], (0.5 * (double)(cnt - 1)) / (double)p.n[a]);
    }
    return p;
}

LP_HD inline double lp_frac(int64_t i, int64_t n) { return ((double)i + 0.5) / (double)n; }

// the centre of the voxel with crystal coordinates f
template <class P> LP_HD inline void lp_center(const P &c, const double f[3], double x[3])
{
    for (int k = 0; k < 3; k++) x[k] = (f[0] * c.cm[3 * k] + f[1] * c.cm[3 * k + 1]) + f[2] * c.cm[3 * k + 2];
}

// T(m) of barrier_plan.h
template <class P> LP_HD inline void lp_translation(const P &c, int m0, int m1, int m2, double T[3])
{
    T[0] = ((double)m0 * c.cm[0] + (double)m1 * c.cm[1]) + (double)m2 * c.cm[2];
    T[1] = ((double)m0 * c.cm[3] + (double)m1 * c.cm[4]) + (double)m2 * c.cm[5];
    T[2] = ((double)m0 * c.cm[6] + (double)m1 * c.cm[7]) + (double)m2 * c.cm[8];
}

// e += the term of the atom at s with the translation T and the parameters par, if it is counted
template <class Phi> LP_HD inline void lp_add_term(const double x[3], const double s[3], const double T[3], const double *par, double rc2,
                                                   double &e)
{
    const double b0 = x[0] - s[0], b1 = x[1] - s[1], b2 = x[2] - s[2];
    const double d0 = b0 - T[0], d1 = b1 - T[1], d2 = b2 - T[2];
    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
    if (dd <= rc2) e += Phi::phi(dd, par);
}

// the direct form: e += every counted term of the atom of `atom` (a bp_atom record) at the voxel centre x with crystal
// coordinates f, in ascending m; the return value is the number of triples walked
template <class Phi, class P> LP_HD inline int64_t lp_atom_add(const P &c, const BarrierPlan &pl, const double *atom, const double x[3],
                                                               const double f[3], double &e)
{
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        bp_axis_range(f[a] - atom[3 + a], pl.q[a], pl.n[a], &lo[a], &hi[a]);
        if (lo[a] > hi[a]) return 0;
    }
    for (int m0 = lo[0]; m0 <= hi[0]; m0++)
        for (int m1 = lo[1]; m1 <= hi[1]; m1++)
            for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                double T[3];
                lp_translation(c, m0, m1, m2, T);
                lp_add_term<Phi>(x, atom, T, atom + 6, pl.rc2, e);
            }
    return (int64_t)(hi[0] - lo[0] + 1) * (int64_t)(hi[1] - lo[1] + 1) * (int64_t)(hi[2] - lo[2] + 1);
}

// ---- the tiled form ---------------------------------------------------------------------------------------------------------------

struct LpTile {
    int64_t o[3];                                      // the first voxel
    int cnt[3];                                        // voxels along every axis, 1 .. the tile's edge
    double fc[3], half[3];                             // the central crystal coordinate and the half-extent of the voxel centres
};

LP_HD inline LpTile lp_tile(const LandscapePlan &p, int64_t t)
{
    LpTile tl;
    const int64_t at[3] = {t / (p.tiles[1] * p.tiles[2]), t / p.tiles[2] % p.tiles[1], t % p.tiles[2]};
    for (int a = 0; a < 3; a++) {
        const int64_t edge = lp_tile_edge(a), left = p.n[a] - at[a] * edge;
        tl.o[a] = at[a] * edge;
        tl.cnt[a] = (int)(left < edge ? left : edge);
        tl.fc[a] = ((double)tl.o[a] + 0.5 * (double)tl.cnt[a]) / (double)p.n[a];
        tl.half[a] = (0.5 * (double)(tl.cnt[a] - 1)) / (double)p.n[a];
    }
    return tl;
}

// the voxel of thread x of a tile: false outside a partial tile
LP_HD inline bool lp_tile_voxel(const LpTile &tl, int x, int64_t i[3])
{
    const int l[3] = {x / (LP_TILE1 * LP_TILE2), x / LP_TILE2 % LP_TILE1, x % LP_TILE2};
    for (int a = 0; a < 3; a++) i[a] = tl.o[a] + l[a];
    return l[0] < tl.cnt[0] && l[1] < tl.cnt[1] && l[2] < tl.cnt[2];
}

// the triples of one atom (ci(s) in `crystal`) in a tile's list: lo[a] .. hi[a] on every axis; the return value is their number
LP_HD inline int64_t lp_tile_range(const BarrierPlan &pl, const LpTile &tl, const double crystal[3], int lo[3], int hi[3])
{
    int64_t count = 1;
    for (int a = 0; a < 3; a++) {
        bp_axis_range(tl.fc[a] - crystal[a], pl.q[a] + tl.half[a], lp_wide(pl.q[a], tl.half[a]), &lo[a], &hi[a]);
        if (lo[a] > hi[a]) return 0;
        count *= (int64_t)(hi[a] - lo[a] + 1);
    }
    return count;
}

// entry k of an atom's triples in ascending (m0, m1, m2), as a list record
template <class P> LP_HD inline void lp_record(const P &c, const double *atom, const int lo[3], const int hi[3], int64_t k, double *rec)
{
    const int64_t c1 = hi[1] - lo[1] + 1, c2 = hi[2] - lo[2] + 1;
    const int m0 = lo[0] + (int)(k / (c1 * c2)), m1 = lo[1] + (int)(k / c2 % c1), m2 = lo[2] + (int)(k % c2);
    for (int j = 0; j < 3; j++) rec[j] = atom[j];
    lp_translation(c, m0, m1, m2, rec + 3);
    for (int j = 6; j < LP_REC; j++) rec[j] = atom[j];
}

// An atom's entries hold the places [off, off + cnt) of its batch; those of them within the window [w0, w1) are its entries
// [*k0, *k1) (none: *k0 >= *k1)
LP_HD inline void lp_window(int64_t off, int64_t cnt, int64_t w0, int64_t w1, int64_t *k0, int64_t *k1)
{
    *k0 = (w0 > off ? w0 : off) - off;
    *k1 = (w1 < off + cnt ? w1 : off + cnt) - off;
}

// every thread's run over a chunk of `fill` records
template <class Phi> LP_HD inline void lp_run_chunk(const double *list, int fill, const double x[3], double rc2, double &e)
{
    for (int j = 0; j < fill; j++) {
        const double *r = list + j * LP_REC;
        lp_add_term<Phi>(x, r, r + 3, r + 6, rc2, e);
    }
}

#ifndef __HIPCC__
// The schedule of the tiled kernel for one tile, one thread after the other: e[x] for the LP_BLOCK threads (0.0 outside a partial
// tile), the chunks it took and the entries of the list; `triples`, where given, receives (s, m0, m1, m2) of every entry in list
// order.  `atoms`: S bp_atom records.
template <class Phi, class P> inline void lp_tile_serial(const P &c, const LandscapePlan &p, const double *atoms, int64_t S, int64_t t,
                                                         double *e, int64_t *chunks, int64_t *entries, int64_t *triples)
{
    const LpTile tl = lp_tile(p, t);
    double *list = new double[LP_CHUNK * LP_REC];
    double x[LP_BLOCK][3];
    bool live[LP_BLOCK];
    for (int th = 0; th < LP_BLOCK; th++) {
        int64_t i[3];
        live[th] = lp_tile_voxel(tl, th, i);
        const double f[3] = {lp_frac(i[0], p.n[0]), lp_frac(i[1], p.n[1]), lp_frac(i[2], p.n[2])};
        lp_center(c, f, x[th]);
        e[th] = 0.0;
    }
    int fill = 0;
    *chunks = 0; *entries = 0;
    const auto run = [&]() {
        for (int th = 0; th < LP_BLOCK; th++)
            if (live[th]) lp_run_chunk<Phi>(list, fill, x[th], p.bp.rc2, e[th]);
        (*chunks)++;
        fill = 0;
    };
    for (int64_t first = 0; first < S; first += LP_BLOCK) {
        const int batch = (int)(S - first < LP_BLOCK ? S - first : LP_BLOCK);
        int lo[LP_BLOCK][3], hi[LP_BLOCK][3];
        int64_t cnt[LP_BLOCK], off[LP_BLOCK], total = 0;
        for (int th = 0; th < batch; th++) {
            cnt[th] = lp_tile_range(p.bp, tl, atoms + (first + th) * BP_REC + 3, lo[th], hi[th]);
            off[th] = total;
            total += cnt[th];
        }
        for (int64_t done = 0; done < total;) {
            const int64_t room = LP_CHUNK - fill, take = total - done < room ? total - done : room;
            for (int th = 0; th < batch; th++) {
                int64_t k0, k1;
                lp_window(off[th], cnt[th], done, done + take, &k0, &k1);
                for (int64_t k = k0; k < k1; k++) {
                    const int64_t slot = fill + (off[th] + k - done);
                    lp_record(c, atoms + (first + th) * BP_REC, lo[th], hi[th], k, list + slot * LP_REC);
                    if (triples) {
                        const int64_t c1 = hi[th][1] - lo[th][1] + 1, c2 = hi[th][2] - lo[th][2] + 1;
                        int64_t *out = triples + 4 * (*entries + done + (slot - fill));
                        out[0] = first + th; out[1] = lo[th][0] + k / (c1 * c2); out[2] = lo[th][1] + k / c2 % c1; out[3] = lo[th][2] + k % c2;
                    }
                }
            }
            fill += (int)take; done += take;
            if (fill == LP_CHUNK) run();
        }
        *entries += total;
    }
    if (fill) run();
    delete[] list;
}
#endif
