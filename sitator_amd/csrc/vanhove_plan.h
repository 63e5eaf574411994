// Every decision of the van Hove correlation function (vanhove.hip), in ONE place: the bin of a squared distance, the table
// of squared edges, the fractional coordinate and the minimum image of a pair (the origins of a lag are series_plan.h's),
// the largest r_max a cell allows, the split of the pairs over workgroups, the windows of frames and the batches of atoms
// that fit a workspace cap, and - vh_layout(), the one place that names them - the pieces of a call's device buffer.  Host
// and device arithmetic only: no HIP call, no context, no side effect (tests/test_vanhove_plan.py compiles it with g++ under
// ASan / UBSan).
//
// Definitions.  Cell rows c_0..c_2, ci = inverse(cell^T), lists a and b of atoms, lags tau, origins
// t = 0, s, 2 s, .. while t + tau <= F - 1:
//   distinct  s = x . ci per atom and frame; ds = s_b(t + tau) - s_a(t); ds -= nearbyint(ds); d = (ds_0 c_0 + ds_1 c_1) + ds_2 c_2;
//             r2 = (d_x^2 + d_y^2) + d_z^2; with `same` the pairs of equal position in the lists are left out
//   self      d = y[t + tau] - y[t] of the unwrapped series of section 20 (unwrap off: y = x), r2 as above, no image
//   bins      e2[k] = (k (r_max / n_bins))^2, e2[n_bins] = r_max^2; bin k holds e2[k] <= r2 < e2[k + 1]; everything else,
//             a NaN included, is the overflow entry n_bins
#pragma once
#include <math.h>
#include <stdint.h>

#include "scratch_carve.h"
#include "series_plan.h"

#define VH_THREADS 256                            // threads of a workgroup of either kernel: four waves
#define VH_WAVE 64
#define VH_WAVES (VH_THREADS / VH_WAVE)
#define VH_MAX_BINS 2048                          // bins of a call: the edges and four histograms stay below 64 KB of LDS
#define VH_MAX_ATOMS ((int64_t)1 << 20)           // atoms of a list: one item (n_a x 64 pairs) stays below 2^26 pairs
#define VH_MAX_F ((int64_t)1 << 29)               // as sit_msd
#define VH_TARGET_PAIRS ((int64_t)1 << 20)        // pairs a distinct workgroup aims at: a flush of n_bins + 1 atomics per 2^20
#define VH_MAX_PAIRS ((int64_t)1 << 31)           // pairs a workgroup may count: its LDS counters are uint32
#define VH_SELF_RUN 4096                          // origins of a self workgroup: sixteen per thread
#define VH_MAX_FRAC ((int64_t)1 << 36)            // (frame, atom) elements of one k_series_frac launch: 2^28 workgroups
#define VH_MAX_GRID_YZ 65535

// ---- the bins ---------------------------------------------------------------------------------------------------------

// e2[0 .. n_bins]
inline void vh_edges2(double r_max, int64_t n_bins, double *e2)
{
    const double dr = r_max / (double)n_bins;
    for (int64_t k = 0; k < n_bins; k++) { const double e = (double)k * dr; e2[k] = e * e; }
    e2[n_bins] = r_max * r_max;
}

// The bin of r2 from any first guess: n_bins (overflow) unless 0 <= r2 < e2[n_bins] - a NaN fails the comparison - and else
// the k the guess is walked to, down while r2 < e2[k], up while r2 >= e2[k + 1].  e2 does not decrease, so this is the last
// k with e2[k] <= r2: numpy's searchsorted(e2, r2, "right") - 1.
MSD_HD int64_t vh_bin(double r2, const double *e2, int64_t n_bins, int64_t guess)
{
    if (!(r2 < e2[n_bins]) || !(r2 >= 0.0)) return n_bins;
    int64_t k = guess < 0 ? 0 : guess > n_bins - 1 ? n_bins - 1 : guess;
    while (k > 0 && r2 < e2[k]) k--;
    while (k < n_bins - 1 && r2 >= e2[k + 1]) k++;
    return k;
}

// the first guess of the kernels: single precision is enough, the walk decides
MSD_HD int64_t vh_guess(double r2, float inv_dr) { return (int64_t)(sqrtf((float)r2) * inv_dr); }

// ---- a pair ------------------------------------------------------------------------------------------------------------

// the squared length of the minimum image of the fractional difference (ds0, ds1, ds2): cm = cell^T, as msd_unwrap reads it
MSD_HD double vh_image_r2(double ds0, double ds1, double ds2, const double *cm)
{
    ds0 -= nearbyint(ds0); ds1 -= nearbyint(ds1); ds2 -= nearbyint(ds2);
    const double dx = (ds0 * cm[0] + ds1 * cm[1]) + ds2 * cm[2];
    const double dy = (ds0 * cm[3] + ds1 * cm[4]) + ds2 * cm[5];
    const double dz = (ds0 * cm[6] + ds1 * cm[7]) + ds2 * cm[8];
    return (dx * dx + dy * dy) + dz * dz;
}

MSD_HD double vh_r2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

// ---- r_max (the origins of a lag: series_origins of series_plan.h) --------------------------------------------------------

// the name the probe of tests/test_vanhove_plan.py asks for; the library calls series_origins
inline int64_t vh_origins(int64_t F, int64_t tau, int64_t stride) { return series_origins(F, tau, stride); }

// the smallest perpendicular height of the cell: 1 / |row a of ci| (what the context keeps as hmin once it has a basis)
inline double vh_hmin(const double *ci)
{
    double hm = INFINITY;
    for (int a = 0; a < 3; a++) {
        const double *r = ci + 3 * a;
        const double h = 1.0 / sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (!(h >= hm)) hm = h;                                   // a NaN height stays
    }
    return hm;
}

// 0 < r_max <= hmin / 2 (1 - 2^-30).  A pair within r_max has |ds_a| h_a <= r_max for every a, so its true |ds_a| is at most
// 1/2 - 2^-31 and the rounded image is the nearest one as long as the computed ds is within 2^-31 of the true one.  ds is
// the difference of two s = x . ci, each three products and two sums: an error of at most 4 u (|ci[a][0] x| + |ci[a][1] y| +
// |ci[a][2] z|), u = 2^-53, and the subtraction adds u |ds|.  In a cell whose skew keeps the three terms of s within 2^18
// (atoms within about 2^18 cells of the origin) that is below 2 * 4 * 2^-53 * 2^18 + 2^-53 * 2^19 < 2^-31: the margin holds
// for every trajectory an MD code writes, and a skewed cell asks for no more than an orthorhombic one at this distance.
#define VH_RMAX_MARGIN (1.0 - 1.0 / 1073741824.0)
inline bool vh_rmax_ok(double r_max, double hmin)
{
    return r_max > 0.0 && isfinite(hmin) && hmin > 0.0 && r_max <= 0.5 * hmin * VH_RMAX_MARGIN;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------
struct VhPlanIn {
    int64_t F, n_a, n_b, n_lags, n_bins, stride;
    bool want_self, want_distinct, unwrap;
    int64_t workspace_bytes;                      // the caller's cap, 0: the default
    int hist_copies;                              // LDS histograms of a workgroup: 1 (shared) or VH_WAVES (one per wave)
};

struct VhPlan {
    // distinct: an item is one origin against 64 atoms of b (n_a x 64 pairs); a workgroup takes `run` origins against
    // b_span atoms of b (grid.z tiles of b), its four waves an item each in turn
    int64_t run, b_span, b_tiles, pairs_per_wg;
    int64_t window;                               // frames of a and of b whose fractional coordinates are held at once (F: all)
    int64_t origins_per_window;
    int64_t self_batch;                           // atoms whose series are held at once
    int64_t n_chunks;                             // of the image scan (msd_plan.h)
    int64_t lds_bytes;
    int64_t workspace;                            // bytes of the work area
    const char *err;                              // null, or why there is no launch
};

struct VhPieces {
    unsigned long long *status; int64_t *atoms, *lags; double *e2;
    unsigned long long *self_counts, *distinct_counts;
    int64_t head;                                 // the work area begins here; its two uses take turns
    double *sa, *sb;                              // distinct: [window][3][n_a], [window][3][n_b]
    double *y; int32_t *images; void *totals;     // self: the series of a batch, as msd_layout lays them out
};

// bytes of LDS of either kernel: the edges, the histograms, and (distinct) a wave's tile of 64 atoms of a
inline int64_t vh_lds_bytes(int64_t n_bins, int copies)
{
    return (n_bins + 1) * 8 + (((n_bins + 1) * 4 * copies + 7) & ~(int64_t)7) + VH_WAVES * 3 * VH_WAVE * 8;
}

inline VhPieces vh_layout(Carve &cv, const VhPlan &p, const VhPlanIn &in)
{
    const int64_t table = in.n_lags * (in.n_bins + 1), S = 3 * p.self_batch;
    VhPieces w;
    w.status = cv.take<unsigned long long>(1, 256);
    w.atoms = cv.take<int64_t>(in.n_a + in.n_b, 256);
    w.lags = cv.take<int64_t>(in.n_lags, 256);
    w.e2 = cv.take<double>(in.n_bins + 1, 256);
    w.self_counts = cv.take<unsigned long long>(in.want_self ? table : 0, 256);
    w.distinct_counts = cv.take<unsigned long long>(in.want_distinct ? table : 0, 256);
    cv.take<char>(0, 256);
    w.head = cv.used;
    w.sa = cv.take<double>(in.want_distinct ? p.window * 3 * in.n_a : 0, 256);
    w.sb = cv.take<double>(in.want_distinct ? p.window * 3 * in.n_b : 0, 256);
    const int64_t end_distinct = cv.used;
    cv.used = w.head;                             // the series of the self part lie over the fractional coordinates
    w.y = cv.take<double>(in.want_self ? S * (msd_round256(in.F * 8) / 8) : 0, 256);
    w.images = cv.take<int32_t>(in.want_self && in.unwrap ? S * (msd_round256(in.F * 4) / 4) : 0, 256);
    w.totals = cv.take<double>(in.want_self && in.unwrap ? S * (msd_round256(p.n_chunks * 8) / 8) : 0, 256);
    if (cv.used < end_distinct) cv.used = end_distinct;
    return w;
}

inline VhPlan vh_plan(const VhPlanIn &in, int64_t default_workspace)
{
    VhPlan p = VhPlan();
    if (in.F < 1 || in.F > VH_MAX_F) { p.err = "1 to 2^29 frames are needed"; return p; }
    if (in.n_lags < 1) { p.err = "an empty lag list"; return p; }
    if (in.stride < 1) { p.err = "origin_stride is below 1"; return p; }
    if (in.n_bins < 1 || in.n_bins > VH_MAX_BINS) { p.err = "n_bins is outside [1, 2048]"; return p; }
    if (in.n_a < 1 || in.n_b < 1 || in.n_a > VH_MAX_ATOMS || in.n_b > VH_MAX_ATOMS) { p.err = "a list holds no atom or more than 2^20"; return p; }
    if (!in.want_self && !in.want_distinct) { p.err = "neither part is asked for"; return p; }
    if (in.hist_copies != 1 && in.hist_copies != VH_WAVES) { p.err = "1 or 4 histograms per workgroup"; return p; }
    const int64_t cap = in.workspace_bytes > 0 ? in.workspace_bytes : default_workspace;
    p.n_chunks = msd_chunks(in.F);
    p.lds_bytes = vh_lds_bytes(in.n_bins, in.hist_copies);
    // the pairs of a distinct workgroup
    const int64_t item = in.n_a * VH_WAVE, chunks = (in.n_b + VH_WAVE - 1) / VH_WAVE;
    int64_t items = VH_TARGET_PAIRS / item;
    if (items < VH_WAVES) items = VH_WAVES;
    if (items > VH_MAX_PAIRS / item) items = VH_MAX_PAIRS / item;
    if (chunks >= items) { p.b_span = items * VH_WAVE; p.run = 1; }
    else { p.b_span = chunks * VH_WAVE; p.run = items / chunks; }
    p.b_tiles = (in.n_b + p.b_span - 1) / p.b_span;
    p.pairs_per_wg = p.run * in.n_a * p.b_span;
    // the frames whose fractional coordinates fit, the atoms whose series fit
    p.window = in.F; p.self_batch = 0;
    if (in.want_distinct) {
        const int64_t frame = (in.n_a + in.n_b) * 24, slack = 512;       // the two pieces start on 256 bytes
        const int64_t w = cap > slack ? (cap - slack) / frame : 0;
        if (w < 1) { p.err = "the workspace cap is below one window of fractional coordinates"; return p; }
        if (w < p.window) p.window = w;
        const int64_t most = VH_MAX_FRAC / (in.n_a > in.n_b ? in.n_a : in.n_b);
        if (most < p.window) p.window = most;
    }
    p.origins_per_window = (p.window - 1) / in.stride + 1;
    if (in.want_self) {
        const int64_t atom = 3 * (msd_round256(in.F * 8) + (in.unwrap ? msd_round256(in.F * 4) + msd_round256(p.n_chunks * 8) : 0)), slack = 768;
        int64_t b = cap > slack ? (cap - slack) / atom : 0;
        if (b < 1) { p.err = "the workspace cap is below one atom's series"; return p; }
        if (b > MSD_MAX_BATCH) b = MSD_MAX_BATCH;
        if (b > in.n_a) b = in.n_a;
        p.self_batch = b;
    }
    Carve cv = {nullptr, 0};
    const VhPieces w = vh_layout(cv, p, in);
    p.workspace = cv.used - w.head;
    return p;
}
