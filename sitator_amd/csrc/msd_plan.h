// Every decision of the mean squared displacement (msd.hip), in ONE place: the rounding of a step to its periodic
// image, the operation order of the unwrapped position, the chunks of the two scans along the frames and the order of
// their sums, the windowed term S1, the combination with the autocorrelation, the atoms per batch, and - msd_layout(), the
// one place that names them - the pieces of a call's device buffer, from which the plan takes its byte counts.  Host and device
// arithmetic only: no HIP call, no context, no side effect (tests/test_msd_plan.py compiles it with g++ under ASan / UBSan).
//
// Definitions.  For a selected atom with positions x[t], t = 0..F-1, under the cell with rows c_0..c_2:
//   d = x[t] - x[t-1], f = d . cell^-1, n_a = nearbyint(f_a) (0 where f_a is not finite), shift[t] = -n, shift[0] = 0,
//   N[t] = sum_{s<=t} shift[s] (int32, exact), x_u[t] = x[t] + (N_0 c_0 + N_1 c_1 + N_2 c_2), y[t] = x_u[t] - x_u[0],
//   msd(tau) = (1 / (F - tau)) sum_{t < F - tau} (y[t + tau] - y[t])^2 = S1(tau) - 2 acf(tau) / (F - tau),
//   S1(tau) = (P[F - tau] + (P[F] - P[tau])) / (F - tau), P[k] = sum_{t<k} y[t]^2, acf(tau) = sum_t y[t] y[t + tau].
#pragma once
#include <math.h>
#include <stdint.h>

#include "spectrum_plan.h"

#if defined(__HIPCC__)
#define MSD_HD __host__ __device__ inline
#else
#define MSD_HD inline
#endif

#define MSD_THREADS 256                           // threads of a scan workgroup
#define MSD_GROUP 4                               // consecutive elements a thread sums on its own
#define MSD_CHUNK (MSD_THREADS * MSD_GROUP)       // elements of a chunk of either scan
#define MSD_MAX_BATCH 16384                       // atoms of one launch: three series each in grid.y
#define MSD_MAX_F ((int64_t)1 << 29)              // the padded length of the transform stays within 2^30
#define MSD_IMAGE_LIMIT 1073741824.0              // 2^30: a step of more images than this is treated like a non-finite one

// the periodic images a step of f cell vectors crosses: round to nearest, ties to even; 0 where f is not finite (or
// beyond what an int32 sum can hold).  *residual = |f - n| in [0, 0.5], or -1 where the step does not count
MSD_HD int32_t msd_image(double f, double *residual)
{
    if (!(fabs(f) < MSD_IMAGE_LIMIT)) { *residual = -1.0; return 0; }        // NaN and +-inf fail the comparison too
    const double n = nearbyint(f);
    *residual = fabs(f - n);
    return (int32_t)n;
}

// coordinate a of a step in units of the cell vectors: ci = inverse(cell^T), rows summed left to right (as wrap3 does)
MSD_HD double msd_frac(const double *ci, int a, double dx, double dy, double dz)
{
    return (ci[3 * a] * dx + ci[3 * a + 1] * dy) + ci[3 * a + 2] * dz;
}

// coordinate a of the unwrapped position: cm = cell^T (cm[3 a + i] is coordinate a of cell vector i).  No image: the
// position itself, bit for bit (also a negative zero)
MSD_HD double msd_unwrap(double x, int32_t n0, int32_t n1, int32_t n2, const double *cm, int a)
{
    if ((n0 | n1 | n2) == 0) return x;
    return x + (((double)n0 * cm[3 * a] + (double)n1 * cm[3 * a + 1]) + (double)n2 * cm[3 * a + 2]);
}

// ---- the scans along the frames ---------------------------------------------------------------------------------------
// Both (the int32 image sums; P, the float64 sums of y^2) take chunks of MSD_CHUNK consecutive elements; an element
// beyond F counts as zero.  Inside a chunk thread j sums elements 4 j .. 4 j + 3 one after the other (`local`), the
// MSD_THREADS group totals are scanned by msd_group_scan, and the chunk totals are added up one after the other in chunk
// order (`offset`, exclusive).  The inclusive sum at an element is  offset + (groups before + local) : msd_scan_value.
// Integer adds are exact, so for the images the order does not matter; for P it is this order and no other.
MSD_HD int64_t msd_chunks(int64_t F) { return (F + MSD_CHUNK - 1) / MSD_CHUNK; }

// inclusive scan of g[0 .. MSD_THREADS) in place: Hillis-Steele, steps d = 1, 2, 4, ..: g[j] <- g[j - d] + g[j] for
// j >= d, every right-hand side read before any element of the step is written (tmp: MSD_THREADS elements).  The kernels
// run the same steps with one thread per j.
template <typename T> inline void msd_group_scan(T *g, T *tmp)
{
    for (int d = 1; d < MSD_THREADS; d <<= 1) {
        for (int j = 0; j < MSD_THREADS; j++) tmp[j] = j >= d ? g[j - d] + g[j] : g[j];
        for (int j = 0; j < MSD_THREADS; j++) g[j] = tmp[j];
    }
}

template <typename T> MSD_HD T msd_scan_value(T offset, T groups_before, T local) { return offset + (groups_before + local); }

// the windowed term from the prefix sums P[0 .. F] of one series
MSD_HD double msd_s1(const double *P, int64_t F, int64_t tau)
{
    return (P[F - tau] + (P[F] - P[tau])) / (double)(F - tau);
}

// msd(tau) from S1 and the raw circular autocorrelation `re` (the stage-by-stage inverses leave a factor M = 1 / inv_m)
MSD_HD double msd_combine(double s1, double re, double inv_m, int64_t F, int64_t tau)
{
    if (tau == 0) return 0.0;
    return s1 - 2.0 * (re * inv_m) / (double)(F - tau);
}

// ---- the batches --------------------------------------------------------------------------------------------------------
struct MsdPlanIn {
    int64_t F, n_sel, n_lags;
    bool direct;                                  // an explicit lag list: no transform
    bool collective;
    int64_t workspace_bytes;                      // the caller's cap, 0: the knob's
};

struct MsdPlan {
    SpPlan sp;                                    // the passes of the transform (n = F, so M >= 2 F - 1); unused when direct
    int64_t n_chunks;
    int64_t atom_bytes;                           // workspace of one atom (three series)
    int64_t fixed_bytes;                          // the collective series, whatever the batch
    int64_t atoms_per_batch, n_batches, workspace;
    const char *err;                              // null, or why there is no launch
};

inline int64_t msd_round256(int64_t v) { return (v + 255) / 256 * 256; }

// The device buffer of a call: a head, then, from `head` bytes on, the plan's workspace - the collective series, whatever
// the batch, and for each of the 3 B series of a batch of B atoms y, N, P (F + 1 values), the chunk totals of a scan (int32
// or float64), the transform's M complex points as (re, im) pairs, the results (msd; r4 is a fourth row of an atom).  A
// series' piece is sized in whole units of 256 bytes; what is not needed takes nothing.
struct MsdPieces {
    unsigned long long *status; int64_t *atoms, *lags;
    int64_t head;
    double *coll_y, *y; int32_t *images; double *psum; void *totals; double *buf, *out, *r4;
};

inline MsdPieces msd_layout(Carve &cv, const MsdPlan &p, const MsdPlanIn &in, int64_t B)
{
    const int64_t S = 3 * B, y = msd_round256(in.F * 8) / 8, out = msd_round256(in.n_lags * 8) / 8;
    MsdPieces w;
    w.status = cv.take<unsigned long long>(1, 256);
    w.atoms = cv.take<int64_t>(in.n_sel, 256);
    w.lags = cv.take<int64_t>(in.direct ? in.n_lags : 0, 256);
    cv.take<char>(0, 256);
    w.head = cv.used;
    w.coll_y = cv.take<double>(in.collective ? 3 * y : 0);
    w.y = cv.take<double>(S * y);
    w.images = cv.take<int32_t>(S * (msd_round256(in.F * 4) / 4));
    w.psum = cv.take<double>(in.direct ? 0 : S * (msd_round256((in.F + 1) * 8) / 8));
    w.totals = cv.take<double>(S * (msd_round256(p.n_chunks * 8) / 8));
    w.buf = cv.take<double>(in.direct ? 0 : S * p.sp.M * 2);
    w.out = cv.take<double>(S * out);
    w.r4 = cv.take<double>(in.direct ? B * out : 0);
    return w;
}

inline MsdPlan msd_plan(const MsdPlanIn &in, const SpKnobs &k)
{
    MsdPlan p = MsdPlan();
    if (in.F < 2 || in.F > MSD_MAX_F) { p.err = "the mean squared displacement needs 2 to 2^29 frames"; return p; }
    if (in.n_lags < 1 || in.n_sel < 0) { p.err = "no lag"; return p; }
    p.n_chunks = msd_chunks(in.F);
    if (!in.direct) {
        SpPlanIn si;
        si.n = in.F; si.n_sel = 1; si.workspace_bytes = (int64_t)1 << 62; si.want_spectrum = false;
        p.sp = sp_plan(si, k);
        if (p.sp.err) { p.err = p.sp.err; return p; }
    }
    Carve none = {nullptr, 0}, one = {nullptr, 0};
    const int64_t head = msd_layout(none, p, in, 0).head;
    msd_layout(one, p, in, 1);
    p.fixed_bytes = none.used - head;
    p.atom_bytes = one.used - none.used;
    const int64_t cap = in.workspace_bytes > 0 ? in.workspace_bytes : k.workspace;
    int64_t b = (cap - p.fixed_bytes) / p.atom_bytes;
    if (cap < p.fixed_bytes || b < 1) { p.err = "the workspace cap is below one atom's series and transform"; return p; }
    if (b > MSD_MAX_BATCH) b = MSD_MAX_BATCH;
    if (in.n_sel > 0 && b > in.n_sel) b = in.n_sel;
    p.atoms_per_batch = b;
    p.n_batches = in.n_sel > 0 ? (in.n_sel + b - 1) / b : 0;
    p.workspace = p.fixed_bytes + b * p.atom_bytes;
    return p;
}
