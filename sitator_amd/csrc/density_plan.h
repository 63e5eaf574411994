// Every decision of the ionic density (density.hip), in ONE place: the voxel of a point, the plane of a label, the slot and the
// probe sequence of the workgroup's count table, the peak rule, the limits, the frames of a run, the frames uploaded at once
// under a workspace cap, the smoothing tile and its halo, the form that 0 resolves to, and - dn_layout(), the one place that
// names them - the pieces of a call's device buffer.  Host and device arithmetic only: no HIP call, no context, no side effect
// (tests/test_density_plan.py compiles it with g++ under ASan / UBSan).  No fma: every product and every sum below is one
// rounded float64 operation (-ffp-contract=off), which numpy repeats bit for bit (tests/density_ref.py).
//
// Definitions.  ci = inverse(cell^T), grid n = (n0, n1, n2), V = n0 n1 n2:
//   voxel     s_a = (ci[a][0] x + ci[a][1] y) + ci[a][2] z (msd_frac), f_a = s_a - floor(s_a), g_a = f_a n_a (one rounded
//             product), i_a = (int64) g_a, n_a - 1 where that is n_a or more; v = (i0 n1 + i1) n2 + i2.  An s_a that is not
//             finite: no voxel, the entry is counted in `skipped`
//   plane     no labels: 0; label l >= 0: site_class[l]; l == -1: n_classes - 1
//   counts    [plane][v] += 1 for every (taken frame, selected atom); taken frames are 0, s, 2 s, .. below F
//   smoothed  [p][v] = sum over the taps k in list order, from +0, of w_k * (double) counts[p][(i + d_k) mod n]
//   peak      grid[v] >= threshold and, for every one of the 26 periodic neighbours u != v, grid[u] < grid[v] or grid[u] ==
//             grid[v] and u > v: a total order on (value, index)
#pragma once
#include <math.h>
#include <stdint.h>

#include "scratch_carve.h"
#include "series_plan.h"

#define DN_THREADS 256                            // threads of a workgroup of every kernel: four waves
#define DN_MAX_GRID 1024                          // voxels along an axis
#define DN_MAX_CLASSES 16
#define DN_MAX_CELLS ((int64_t)1 << 27)           // n_classes x V: a key of the table is a uint32
#define DN_MAX_F ((int64_t)1 << 29)               // as sit_msd
#define DN_MAX_ATOMS ((int64_t)1 << 20)           // atoms of a selection, as sit_vanhove
#define DN_MAX_TAPS ((int64_t)1 << 15)
#define DN_MAX_ENTRIES ((int64_t)1 << 53)         // a count converts to a double exactly
#define DN_RUN 64                                 // taken frames of a workgroup of k_dn_count: at most 2^26 entries, a uint32 count
#define DN_SLOT_BITS 12
#define DN_SLOTS (1 << DN_SLOT_BITS)              // slots of the table: a uint32 key and a uint32 count each, 32 KB of LDS
#define DN_PROBE 16                               // slots an entry tries before it goes to memory on its own
#define DN_EMPTY 0xFFFFFFFFu                      // no key: n_classes x V stays below it
#define DN_TILE0 4                                // the smoothing tile: 4 x 8 x 8 voxels, one per thread, the last axis across lanes
#define DN_TILE1 8
#define DN_TILE2 8
#define DN_SMOOTH_LDS 61440                       // bytes the haloed tile may take as doubles; beyond it the taps read memory
#define DN_FORM_DIRECT 1
#define DN_FORM_TABLE 2

// ---- the voxel ----------------------------------------------------------------------------------------------------------

// the index along an axis of n voxels of the fractional coordinate s; -1 where s is not finite
MSD_HD int64_t dn_axis(double s, int64_t n)
{
    if (!(fabs(s) < INFINITY)) return -1;                        // NaN fails the comparison too
    const double f = s - floor(s);                               // [0, 1]: 1 for a tiny negative s
    const double g = f * (double)n;
    const int64_t i = (int64_t)g;
    return i >= n ? n - 1 : i;
}

// the voxel of (x, y, z), or -1
MSD_HD int64_t dn_voxel(const double *ci, const int64_t *n, double x, double y, double z)
{
    const int64_t i0 = dn_axis(msd_frac(ci, 0, x, y, z), n[0]);
    const int64_t i1 = dn_axis(msd_frac(ci, 1, x, y, z), n[1]);
    const int64_t i2 = dn_axis(msd_frac(ci, 2, x, y, z), n[2]);
    if ((i0 | i1 | i2) < 0) return -1;
    return (i0 * n[1] + i1) * n[2] + i2;
}

// the plane of a label in [-1, K): the caller has looked at the label first
MSD_HD int64_t dn_plane(int64_t label, const int32_t *site_class, int64_t n_classes)
{
    return label < 0 ? n_classes - 1 : (int64_t)site_class[label];
}

// ---- the table of a workgroup --------------------------------------------------------------------------------------------

// the first slot of a key (Knuth's multiplicative hash, the top bits) and the i-th slot of its probe sequence
MSD_HD uint32_t dn_slot(uint32_t key) { return (uint32_t)(key * 2654435761u) >> (32 - DN_SLOT_BITS); }
MSD_HD uint32_t dn_probe(uint32_t slot, int i) { return (slot + (uint32_t)i) & (DN_SLOTS - 1); }

// ---- the peak rule --------------------------------------------------------------------------------------------------------

MSD_HD int64_t dn_wrap(int64_t i, int64_t n) { return ((i % n) + n) % n; }

MSD_HD bool dn_is_peak(const double *grid, const int64_t *n, int64_t v, double threshold)
{
    const double c = grid[v];
    if (!(c >= threshold)) return false;                         // a NaN never passes
    const int64_t i2 = v % n[2], i1 = (v / n[2]) % n[1], i0 = v / (n[1] * n[2]);
    for (int d0 = -1; d0 <= 1; d0++)
        for (int d1 = -1; d1 <= 1; d1++)
            for (int d2 = -1; d2 <= 1; d2++) {
                const int64_t u = (dn_wrap(i0 + d0, n[0]) * n[1] + dn_wrap(i1 + d1, n[1])) * n[2] + dn_wrap(i2 + d2, n[2]);
                if (u == v) continue;                            // the voxel itself, also through an axis of one or two voxels
                const double g = grid[u];
                if (!(g < c || (g == c && u > v))) return false;
            }
    return true;
}

// ---- the validation of the lists --------------------------------------------------------------------------------------

// the largest |d_a| of the taps into halo[3]; false for a tap with |d_a| > (n_a - 1) / 2
inline bool dn_halo(const int64_t *taps, int64_t n_taps, const int64_t *n, int64_t *halo)
{
    halo[0] = halo[1] = halo[2] = 0;
    for (int64_t i = 0; i < 3 * n_taps; i++) {
        const int a = (int)(i % 3);
        const int64_t d = taps[i], m = (n[a] - 1) / 2;
        if (d < -m || d > m) return false;
        if ((d < 0 ? -d : d) > halo[a]) halo[a] = d < 0 ? -d : d;
    }
    return true;
}

// the names the probe of tests/test_density_plan.py asks for; the library calls the shared ones of series_plan.h
template <typename T> inline int64_t dn_first_outside(const T *list, int64_t n, int64_t lo, int64_t hi) { return series_first_outside(list, n, lo, hi); }
inline bool dn_cell_ok(const double *m, const double *ci) { return series_cell_ok(m, ci); }

// ---- the plan -----------------------------------------------------------------------------------------------------------
struct DnPlanIn {
    int64_t F, A;                                 // frames; atoms of a frame of the source
    int64_t n_sel, stride;
    int64_t n[3];
    int64_t K, n_classes;                         // sites of site_class (0: no labels) and planes
    int64_t n_taps, halo[3];                      // dn_halo
    int64_t form;
    bool host;                                    // the positions are a host array: frames are uploaded in windows
    int64_t workspace_bytes;                      // the caller's cap, 0: the default
};

struct DnPlan {
    int64_t V, cells;                             // voxels of a plane, of all planes
    int64_t taken, runs;                          // frames taken, workgroups of k_dn_count over all of them
    int64_t form;                                 // DN_FORM_DIRECT or DN_FORM_TABLE
    int64_t lds_bytes;                            // of k_dn_count
    int64_t window, n_windows;                    // taken frames uploaded at once (whole runs); resident frames: all, once
    int64_t window_frames;                        // frames from the first to the last taken one of a full window
    int64_t ext[3];                               // the haloed smoothing tile
    int64_t smooth_lds;                           // bytes of the haloed tile in LDS, 0: the taps read memory
    int64_t workspace;                            // bytes of the work area
    const char *err;                              // null, or why there is no launch
};

struct DnPieces {
    int64_t *atoms; int32_t *site_class, *taps; double *weights; unsigned long long *status, *counts; double *smoothed;
    int64_t head;                                 // the work area begins here
    double *upload;                               // [window_frames][A][3]
};

inline DnPieces dn_layout(Carve &cv, const DnPlan &p, const DnPlanIn &in)
{
    DnPieces w;
    w.atoms = cv.take<int64_t>(in.n_sel, 256);
    w.site_class = cv.take<int32_t>(in.K, 256);
    w.taps = cv.take<int32_t>(in.n_taps * 3, 256);
    w.weights = cv.take<double>(in.n_taps, 256);
    w.status = cv.take<unsigned long long>(4, 256);
    w.counts = cv.take<unsigned long long>(p.cells, 256);
    w.smoothed = cv.take<double>(in.n_taps > 0 ? p.cells : 0, 256);
    cv.take<char>(0, 256);
    w.head = cv.used;
    w.upload = cv.take<double>(in.host ? p.window_frames * in.A * 3 : 0, 256);
    cv.take<char>(0, 256);
    return w;
}

// frames from the first to the last of w taken frames
inline int64_t dn_span(int64_t w, int64_t stride) { return (w - 1) * stride + 1; }

inline DnPlan dn_plan(const DnPlanIn &in, int64_t default_workspace)
{
    DnPlan p = DnPlan();
    for (int a = 0; a < 3; a++)
        if (in.n[a] < 1 || in.n[a] > DN_MAX_GRID) { p.err = "an axis of the grid holds 1 to 1024 voxels"; return p; }
    if (in.n_classes < 1 || in.n_classes > DN_MAX_CLASSES) { p.err = "1 to 16 classes are needed"; return p; }
    if (in.K < 0 || (in.K > 0 && in.n_classes < 2)) { p.err = "labels need a class of their own beside the unassigned one"; return p; }
    p.V = in.n[0] * in.n[1] * in.n[2];
    p.cells = in.n_classes * p.V;
    if (p.cells > DN_MAX_CELLS) { p.err = "more than 2^27 voxels over all classes"; return p; }
    if (in.F < 1 || in.F > DN_MAX_F) { p.err = "1 to 2^29 frames are needed"; return p; }
    if (in.stride < 1) { p.err = "frame_stride is below 1"; return p; }
    if (in.n_sel < 1 || in.n_sel > DN_MAX_ATOMS) { p.err = "a selection holds 1 to 2^20 atoms"; return p; }
    if (in.A < 1) { p.err = "no atom in a frame"; return p; }
    if (in.n_taps < 0 || in.n_taps > DN_MAX_TAPS) { p.err = "0 to 2^15 taps are taken"; return p; }
    for (int a = 0; a < 3; a++)
        if (in.halo[a] < 0 || in.halo[a] > (in.n[a] - 1) / 2) { p.err = "a tap reaches beyond (n - 1) / 2 voxels"; return p; }
    if (in.form < 0 || in.form > 2) { p.err = "form is 0, 1 or 2"; return p; }
    if (in.workspace_bytes < 0) { p.err = "a negative workspace cap"; return p; }
    p.taken = (in.F - 1) / in.stride + 1;
    if (p.taken * in.n_sel >= DN_MAX_ENTRIES) { p.err = "2^53 entries or more"; return p; }
    p.runs = (p.taken + DN_RUN - 1) / DN_RUN;
    // form 0: on a grid of 0.2 A voxels neither form was faster than the other beyond the spread of the
    // calls, so it is the direct one - except where every key has a slot of its own, nothing can spill and the adds of a run
    // to memory are at most the slots: there the aggregated form was faster by orders of magnitude (one voxel: 590 times)
    p.form = in.form ? in.form : (p.cells <= DN_SLOTS ? DN_FORM_TABLE : DN_FORM_DIRECT);
    p.lds_bytes = DN_SLOTS * 8 + 24;                             // static: the direct form is the same kernel
    if (in.host) {
        // whole runs of taken frames, as many as the cap holds; the frames between two taken ones are uploaded with them
        const int64_t cap = (in.workspace_bytes > 0 ? in.workspace_bytes : default_workspace) & ~(int64_t)255;
        const int64_t frame = in.A * 24, most = cap / frame;                   // frames the cap holds
        const int64_t first = p.taken < DN_RUN ? p.taken : DN_RUN;
        if (most < dn_span(first, in.stride)) { p.err = "the workspace cap is below one run of frames"; return p; }
        const int64_t w = (most - 1) / in.stride + 1;                          // taken frames it holds
        p.window = w >= p.taken ? p.taken : w / DN_RUN * DN_RUN;
    } else
        p.window = p.taken;
    p.n_windows = (p.taken + p.window - 1) / p.window;
    p.window_frames = dn_span(p.window, in.stride);
    const int64_t tile[3] = {DN_TILE0, DN_TILE1, DN_TILE2};
    for (int a = 0; a < 3; a++) p.ext[a] = tile[a] + 2 * in.halo[a];
    const int64_t ext_bytes = p.ext[0] * p.ext[1] * p.ext[2] * 8;
    p.smooth_lds = in.n_taps > 0 && ext_bytes <= DN_SMOOTH_LDS ? ext_bytes : 0;
    Carve cv = {nullptr, 0};
    const DnPieces w = dn_layout(cv, p, in);
    p.workspace = cv.used - w.head;
    return p;
}
