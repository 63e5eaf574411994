// The launch plan of the speed power spectrum (spectrum.hip), decided in ONE place: sp_plan() takes the transform length
// and the SITATOR_SPECTRUM_* knobs and returns the padded length, the passes, the LDS of every pass, the atoms per batch
// and the workspace; sp_layout() is the one place that names the pieces of a call's device buffer, and the plan takes its
// byte counts from it.  Host arithmetic only: no HIP call, no context, no side effect (tests/test_vibfreq_ref.py compiles
// it with g++).
//
// Bluestein: a transform of arbitrary length n is a circular convolution of length M = 2^m >= 2n - 1.  The M points of
// an atom are factored M = L_1 x ... x L_p (p <= 3, every L_i <= 1024): pass i transforms, inside every block of
// L_i x S_i consecutive points (S_i = L_{i+1} ... L_p), the L_i points that lie S_i apart, wholly in LDS.  A workgroup
// takes T_i such transforms ("lines") at once: adjacent columns of a block where S_i >= T_i, so that every row it reads
// from global memory is one run of T_i x 16 bytes; consecutive rows at the last level (S_p = 1).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "scratch_carve.h"

#define SP_MAX_PASS 3
#define SP_MAX_STAGE_BITS 10                      // a 1024-point complex float64 line is 16 KB of LDS
#define SP_MAX_N ((int64_t)1 << 29)               // M <= 2^30
#define SP_THREADS 256
#define SP_TILE_POINTS 4096                       // points a workgroup holds: 64 KB, two workgroups per CU
#define SP_MAX_LINES 16
#define SP_MAX_BATCH 32768                        // atoms of one launch (grid.y)
#define SP_LDS_PER_CU ((size_t)160 * 1024)
#define SP_LDS_LIMIT (SP_LDS_PER_CU - 256)
#define SP_DEFAULT_WORKSPACE ((int64_t)1 << 30)

struct SpKnobs {
    int64_t workspace;                            // SITATOR_SPECTRUM_WORKSPACE_MB: the cap when the caller passes 0
    int stage_bits;                               // SITATOR_SPECTRUM_STAGE_BITS: most stages of a pass (1..10)
    int lines;                                    // SITATOR_SPECTRUM_LINES: most lines per workgroup (1..16, power of two)
};

inline SpKnobs sp_knobs_from_env()
{
    SpKnobs k;
    const char *e = getenv("SITATOR_SPECTRUM_WORKSPACE_MB");
    const long long mb = e && *e ? atoll(e) : 0;
    k.workspace = mb > 0 ? (int64_t)mb << 20 : SP_DEFAULT_WORKSPACE;
    e = getenv("SITATOR_SPECTRUM_STAGE_BITS");
    k.stage_bits = e && *e ? atoi(e) : SP_MAX_STAGE_BITS;
    if (k.stage_bits < 1 || k.stage_bits > SP_MAX_STAGE_BITS) k.stage_bits = SP_MAX_STAGE_BITS;
    e = getenv("SITATOR_SPECTRUM_LINES");
    k.lines = e && *e ? atoi(e) : SP_MAX_LINES;
    if (k.lines < 1 || k.lines > SP_MAX_LINES || (k.lines & (k.lines - 1))) k.lines = SP_MAX_LINES;
    return k;
}

struct SpPlanIn {
    int64_t n;                                    // transform length: frames - 1
    int64_t n_sel;                                // selected atoms
    int64_t workspace_bytes;                      // the caller's cap, 0: the knob's
    bool want_spectrum;                           // the complex bins are staged in the workspace too
};

struct SpPass {
    int bits;                                     // stages: L = 2^bits
    int64_t L, S;                                 // line length; distance of a line's points (1 at the last level)
    int lines;                                    // T: lines per workgroup
    int pad;                                      // LDS: a line starts every L + pad doubles
    int64_t tiles;                                // workgroups per atom: (M / L) / T
    size_t lds;                                   // dynamic LDS of a workgroup
};

struct SpPlan {
    int log_m;
    int64_t M, nbins;                             // padded length; n / 2 + 1 bins kept
    int npass;
    SpPass pass[SP_MAX_PASS];
    int64_t atom_bytes;                           // workspace of one atom
    int64_t atoms_per_batch, n_batches, workspace;
    const char *err;                              // null, or why there is no launch
};

// LDS of a workgroup: re and im of T lines of L + pad doubles, the L / 2 twiddles of the line length, two doubles per
// thread for the band sums.  The pad puts the T points of one row, which a workgroup stores side by side when it loads
// adjacent columns, 16 / T doubles apart modulo the banks.
inline int sp_pad(int lines) { return lines >= 16 ? 1 : 16 / lines; }
inline size_t sp_lds_bytes(int64_t L, int lines)
{
    const int64_t half = L / 2 > 0 ? L / 2 : 1;
    return (size_t)(2 * lines * (L + sp_pad(lines)) + 2 * half + 2 * SP_THREADS) * 8;
}

// The device buffer of a call: a head that every batch reads, then, from `head` bytes on, the workspace of a batch of B
// atoms - per atom the M complex points (transformed in place; complex arrays are (re, im) pairs), the bins when they are
// asked for, the band sums of every workgroup of the last inverse pass, the result pair and the n speeds.
struct SpPieces {
    double *freqs; unsigned char *fmask; int64_t *atoms;
    int64_t head;
    double *buf, *spec, *partial, *result, *speeds;
};

inline SpPieces sp_layout(Carve &cv, const SpPlan &p, const SpPlanIn &in, int64_t B)
{
    SpPieces w;
    w.freqs = cv.take<double>(p.nbins);
    w.fmask = cv.take<unsigned char>(p.nbins);
    w.atoms = cv.take<int64_t>(in.n_sel);
    cv.take<char>(0, 256);
    w.head = cv.used;
    w.buf = cv.take<double>(B * p.M * 2);
    w.spec = in.want_spectrum ? cv.take<double>(B * p.nbins * 2) : nullptr;
    w.partial = cv.take<double>(B * p.pass[0].tiles * 2);
    w.result = cv.take<double>(B * 2);
    w.speeds = cv.take<double>(B * in.n);
    return w;
}

inline SpPlan sp_plan(const SpPlanIn &in, const SpKnobs &k)
{
    SpPlan p = SpPlan();
    if (in.n < 1 || in.n > SP_MAX_N) { p.err = "the spectrum needs 2 to 2^29 + 1 frames"; return p; }
    int m = 1;                                    // M >= 2 keeps every index rule below free of special cases
    while (((int64_t)1 << m) < 2 * in.n - 1) m++;
    p.log_m = m; p.M = (int64_t)1 << m; p.nbins = in.n / 2 + 1;
    p.npass = (m + k.stage_bits - 1) / k.stage_bits;
    if (p.npass > SP_MAX_PASS) { p.err = "the spectrum's padded length needs more than three passes"; return p; }
    // the stages dealt evenly, the longer lines at the later levels (the last one reads consecutive points)
    int64_t S = p.M;
    for (int i = 0; i < p.npass; i++) {
        SpPass &q = p.pass[i];
        q.bits = m / p.npass + (i >= p.npass - m % p.npass ? 1 : 0);
        q.L = (int64_t)1 << q.bits;
        S >>= q.bits;
        q.S = S;
        int64_t T = SP_TILE_POINTS >> q.bits;
        if (T > k.lines) T = k.lines;
        if (T < 1) T = 1;
        if (T > p.M / q.L) T = p.M / q.L;
        q.lines = (int)T;
        q.pad = sp_pad(q.lines);
        q.tiles = p.M / q.L / T;
        q.lds = sp_lds_bytes(q.L, q.lines);
        if (q.lds > SP_LDS_LIMIT) { p.err = "a pass of the spectrum does not fit in LDS"; return p; }
    }
    // per atom: what a batch of one takes beyond the head, in units of 256 bytes
    Carve one = {nullptr, 0};
    const int64_t head = sp_layout(one, p, in, 1).head;
    p.atom_bytes = (one.used - head + 255) / 256 * 256;
    const int64_t cap = in.workspace_bytes > 0 ? in.workspace_bytes : k.workspace;
    int64_t b = cap / p.atom_bytes;
    if (b < 1) { p.err = "the workspace cap is below one atom's transform"; return p; }
    if (b > SP_MAX_BATCH) b = SP_MAX_BATCH;
    if (in.n_sel > 0 && b > in.n_sel) b = in.n_sel;
    p.atoms_per_batch = b;
    p.n_batches = in.n_sel > 0 ? (in.n_sel + b - 1) / b : 0;
    p.workspace = b * p.atom_bytes;
    return p;
}
