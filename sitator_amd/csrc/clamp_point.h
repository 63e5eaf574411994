// The arithmetic of ONE clamped point of GenerateClampedTrajectory (clamp.hip), in a form the host compiler takes too
// (tests/test_clamp_point.py runs it with g++ under ASan / UBSan on the reference's own inputs).  Every function follows
// the operation order of the reference, sums left to right, and must be compiled without contraction (-ffp-contract=off):
// its results are compared bit for bit.
//
// The cell type P is anything with the members of Pbc (sit_internal.h): cm = cell.T and ci = inverse(cm), row-major.
// The reference's _cell[j, d] (row j of the cell, PBCCalculator.pyx:287-295) is cm[3 d + j].
#pragma once

#include <math.h>

#ifdef __HIPCC__
#define CP_HD __host__ __device__
#else
#define CP_HD
#endif

// util/PBCCalculator.pyx:240-259 (to_cell_coords) for one point: b = ci . p
template <class P> CP_HD inline void cp_to_cell(const P &c, const double p[3], double b[3])
{
    b[0] = (c.ci[0] * p[0] + c.ci[1] * p[1] + c.ci[2] * p[2]);
    b[1] = (c.ci[3] * p[0] + c.ci[4] * p[1] + c.ci[5] * p[2]);
    b[2] = (c.ci[6] * p[0] + c.ci[7] * p[1] + c.ci[8] * p[2]);
}

// util/PBCCalculator.pyx:319-338 (to_real_coords) for one point: p = cm . b
template <class P> CP_HD inline void cp_to_real(const P &c, const double b[3], double p[3])
{
    p[0] = (c.cm[0] * b[0] + c.cm[1] * b[1] + c.cm[2] * b[2]);
    p[1] = (c.cm[3] * b[0] + c.cm[4] * b[1] + c.cm[5] * b[2]);
    p[2] = (c.cm[6] * b[0] + c.cm[7] * b[1] + c.cm[8] * b[2]);
}

// util/PBCCalculator.pyx:174-193 (wrap_point) / :341-366 (wrap_points) for one point.  fl = floor of the crystal
// coordinates: to_cell_coords of the same point (GenerateClampedTrajectory.pyx:119) evaluates the same expression, so the
// floor the reference takes at :121 is this one.
template <class P> CP_HD inline void cp_wrap(const P &c, const double p[3], double w[3], double fl[3])
{
    double b[3];
    cp_to_cell(c, p, b);
    for (int d = 0; d < 3; d++) { fl[d] = floor(b[d]); b[d] -= fl[d]; }
    cp_to_real(c, b, w);
}

// The 27 image vectors of util/PBCCalculator.pyx:287-295 in the order of the loops (i outermost, k innermost):
// img[9 i + 3 j + k][d] = (i - 1) cell[0, d] + (j - 1) cell[1, d] + (k - 1) cell[2, d]
struct Images27 { double img[27][3]; };                             // the table as a kernel argument, passed by value

template <class P> CP_HD inline void cp_images(const P &c, double img[27][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++)
                for (int d = 0; d < 3; d++)
                    img[9 * i + 3 * j + k][d] = (double)(i - 1) * c.cm[3 * d] + (double)(j - 1) * c.cm[3 * d + 1] + (double)(k - 1) * c.cm[3 * d + 2];
}

// util/PBCCalculator.pyx:262-304 (min_image), the decision only: which of the 27 images of `pt` is nearest to `ref`, the
// first minimum of the loop (strict <).  The reference compares square roots.  The root is monotonic, so an image whose
// squared distance is not below the incumbent's cannot win; the others are compared by their roots as the reference
// compares them - a few roots per point instead of 27.  Returns 9 i + 3 j + k.
CP_HD inline int cp_min_image(const double img[27][3], const double ref[3], const double pt[3])
{
    int best = 0;
    double best2 = INFINITY, bestd = INFINITY;
    for (int m = 0; m < 27; m++) {
        double b0 = pt[0] + img[m][0], b1 = pt[1] + img[m][1], b2 = pt[2] + img[m][2];
        b0 -= ref[0]; b1 -= ref[1]; b2 -= ref[2];
        b0 *= b0; b1 *= b1; b2 *= b2;
        const double d2 = b0 + b1 + b2;
        if (d2 < best2) {
            const double cur = sqrt(d2);
            if (cur < bestd) { bestd = cur; best2 = d2; best = m; }
        }
    }
    return best;
}

// What a site contributes to every point clamped to it: the centre as given (wrap mode copies it), the centre wrapped
// into the cell (the search's `pt`, GenerateClampedTrajectory.pyx:112-113) and the crystal coordinates of the centre as
// given, NOT wrapped (:103-104, :122).
struct ClampSite {
    double center[3], wrapped[3], crystal[3];
};

template <class P> CP_HD inline ClampSite cp_site(const P &c, const double center[3])
{
    ClampSite s;
    double fl[3];
    for (int d = 0; d < 3; d++) s.center[d] = center[d];
    cp_wrap(c, center, s.wrapped, fl);
    cp_to_cell(c, center, s.crystal);
    return s;
}

// GenerateClampedTrajectory.pyx:107-126 for one ion at one frame, wrap = False: the periodic image of the site's centre
// nearest the ion's real position `p`.
template <class P> CP_HD inline void cp_clamp_point(const P &c, const double img[27][3], const ClampSite &s, const double p[3], double out[3])
{
    double w[3], fl[3], b[3];
    cp_wrap(c, p, w, fl);                                            // :114
    const int m = cp_min_image(img, w, s.wrapped);                   // :115
    const int mic[3] = {m / 9 - 1, m / 3 % 3 - 1, m % 3 - 1};        // :116-117
    for (int d = 0; d < 3; d++) b[d] = s.crystal[d] + (double)((int)fl[d] + mic[d]);   // :120-124
    cp_to_real(c, b, out);                                           // :125
}
