/* The van Hove correlation function of libsitator_hip.so: a second header beside sitator_hip.h, whose symbols, structs and
 * SIT_ABI_VERSION it leaves as they are.  Definitions: DESIGN.md section 21.                                          */
#ifndef SITATOR_HIP_VANHOVE_H
#define SITATOR_HIP_VANHOVE_H

#include "sitator_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Histograms of pair distances against the lag, as integer counts.  positions: a host [F, A, 3] float64 array, or NULL for
 * the frames resident after sit_set_frames / sit_upload_fill_fit (F and A must then be theirs).  atoms_a [n_a], atoms_b
 * [n_b]: columns of a frame; same != 0: the two lists are one selection (n_b == n_a) and the pairs of equal position in
 * them are left out of the distinct part.  lags [n_lags], each in [0, F - 1]; the origins of lag tau are t = 0, s, 2 s, ..
 * while t + tau <= F - 1, s = origin_stride >= 1: (F - 1 - tau) / s + 1 of them.  n_bins (at most 2048) bins of equal width
 * on [0, r_max) are decided on SQUARED distances against e2[k] = (k (r_max / n_bins))^2, e2[n_bins] = r_max^2: bin k holds
 * e2[k] <= r2 < e2[k + 1]; everything else, a distance that is not finite included, is counted in the overflow entry
 * n_bins.  self_counts, distinct_counts: uint64 [n_lags, n_bins + 1]; either may be NULL (that part is not computed), not
 * both.
 *   distinct: |x_b(t + tau) - x_a(t)| over the pairs, by the minimum image: s = x . ci per atom and frame ((ci[a][0] x +
 *   ci[a][1] y) + ci[a][2] z, ci the inverse the context was created with), ds = s_b - s_a, ds -= nearbyint(ds),
 *   d = (ds_0 c_0 + ds_1 c_1) + ds_2 c_2, r2 = (d_x^2 + d_y^2) + d_z^2.  This is the true minimum image for any cell shape
 *   while r_max <= hmin / 2 (hmin: the smallest perpendicular height): the call needs 0 < r_max <= hmin / 2 (1 - 2^-30).
 *   A row sums to origins x (n_a n_b, less n_a with same).
 *   self: |y_a(t + tau) - y_a(t)| of the atoms of list a, y the unwrapped series of sit_msd (unwrap != 0; *max_residual
 *   as there) or the positions as they are; no image, a displacement beyond r_max is overflow.  A row sums to origins x n_a.
 * workspace_bytes: cap on the device buffers of the fractional coordinates (frames are taken in windows that fit) and of
 * the series (atoms are taken in batches that fit); 0: SITATOR_SPECTRUM_WORKSPACE_MB, default 1024, as sit_msd.  The counts
 * are added with integer atomics: the same bytes on every call, whatever the windows.  Reads only: frames, rows, labels and
 * their validity stay as they are.  SIT_ERR_INVALID: F < 1 or > 2^29, a lag outside [0, F - 1], origin_stride < 1, n_bins
 * outside [1, 2048], an empty list or one of more than 2^20 atoms, an atom outside [0, A), same with lists of two lengths,
 * an F or A other than the resident frames', r_max outside (0, hmin / 2 (1 - 2^-30)], a degenerate cell, both outputs NULL,
 * a cap below one frame's fractional coordinates or one atom's series.                                                */
int sit_vanhove(sit_ctx *ctx, const double *positions, int64_t F, int64_t A, const int64_t *atoms_a, int64_t n_a,
                const int64_t *atoms_b, int64_t n_b, int same, const int64_t *lags, int64_t n_lags, int64_t origin_stride,
                double r_max, int64_t n_bins, int unwrap, int64_t workspace_bytes, uint64_t *self_counts,
                uint64_t *distinct_counts, double *max_residual);
/* The plan of sit_vanhove, no context needed: out12 = {threads per workgroup, the largest n_bins, the largest list, origins
 * and atoms of b of a distinct workgroup, its pairs (below 2^31), tiles of b, frames per window, atoms per batch of the self
 * part, LDS bytes per workgroup, bytes of the work area, origins of a self workgroup}.  self_part / distinct_part /
 * unwrap: as the call's.  SIT_ERR_INVALID: whatever sit_vanhove refuses of these arguments.                           */
int sit_vanhove_plan(int64_t F, int64_t n_a, int64_t n_b, int64_t n_lags, int64_t n_bins, int64_t origin_stride,
                     int self_part, int distinct_part, int unwrap, int64_t workspace_bytes, int64_t *out12);

#ifdef __cplusplus
}
#endif

#endif
