/* The ionic density of libsitator_hip.so: a fourth header beside sitator_hip.h, sitator_hip_vanhove.h and
 * sitator_hip_scattering.h, whose symbols, structs and SIT_ABI_VERSION it leaves as they are.  Definitions: DESIGN.md section 23. */
#ifndef SITATOR_HIP_DENSITY_H
#define SITATOR_HIP_DENSITY_H

#include "sitator_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Counts of chosen atoms per voxel of a periodic grid over every frame_stride-th frame, and a smoothing of them.
 * positions: a host [F, A, 3] float64 array, or NULL for the frames resident after sit_set_frames / sit_upload_fill_fit (F and A
 * must then be theirs).  atoms [n_sel]: columns of a frame.  grid3 = (n0, n1, n2), each in [1, 1024]; V = n0 n1 n2.
 *   voxel: s_a = (ci[a][0] x + ci[a][1] y) + ci[a][2] z, ci the inverse the context was created with; f_a = s_a - floor(s_a);
 *   i_a = (int64)(f_a n_a), n_a - 1 where that gives n_a or more (f_a == 1, or a product that rounds up: the point lies just
 *   below the upper face); v = (i0 n1 + i1) n2 + i2.  A point with an s_a that is not finite lands in no voxel.
 *   classes: site_class NULL - one plane (K = 0, n_classes = 1), frames alone are read, no deferred pass is collected.
 *   site_class [K], each in [0, n_classes - 2]: the selection must be the M label columns in order (F the frames of the resident
 *   labels, which must be valid) - with the resident frames atoms is compared with their mobile atoms, with a host array only
 *   n_sel == M can be checked and column i of the labels is taken to belong to atoms[i]; an entry with label l >= 0 goes to
 *   plane site_class[l], one with l == -1 to plane n_classes - 1.  A label >= K: SIT_ERR_INVALID with the message of an index out of bounds; below -1: SIT_ERR_INVALID.
 *   counts [n_classes, V] uint64.  info2 = {frames taken, entries in no voxel}: sum(counts) + info2[1] == info2[0] n_sel.
 *   taps [n_taps, 3] integer offsets with |d_a| <= (n_a - 1) / 2, weights [n_taps] finite, smoothed [n_classes, V] float64:
 *   smoothed[p][v] = sum over the taps k in list order, from +0, of w_k * (double) counts[p][(i + d_k) mod n], every product and
 *   sum one rounded float64 operation.  n_taps == 0: no smoothing, smoothed is not touched.
 * form: 1 - one 64-bit atomic add in memory per entry; 2 - a workgroup aggregates its run of frames in an LDS table first; 0 -
 * the plan decides.  Integer atomics only: the same bytes in every form, on every call, whatever workspace_bytes is.
 * workspace_bytes: cap on the device buffer a host array is uploaded through, in windows of whole runs of frames; 0:
 * SITATOR_SPECTRUM_WORKSPACE_MB, default 1024, as sit_msd.  Reads only: frames, rows, labels and their validity stay.
 * SIT_ERR_INVALID: an n_a outside [1, 1024], n_classes outside [1, 16], n_classes V > 2^27, F outside [1, 2^29], frame_stride
 * < 1, n_sel outside [1, 2^20], an atom outside [0, A), an F or A other than the resident frames', a degenerate cell, a
 * site_class entry out of range, n_taps outside [0, 2^15], a tap beyond (n_a - 1) / 2, a weight that is not finite, a cap below
 * one run of frames, a form outside {0, 1, 2}, classes without site_class.                                                    */
int sit_density(sit_ctx *ctx, const double *positions, int64_t F, int64_t A, const int64_t *atoms, int64_t n_sel,
                int64_t frame_stride, const int64_t *grid3, const int32_t *site_class, int64_t K, int64_t n_classes,
                const int64_t *taps, const double *weights, int64_t n_taps, int form, int64_t workspace_bytes,
                uint64_t *counts, double *smoothed, int64_t *info2);
/* The peaks of a host grid of V doubles: voxel v is one when grid[v] >= threshold (a NaN never passes) and every one of its 26
 * periodic neighbours u != v has grid[u] < grid[v], or grid[u] == grid[v] and u > v.  voxels [cap] receives the first cap of
 * them in ascending index, *n_out their number: where it exceeds cap the caller asks again with room for all.            */
int sit_density_peaks(sit_ctx *ctx, const double *grid, const int64_t *grid3, double threshold, int64_t cap, int64_t *voxels,
                      int64_t *n_out);
/* The plan of sit_density, no context needed: out20 = {threads per workgroup, slots of the LDS table, probe limit, LDS bytes of
 * the count kernel, taken frames of a run, runs, the form 0 resolves to (or the form given), the smoothing tile (3), the tile
 * with its halo (3), LDS bytes of the haloed tile (0: the taps read memory), taken frames per upload window, windows, bytes of
 * the work area, frames taken, V, n_classes V}.  halo3: the largest |d_a| of the taps.  host != 0: the positions are a host
 * array.  SIT_ERR_INVALID: whatever sit_density refuses of these arguments.                                                */
int sit_density_plan(int64_t F, int64_t A, int64_t n_sel, int64_t frame_stride, const int64_t *grid3, int64_t K,
                     int64_t n_classes, int64_t n_taps, const int64_t *halo3, int form, int host, int64_t workspace_bytes,
                     int64_t *out20);

#ifdef __cplusplus
}
#endif

#endif
