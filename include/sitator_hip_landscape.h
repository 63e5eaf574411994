/* The energy landscape of a probe ion of libsitator_hip.so: a sixth header beside sitator_hip.h, sitator_hip_vanhove.h,
 * sitator_hip_scattering.h, sitator_hip_density.h and sitator_hip_percolation.h, whose symbols, structs and version it leaves as
 * they are.  Definitions: DESIGN.md section 25.
 *
 * Voxel (i0, i1, i2) of the grid (n0, n1, n2) has the flat index v = (i0 n1 + i1) n2 + i2 and the centre
 *     f_a = ((double)i_a + 0.5) / (double)n_a,    x_k = (f0 cell[0][k] + f1 cell[1][k]) + f2 cell[2][k].
 * The term of a static atom s and an integer triple m: b = x - s, T(m)[k] = (m0 cell[0][k] + m1 cell[1][k]) + m2 cell[2][k],
 * d = b - T, dd = (d0 d0 + d1 d1) + d2 d2, counted where dd <= rc rc, value (eps4 s6)(s6 - 1) - e0 with s6 = (sigma sigma / dd)^3
 * as (q q) q, eps4 = 4 eps and e0 the same at dd = rc rc: dd = 0 gives +inf, never NaN.  E(v) is the flat sequential float64 sum,
 * from 0.0, of the counted terms in ascending (s, m0, m1, m2).                                                                  */
#ifndef SITATOR_HIP_LANDSCAPE_H
#define SITATOR_HIP_LANDSCAPE_H

#include "sitator_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* energies [V]: E(v) at every voxel centre of the grid over the context's cell, among the S atoms static_pos [S][3] with the
 * parameters eps [S], sigma [S] and all their periodic images - any cell shape, cells shorter than rc.  grid3 = (n0, n1, n2), each in
 * [1, 1024], V = n0 n1 n2 <= 2^27.  The energies stay on the device until one copy back.
 *   form: 1 - direct, a thread per voxel walks every atom's translations; 2 - tiled, a workgroup lists the (s, m) that can lie
 *   within rc of its tile of voxels and every thread runs the list; 0 - the plan decides.  The same bytes in every form and on every
 *   call.
 *   info4 = {form taken, tiles, list chunks of the longest tile (0 in the direct form), candidate terms: the entries of the lists of
 *   all tiles, in the direct form the triples the threads of all voxels walked}.
 * SIT_ERR_INVALID: whatever sit_barrier_energies refuses of the same arguments (a missing array, S < 1 or S >= 2^31, rc not positive,
 * a degenerate cell, rc beyond 255 perpendicular heights of the cell, an epsilon or sigma that is not positive and finite, an atom
 * that is not finite or more than 2^20 cells from the origin), an n_a outside [1, 1024], V > 2^27, a form outside {0, 1, 2}.
 * Reads nothing of the context but its cell.                                                                                */
int sit_landscape_energies(sit_ctx *ctx, const double *static_pos, const double *eps, const double *sigma, int64_t S, double rc,
                           const int64_t *grid3, int form, double *energies, int64_t *info4);
/* The plan, no context needed; cell [3][3], rows are the cell vectors.  out16 = {the tile (3), threads per workgroup, LDS bytes of the
 * form taken, records of a list chunk, tiles, the form 0 resolves to (or the form given), |t_a| of the direct form's translations (3),
 * |t_a| of the list of a full tile (3), V, static atoms of the direct form's LDS tile}.
 * SIT_ERR_INVALID: whatever sit_landscape_energies refuses of these arguments.                                              */
int sit_landscape_plan(const double *cell, double rc, const int64_t *grid3, int form, int64_t *out16);

#ifdef __cplusplus
}
#endif

#endif
