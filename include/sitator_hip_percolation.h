/* The percolation of a density of libsitator_hip.so: a fifth header beside sitator_hip.h, sitator_hip_vanhove.h,
 * sitator_hip_scattering.h and sitator_hip_density.h, whose symbols, structs and version it leaves as they are.  Definitions:
 * DESIGN.md section 24. */
#ifndef SITATOR_HIP_PERCOLATION_H
#define SITATOR_HIP_PERCOLATION_H

#include "sitator_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The connected components of {v : grid[v] >= level} on a periodic grid.  grid: a host array of V = n0 n1 n2 doubles, v = (i0 n1
 * + i1) n2 + i2; grid3 = (n0, n1, n2), each in [1, 1024], V <= 2^27.  A NaN voxel is never in the set.
 *   connectivity 6, 18 or 26: the offsets d in {-1, 0, 1}^3 with 1, at most 2, at most 3 non-zero entries.  The neighbour of i
 *   under d is (i + d) mod n, the edge carries the shift s_a = floor((i_a + d_a) / n_a); an axis of one voxel joins a voxel to
 *   itself with shift +-1, an axis of two voxels joins its two voxels twice, once with shift 0 and once with +-1.
 *   labels [V] int32, or NULL: the lowest flat index of the voxel's component, -1 outside the set.
 *   records [cap][12] int64: (root, size, rank, basis[3][3]) of the first cap components in ascending root, *n_out their number:
 *   where it exceeds cap the caller asks again with room for all.  rank and basis: the rank and the row Hermite normal form
 *   (upper triangular, positive pivots, entries above a pivot in [0, pivot), zero rows last) of the lattice the shift sums of
 *   the component's closed walks generate; basis x cell are the directions the component is unbounded in.
 *   form: 1 - labelling rounds over every edge; 2 - a workgroup brings a tile to its fixed point in LDS first and the rounds
 *   look at the edges between tiles; 0 - the plan decides.  The same bytes in every form and on every call.
 *   info4 = {labelling rounds, seam records, form taken, distinct seam records}.
 * SIT_ERR_INVALID: an n_a outside [1, 1024], V > 2^27, a connectivity other than 6, 18, 26, a NaN level, a negative cap, a form
 * outside {0, 1, 2}.                                                                                                          */
int sit_percolation_components(sit_ctx *ctx, const double *grid, const int64_t *grid3, double level, int connectivity, int form,
                               int32_t *labels, int64_t cap, int64_t *records, int64_t *n_out, int64_t *info4);
/* levels3[d - 1], d = 1, 2, 3: the largest positive value of the grid at which the set has a component of rank >= d, as the
 * bytes of that voxel's value; 0.0 where not even {grid > 0} has one.  ranks3[d - 1]: the largest rank of a component of the set
 * at that level (0 beside a level of 0.0).  The grid is uploaded once; the search bisects the bit patterns of the positive doubles
 * between the smallest and the largest positive value, the three searches share their probes.
 *   info4 = {labelling passes, rounds of the last pass, seam records of the last pass, form taken}.                           */
int sit_percolation_levels(sit_ctx *ctx, const double *grid, const int64_t *grid3, int connectivity, int form, double *levels3,
                           int32_t *ranks3, int64_t *info4);
/* The plan, no context needed: out12 = {threads per workgroup, the tile (3), LDS bytes of the tile kernel, tiles, the form 0
 * resolves to (or the form given), seam records of the full grid (no set has more), bytes of the work area of
 * sit_percolation_levels, V, workgroups of a kernel with a thread per voxel, int64 words of a component record}.
 * SIT_ERR_INVALID: whatever the two calls refuse of these arguments.                                                       */
int sit_percolation_plan(const int64_t *grid3, int connectivity, int form, int64_t *out12);

#ifdef __cplusplus
}
#endif

#endif
