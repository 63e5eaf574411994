/* The intermediate scattering function of libsitator_hip.so: a third header beside sitator_hip.h and sitator_hip_vanhove.h,
 * whose symbols, structs and SIT_ABI_VERSION it leaves as they are.  Definitions: DESIGN.md section 22.                */
#ifndef SITATOR_HIP_SCATTERING_H
#define SITATOR_HIP_SCATTERING_H

#include "sitator_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Raw complex sums of the self and the coherent intermediate scattering function over q vectors commensurate with the cell.
 * positions: a host [F, A, 3] float64 array, or NULL for the frames resident after sit_set_frames / sit_upload_fill_fit (F and
 * A must then be theirs).  atoms_a [n_a], atoms_b [n_b]: columns of a frame; same != 0: the two lists are one selection
 * (n_b == n_a) and its density modes are computed once.  q_int [n_q, 3]: integer triples (h, k, l), each index within +-32,
 * (0, 0, 0) allowed, 1 <= n_q <= 2^16: q = 2 pi (h ci[0] + k ci[1] + l ci[2]), ci the inverse the context was created with.
 * lags [n_lags], each in [0, F - 1]; the origins of lag tau are t = 0, s, 2 s, .. while t + tau <= F - 1, s = origin_stride.
 *   phase: s = x . ci per atom and frame ((ci[a][0] x + ci[a][1] y) + ci[a][2] z), f = s - nearbyint(s); E_a = (cos, sin) of
 *   2 pi f_a by a polynomial of the library's own; the term of an atom is (E_0^h E_1^k) E_2^l by repeated complex products.
 *   coherent_sums [n_lags, n_q, 2]: sum over the origins of rho_b(t + tau) conj(rho_a(t)), rho the sum of the terms of a list.
 *   self_sums [n_lags, n_q, 2]: sum over the origins and the atoms of list a of the term of f(t + tau) - f(t), reduced again;
 *   at lag 0 exactly (origins x n_a, 0).
 * Either output may be NULL (that part is not computed), not both.  No floating-point atomic is used and the order of every
 * sum is fixed by F, the lag, the stride and the lists alone: the same bytes on every call, whatever workspace_bytes is.
 * workspace_bytes: cap on the device buffers of the fractional coordinates (frames are taken in windows that fit), the
 * density modes (q vectors are taken in batches that fit) and the block sums (lags are taken in runs that fit); 0:
 * SITATOR_SPECTRUM_WORKSPACE_MB, default 1024, as sit_msd.  Reads only: frames, rows, labels and their validity stay as they
 * are.  SIT_ERR_INVALID: F < 1 or > 2^29, a lag outside [0, F - 1], origin_stride < 1, n_q outside [1, 2^16], an index beyond
 * 32, an empty list or one of more than 2^20 atoms, an atom outside [0, A), same with lists of two lengths, an F or A other
 * than the resident frames', a degenerate cell, both outputs NULL, a cap below one q vector's series and one frame's
 * fractional coordinates.                                                                                              */
int sit_scattering(sit_ctx *ctx, const double *positions, int64_t F, int64_t A, const int64_t *atoms_a, int64_t n_a,
                   const int64_t *atoms_b, int64_t n_b, int same, const int64_t *q_int, int64_t n_q, const int64_t *lags,
                   int64_t n_lags, int64_t origin_stride, int64_t workspace_bytes, double *self_sums, double *coherent_sums);
/* The plan of sit_scattering, no context needed: out12 = {threads per workgroup, the largest index, origins of a block, (frame,
 * atom) entries of a tile of power tables, LDS bytes per workgroup, blocks of origins at lag 0, q vectors per batch, batches,
 * frames per window, lags per launch, bytes of the work area, lags of a coherent workgroup}.  h_max [3]: the largest |index|
 * of every axis of the q list.  SIT_ERR_INVALID: whatever sit_scattering refuses of these arguments.                  */
int sit_scattering_plan(int64_t F, int64_t n_a, int64_t n_b, int same, int64_t n_q, const int64_t *h_max, int64_t n_lags,
                        int64_t origin_stride, int self_part, int coherent_part, int64_t workspace_bytes, int64_t *out12);

#ifdef __cplusplus
}
#endif

#endif
