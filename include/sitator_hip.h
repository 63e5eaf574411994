/*
 * sitator_hip.h -- C-ABI of libsitator_hip.so: the MI355X (gfx950) landmark-analysis
 * hot path of Linux-cpp-lisp/sitator, hand-written HIP behind plain pointers and sizes.
 *
 * This is the boundary a reference maintainer binds with ctypes.
 * Each entry point cites the reference interface it replaces; paths are relative to
 * the reference's `sitator/` package.
 *
 * Conventions
 *   - every function returns an int status (SIT_OK == 0); nothing throws or aborts;
 *   - domain errors (the reference's exceptions) are reported through `sit_error`:
 *     the first offender in the reference's (frame, index) iteration order;
 *   - the caller owns every host buffer; the library owns device memory inside the
 *     opaque `sit_ctx` (one context = one GPU = one host thread at a time);
 *   - all reals are float64 and all indices int64 at the boundary, exactly as the
 *     reference (`ctypedef double precision`, landmark/helpers.pyx:10; np.int);
 *   - "rows" are landmark vectors: row i*M + j is mobile ion j in frame i
 *     (landmark/helpers.pyx:212).  They live on the device in a fixed-width sparse
 *     layout and are never materialised densely unless asked for.
 */
#ifndef SITATOR_HIP_H
#define SITATOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sit_ctx sit_ctx;

enum sit_status {
    SIT_OK = 0,
    SIT_ERR_INVALID = 1,            /* bad argument / call order (-> ValueError)            */
    SIT_ERR_HIP = 2,                /* HIP runtime failure, see sit_last_message()          */
    SIT_ERR_STATIC_THRESHOLD = 3,   /* StaticLatticeError, landmark/helpers.pyx:76-80       */
    SIT_ERR_STATIC_UNASSIGNED = 4,  /* StaticLatticeError, landmark/helpers.pyx:87-92       */
    SIT_ERR_ZERO_LANDMARK = 5,      /* ZeroLandmarkError,  landmark/helpers.pyx:116-118     */
    SIT_ERR_MULTIPLE_OCCUPANCY = 6, /* MultipleOccupancyError, SiteTrajectory.py:219-226    */
    SIT_ERR_NOT_CONVERGED = 7,      /* ValueError, util/DotProdClassifier.pyx:312-313       */
    SIT_ERR_CAPACITY = 8,           /* an internal capacity was exceeded (message says which)*/
    SIT_RETRY = 9,                  /* a deferred sit_fill must be repeated (sit_fill_result)  */
    SIT_ERR_UNASSIGNED = 10         /* RuntimeError, misc/GenerateClampedTrajectory.pyx:73-74 */
};

/* kind = one of sit_status; frame / index / aux as the matching reference exception:
 *   STATIC_THRESHOLD  : frame, index = lattice index            (lattice_atoms=[index])
 *   STATIC_UNASSIGNED : frame (the unseen atoms: sit_static_seen)
 *   ZERO_LANDMARK     : frame, index = mobile index
 *   MULTIPLE_OCCUPANCY: frame, index = site                                            */
typedef struct sit_error {
    int32_t kind;
    int64_t frame;
    int64_t index;
    int64_t aux;
} sit_error;

/* ---- context ------------------------------------------------------------------- */

int sit_device_count(int *count);

/* Replaces PBCCalculator.__init__ (util/PBCCalculator.pyx:22-35).
 * cell[9]: rows are the cell vectors (ASE convention); cell_inv[9]: inverse of cell.T,
 * computed by the caller exactly as the reference does (numpy), row-major.            */
int sit_create(const double *cell, const double *cell_inv, int device, sit_ctx **out);
void sit_destroy(sit_ctx *ctx);
const char *sit_last_message(sit_ctx *ctx);
/* Layout of this boundary as the LIBRARY was built: out[0] = SIT_ABI_VERSION, out[1] = sizeof(sit_error),
 * out[2] = sizeof(sit_fill_params), out[3] = offsetof(sit_fill_params, predict_threshold), out[4] = offsetof(sit_error,
 * frame), out[5] = bytes of a communicator id (sit_comm_unique_id).  Writes min(n, 6) words and returns 6.  A binding
 * checks its own struct declarations against these once, at import (tests/test_abi.py does it for the ctypes stubs of
 * INTEGRATION.md and sitator_amd/_lib.py).  No context, no GPU needed.                                        */
#define SIT_ABI_VERSION 14
int sit_abi(int32_t *out, int n);
/* Device buffers of 1 MB and more (the trajectory, the landmark rows, labels, the fit's arena) are kept by the process
 * when a context lets go of them, up to as much as its contexts have held at once, and handed to the next context that asks for a similar size: a process
 * that analyses one trajectory after another (the reference allocates its landmark matrix anew per run,
 * landmark/LandmarkAnalysis.py:211-218) does not pay the driver's free-then-allocate stall per run.
 * SITATOR_POOL_MIN_MB / SITATOR_POOL_GB change the two limits (SITATOR_POOL_GB=0: no pool); this call returns every
 * idle buffer to the driver. */
void sit_release_cached_memory(void);

/* ---- PBCCalculator parity surface (device kernels) -------------------------------- */

/* PBCCalculator.wrap_points, util/PBCCalculator.pyx:341-366 (in place, host buffer). */
int sit_wrap_points(sit_ctx *ctx, double *pts, int64_t n);
/* PBCCalculator.distances, util/PBCCalculator.pyx:64-103 (shift-and-wrap).           */
int sit_distances(sit_ctx *ctx, const double *pt1, const double *pts2, int64_t n, double *out);
/* PBCCalculator.average, util/PBCCalculator.pyx:106-139; weights may be NULL.        */
int sit_average(sit_ctx *ctx, const double *pts, const double *weights, int64_t n, double *out3);

/* PBCCalculator.min_image, util/PBCCalculator.pyx:262-316, for n pairs: pts[p] (in place, host buffer) becomes the one of its
 * 27 periodic images nearest ref[p] - the first strictly smaller distance in the order of the reference's loops, its sums
 * left to right - and code[p] = 100 i + 10 j + k names it (111: the point stayed).  Both points of a pair are taken to lie
 * in the same cell, as in the reference.                                                */
int sit_min_image(sit_ctx *ctx, const double *ref, double *pts, int64_t n, int32_t *code);

/* LandmarkAnalysis.run Step 1 in one call (landmark/LandmarkAnalysis.py:194-202): out[k,h] =
 * PBCCalculator.distances(centers[k], ref_static[verts[k,h]]), NaN where verts[k,h] == -1.          */
int sit_site_vertex_distances(sit_ctx *ctx, const double *centers, const double *ref_static,
                              const int64_t *verts, int64_t D, int64_t V, int64_t S, double *out);

/* ---- landmark basis and trajectory -------------------------------------------------- */

/* Result of LandmarkAnalysis.run Step 1 (landmark/LandmarkAnalysis.py:194-202):
 * ref_static[S,3] = sn.static_structure.positions, verts[D,V] padded with -1 (statics-only
 * numbering), vert_dists[D,V] padded with NaN.  static_threshold is needed here because the
 * result-preserving landmark pruning tables are built from it (DESIGN.md "pruning").       */
int sit_set_basis(sit_ctx *ctx, const double *ref_static, int64_t S,
                  const int64_t *verts, const double *vert_dists, int64_t D, int64_t V,
                  double cutoff_midpoint, double cutoff_steepness, double static_threshold);

/* frames[F,A,3] float64 C-contiguous, UNWRAPPED (Step 0, LandmarkAnalysis.py:182-189, is fused
 * into the kernels).  static_idx[S] / mobile_idx[M] = np.where(mask)[0].  Copies to HBM.
 * frame0 = global index of the first frame (frame sharding across ranks).               */
int sit_set_frames(sit_ctx *ctx, const double *frames, int64_t F, int64_t A,
                   const int64_t *static_idx, int64_t S, const int64_t *mobile_idx, int64_t M,
                   int64_t frame0);
/* Same, but `frames_dev` is already device memory owned by the caller (borrowed).        */
int sit_set_frames_device(sit_ctx *ctx, const void *frames_dev, int64_t F, int64_t A,
                          const int64_t *static_idx, int64_t S, const int64_t *mobile_idx,
                          int64_t M, int64_t frame0);
/* Device address of the context's frame buffer (for callers that fill it on the device). */
int sit_frames_device_ptr(sit_ctx *ctx, void **ptr);

/* ---- landmark vectors: helpers._fill_landmark_vectors (landmark/helpers.pyx:12-124) --- */

typedef struct sit_fill_params {
    uint32_t struct_size;              /* sizeof(sit_fill_params) as the CALLER declares it.  The library refuses any other
                                          value with SIT_ERR_INVALID instead of reading past a shorter struct (a binding
                                          written against an older header fails loudly: its first word is 0 or 1) */
    int32_t dynamic_lattice_mapping;   /* helpers.pyx:60-64,83 */
    int32_t relaxed_lattice_checks;    /* helpers.pyx:87       */
    int32_t check_for_zeros;           /* helpers.pyx:116-120  */
    int32_t store_rows;                /* keep the sparse rows on the device (fit / mcl); without `assign` they always are */
    int32_t assign;                    /* DotProdClassifier.predict (util/DotProdClassifier.pyx:129-197) in the same pass:
                                          rows of up to four entries are assigned inside the fill kernel and never leave
                                          the chip, wider ones by a second kernel (needs centres: sit_set_centers)        */
    int32_t predict_normed;            /* util/DotProdClassifier.pyx:155-161               */
    int32_t defer;                     /* 1: enqueue only - no host synchronisation; status, n_all_zero and the error of
                                          this pass come from sit_fill_result (or a later sit_fill / sit_synchronize)  */
    double  predict_threshold;         /* util/DotProdClassifier.pyx:184                   */
} sit_fill_params;

/* One streaming pass over the resident frames: wrap, static-lattice check, landmark vector
 * per (frame, ion); with `assign` the site assignment in the same pass, without a host round trip.
 * n_all_zero = self.n_all_zero_lvecs.
 * On a domain error returns its status and fills *err.
 * With `defer` the call returns SIT_OK as soon as the pass is enqueued (*n_all_zero = -1); up to four such passes may be in
 * flight.  The reference raises from inside its frame loop (helpers.pyx:76-92,116-118); a deferred pass raises when
 * its result is collected: sit_fill_result waits for every pass in flight and returns the first failure (with *err) -
 * once; a later sit_fill returns a failure that has landed meanwhile INSTEAD of running - once; and every entry point
 * that READS what a pass produces (rows, labels, counts: sit_predict, sit_get_assignments, sit_get_rows_*, sit_gram*,
 * sit_weighted_row_sums*, sit_best_match*, sit_fit_push_stored_rows, sit_site_*, sit_check_occupancy, sit_cooccupancy, sit_jump_*,
 * sit_assign_last_known, sit_running_mode, sit_count_zero_rows) first waits for the passes in flight and returns their
 * first failure instead of the output of a failed pass (the failure stays until sit_fill_result or sit_fill has
 * reported it).  sit_synchronize waits and decodes but returns the HIP status only.  sit_set_frames /
 * sit_upload_fill_fit wait for and DROP the results of passes over the old frames.
 * SIT_RETRY: a row was wider than the buffers of the pass (measured on the leading frames) - call sit_fill again.  */
int sit_fill(sit_ctx *ctx, const sit_fill_params *p, int64_t *n_all_zero, sit_error *err);
int sit_fill_result(sit_ctx *ctx, int64_t *n_all_zero, sit_error *err);

/* sit_set_frames + sit_fill (rows stored) + sit_fit_reset + sit_fit_push_stored_rows(fit_threshold) in one call, with
 * the upload overlapped: the trajectory goes to the GPU in chunks on a copy stream while the chunks that have arrived
 * are filled and their rows streamed through fit_centers (LandmarkAnalysis.py:211-232 followed by the first pass of
 * util/DotProdClassifier.pyx:199-288; the fit is an ordered stream over the rows, so it can start on the first
 * frames).  Same rows, same clustering state, same first-offender error as the separate calls.  *fitted = 1 when the
 * first pass of the fit has been made (read it with sit_fit_get_state); 0 when the call fell back to upload + fill
 * only (dynamic lattice mapping, a short trajectory, SITATOR_FIT=serial).                                          */
int sit_upload_fill_fit(sit_ctx *ctx, const double *frames, int64_t n_frames, int64_t n_atoms, const int64_t *static_idx,
                        int64_t n_static, const int64_t *mobile_idx, int64_t n_mobile, int64_t frame0,
                        const sit_fill_params *p, double fit_threshold, int64_t *n_all_zero, sit_error *err, int *fitted);

/* Seen-flags of the static atoms of one frame under dynamic mapping (helpers.pyx:87-92). */
int sit_static_seen(sit_ctx *ctx, int64_t local_frame, uint8_t *seen);

int sit_row_width(sit_ctx *ctx, int64_t *width);
/* Dense landmark vectors (the `landmark_vectors` property, LandmarkAnalysis.py:136-141). */
int sit_get_rows_dense(sit_ctx *ctx, int64_t row0, int64_t nrows, double *out);
int sit_get_rows_sparse(sit_ctx *ctx, int64_t row0, int64_t nrows,
                        int32_t *nnz, int32_t *idx, double *val);

/* Install caller-provided dense rows X[N,D] as the context's rows (DotProdClassifier used
 * stand-alone on an ndarray, util/DotProdClassifier.pyx:68,129,199).  Sets D if no basis is set. */
int sit_set_rows_dense(sit_ctx *ctx, const double *rows, int64_t N, int64_t D);

/* ---- DotProdClassifier (util/DotProdClassifier.pyx) --------------------------------- */

/* fit_centers (:199-315) is a strictly ordered stream.  The clustering state (centres,
 * counts) lives on the device; rows are pushed through it in order.                      */
int sit_fit_reset(sit_ctx *ctx);
int sit_fit_set_state(sit_ctx *ctx, const double *centers, const int64_t *counts, int64_t K);
int sit_fit_get_state(sit_ctx *ctx, double *centers, int64_t *counts, int64_t *K);
/* Stream the context's stored rows (all weights 1; first iteration, :233-288).           */
int sit_fit_push_stored_rows(sit_ctx *ctx, double threshold);
/* Stream caller-provided dense rows with weights (iterations >= 2, :290-299).            */
int sit_fit_push_dense_rows(sit_ctx *ctx, const double *rows, const int64_t *weights,
                            int64_t nrows, double threshold);

/* set_cluster_centers (:58-59): centres[K,D] used by predict / fused assign.             */
int sit_set_centers(sit_ctx *ctx, const double *centers, int64_t K, int normed);
/* predict (:129-197) over the stored rows.  labels / confs may be NULL (kept on device);
 * counts[K] = np.bincount(labels[labels >= 0]) (:92).                                     */
int sit_predict(sit_ctx *ctx, double threshold, int64_t *labels, double *confs, int64_t *counts);
/* Number of all-zero rows and the first of them (-1: none).  They get label -1; predict warns, or raises with
 * ignore_zeros=False (:168-172, :192).                                                     */
int sit_count_zero_rows(sit_ctx *ctx, int64_t *n_zero, int64_t *first_row);
/* Labels / confidences of the last predict or fused assign, from the device.              */
int sit_get_assignments(sit_ctx *ctx, int64_t *labels, double *confs, int64_t *counts);

/* ---- mcl plugin support (landmark/cluster/mcl.py) ------------------------------------ */

/* G = X^T X (un-normalised, :55), seen[d] = count_nonzero(X[:, d]) (:54).                */
int sit_gram(sit_ctx *ctx, double *G, int64_t *seen);
/* The same sums as exact integers: entry q = (int128)(hi[q] << 64 | lo[q]) * 2^-80.  They are accumulated with
 * integer atomics (order-independent, so bit-reproducible) and can be added up across ranks exactly; sit_gram
 * rounds them to double.                                                                  */
int sit_gram_limbs(sit_ctx *ctx, uint64_t *hi, uint64_t *lo, int64_t *seen);
/* argmax_n |X[n] . c| with first-max tie-break (:80-83): index, the dot, and |X[n]|.     */
int sit_best_match(sit_ctx *ctx, const double *c, int64_t *row, double *dot, double *norm);
/* The same for G centres with DISJOINT supports in one pass over the rows (the mcl plugin's landmark groups
 * partition the landmarks, :71-87): group_of_dim[d] = centre holding dimension d (-1: none), c[d] = that centre's
 * value at d.  rows/dots/norms: [G].                                                      */
int sit_best_match_groups(sit_ctx *ctx, const int32_t *group_of_dim, const double *c, int64_t G,
                          int64_t *rows, double *dots, double *norms);
/* sums[k] = sum_n w_n X[n], wsum[k] = sum_n w_n, w_n = (label==k) * (conf or 1) (:117-122) */
int sit_weighted_row_sums(sit_ctx *ctx, int weighted, int64_t K, double *sums, double *wsum);
/* As sit_gram_limbs: [K*D + K] exact entries, the sums then the weights.                  */
int sit_weighted_row_sums_limbs(sit_ctx *ctx, int weighted, int64_t K, uint64_t *hi, uint64_t *lo);

/* ---- site centres (landmark/LandmarkAnalysis.py:276-287 + PBCCalculator.average) ------ */

/* Pass 1: per site the anchor = first point of maximum weight (np.argmax, :124-125).      */
int sit_site_anchors(sit_ctx *ctx, int weighted, int64_t K,
                     double *wmax, int64_t *first_row, double *anchor_pts);
/* Pass 2: sums[k] = (sum w, sum w*x, sum w*y, sum w*z) of points shifted by
 * (centroid - anchor[k]) and wrapped (:127-134).                                         */
int sit_site_sums(sit_ctx *ctx, int weighted, int64_t K, const double *anchor_pts, double *sums);

/* ---- SiteTrajectory (SiteTrajectory.py) ---------------------------------------------- */

/* check_multiple_occupancy (:205-232) on the device-resident labels:
 * n_multi = sum_frames #(counts > 1), total = sum_frames sum(counts), nsites = sum_frames
 * #unique sites (avg_mobile_per_site = total / nsites).                                   */
int sit_check_occupancy(sit_ctx *ctx, int64_t K, int64_t max_per_site,
                        int64_t *n_multi, int64_t *total, int64_t *nsites, sit_error *err);

/* np.bincount(traj[traj >= 0], minlength=K) of the device labels: compute_site_occupancies (:187-202) divides it
 * by the number of frames.                                                                */
int sit_site_counts(sit_ctx *ctx, int64_t K, int64_t *counts);

/* co[a*K + b] = 1 iff some frame of the resident labels has one ion on site a and one on site b
 * (a == b: the site is occupied at all); 0 otherwise.  Labels < 0 are ignored; a label >= K fails the
 * way sit_jump_analysis does (SIT_ERR_INVALID, message starting "index ", IndexError in Python).
 * MergeSitesByThreshold.py:64-70 clears exactly these entries.  One pass over the labels plus
 * (label changes) x M byte stores, not M^2 per frame.  K <= 16384 (the matrix is K*K bytes, on the
 * device too: 256 MB at the limit); no frames: all zeros.                                        */
int sit_cooccupancy(sit_ctx *ctx, int64_t K, uint8_t *co);

/* Upload a label array (and optional confidences) as the context's assignments, for a
 * SiteTrajectory that was not produced on this context (SiteTrajectory.__init__, :15-42).
 * Sets F, M (and the row count) if no frames are resident.                                */
int sit_set_assignments(sit_ctx *ctx, const int64_t *labels, const double *confs,
                        int64_t F, int64_t M, int64_t frame0);

/* Jump detection, SiteTrajectory._jumped_generator (:347-373): for every (frame >= 1, ion)
 * from[f*M+j] = the last known site before frame f if the ion jumped at f, else INT64_MIN.
 * last_known_in[M] (NULL = frame 0 of this context is the trajectory start) / last_known_out[M]
 * carry the forward-filled state across frame shards.                                     */
int sit_jump_sources(sit_ctx *ctx, int unknown_as_jump, const int64_t *last_known_in,
                     int64_t *from, int64_t *last_known_out);
/* The same scan reported as compact records {frame, mobile atom, from site, to site} (in no particular order; at most
 * max_records are written, *n_records is the number found - call again with a larger buffer if it is larger).     */
int sit_jump_list(sit_ctx *ctx, int unknown_as_jump, const int64_t *last_known_in, int64_t max_records,
                  int64_t *records, int64_t *n_records, int64_t *last_known_out);

/* ---- the steps either side of the path ------------------------------ */

/* JumpAnalysis.run (dynamics/JumpAnalysis.py:27-135) on the device-resident labels.  Outputs the raw
 * accumulators: n_ij[K,K], time_sum[K,K] / time_n[K,K] (jump_lag = time_sum / time_n, inf where time_n
 * is 0), total_time[K] (total_corrected_residences), n_problems.  last_known / time_at_current in (NULL at
 * the trajectory start) and out carry the per-ion state across frame shards.                            */
int sit_jump_analysis(sit_ctx *ctx, int64_t K, const int64_t *last_known_in,
                      const int64_t *time_at_current_in, double *n_ij, double *time_sum,
                      int64_t *time_n, int64_t *total_time, int64_t *n_problems,
                      int64_t *last_known_out, int64_t *time_at_current_out);

/* SiteTrajectory.assign_to_last_known_site (SiteTrajectory.py:235-304): rewrites the device labels in
 * place (labels_out: optional host copy).  frame_max[F]: per frame the largest unknown-streak length that
 * ended there; stats3 = (sum of streak lengths, number of streaks, positions reassigned).              */
int sit_assign_last_known(sit_ctx *ctx, int64_t frame_threshold, const int64_t *last_known_in,
                          const int64_t *time_unknown_in, int64_t *labels_out, int32_t *frame_max,
                          int64_t *stats3, int64_t *last_known_out, int64_t *time_unknown_out);

/* ReplaceUnassignedPositions (dynamics/ReplaceUnassignedPositions.py:90-117) on the device-resident labels, which are
 * only read.  "Unknown" is label == -1; for an unknown frame `before` is the nearest label != -1 at an earlier frame of
 * the ion, failing that before_in[ion], failing that -1; `after` the same towards later frames.  before_in / after_in
 * ([M], both or neither; NULL = -1) are what frame shards carry in from their neighbours.
 *
 * sit_label_ends: per ion the first and the last label != -1 of this context's frames, INT64_MIN where it has none:
 * all that frame shards exchange.                                                                              */
int sit_label_ends(sit_ctx *ctx, int64_t *first_known, int64_t *last_known);
/* labels_out[F*M]: the labels with every unknown frame replaced by `before` (mode 0) or by `after` (mode 1).       */
int sit_replace_unassigned(sit_ctx *ctx, int mode, const int64_t *before_in, const int64_t *after_in,
                           int64_t *labels_out);
/* Every maximal run of unknown frames as a record {ion, start, end, before, after, pos_offset} of int64, ion-major and
 * by start within an ion (the order the reference calls its replacement function in, :99-112; the same on every call).
 * start / end (exclusive) are global frame numbers inside this context's frames.  pos_offset: the running sum of the
 * lengths of the runs whose before and after are both >= 0 and differ (those the closer-site strategy has to decide),
 * -1 for the other runs; *n_positions is that sum.  *n_records is the number found; when it exceeds max_records
 * nothing is written - call again with a larger buffer.                                                          */
int sit_unknown_runs(sit_ctx *ctx, const int64_t *before_in, const int64_t *after_in, int64_t max_records,
                     int64_t *records, int64_t *n_records, int64_t *n_positions);
/* replace_with_closer (:56-87) for records of the layout above: positions[n_positions][3] holds the real-space position
 * of the run's ion at every frame of every run with pos_offset >= 0, in record order; such a frame becomes `before`
 * when dist(position, centers[before]) < dist(position, centers[after]) (the shift-and-wrap distance of sit_distances)
 * and `after` otherwise.  Runs with before == after >= 0 take that site, runs with a side of -1 stay -1, every other
 * entry of labels_out[F*M] is the resident label.  The records are checked before anything is indexed with them: a site
 * >= K fails like sit_jump_analysis (SIT_ERR_INVALID, message starting "index ", IndexError in Python); an ion outside
 * [0, M), frames outside the context, a site < -1 or positions outside [0, n_positions) fail with SIT_ERR_INVALID.   */
int sit_replace_closer(sit_ctx *ctx, const int64_t *records, int64_t n, const double *centers, int64_t K,
                       const double *positions, int64_t n_positions, int64_t *labels_out);

/* running_windowed_mode (dynamics/SmoothSiteTrajectory.pyx:79-111) of the device labels -> out[F*M]; counts
 * (optional, [K]) = np.bincount of the smoothed labels >= 0: which sites are left occupied
 * (dynamics/RemoveUnoccupiedSites.py:31-38 looks for the others).                                        */
int sit_running_mode(sit_ctx *ctx, int64_t wleft, int64_t wright, int64_t threshold,
                     int replace_no_winner_unknown, int64_t *out, int64_t K, int64_t *counts);

/* recenter_traj_array (util/RecenterTrajectory.pyx:66-100) IN PLACE on a host array [F,A,3]:
 * x -= sum_j (factor_j*mass_j / sum(factor*mass)) x_j per frame, then += add3 (NULL = 0).              */
int sit_recenter(sit_ctx *ctx, double *arr, int64_t F, int64_t A, const double *masses,
                 const double *factors, const double *add3);
/* The same on the frames resident after sit_set_frames, in place on the device (the caller's array stays as it is):
 * the recentring as a pre-pass of the landmark analysis without a PCIe round trip of the trajectory.      */
int sit_recenter_resident(sit_ctx *ctx, const double *masses, const double *factors, const double *add3);

/* AverageVibrationalFrequency (dynamics/AverageVibrationalFrequency.py:30-61): per selected atom the speeds
 * s[t] = |x[t+1] - x[t]| (t < n = F - 1, no periodic wrap), their spectrum X = rfft(s) (n / 2 + 1 bins; an exact-length
 * transform by Bluestein's chirp-z over power-of-two passes in float64) and, over the bins with fmask != 0,
 * band_power = sum |X_k|^2 and avg = sum freqs_k |X_k|^2 / band_power (0 / 0 = NaN where an atom never moves).
 * positions: host [F, n_sel, 3], or NULL for the frames resident after sit_set_frames, of which `atoms` [n_sel] names the
 * columns (F must then be the context's).  freqs / fmask [n / 2 + 1]: numpy's rfftfreq(n) and the band, made by the
 * caller.  workspace_bytes: cap on the device buffers of a batch of atoms (0: SITATOR_SPECTRUM_WORKSPACE_MB, default
 * 1024); atoms are processed in batches that fit, every atom's transform on its own: its results do not depend on the
 * batch or on the other atoms.  spectrum [n_sel, n / 2 + 1, 2] and speeds [n_sel, n] are optional (NULL).  Reads only:
 * frames, rows, labels and their validity stay as they are.  SIT_ERR_INVALID: F < 2, F - 1 > 2^29, an atom outside
 * [0, A), F other than the resident frames', a cap below one atom's transform.                              */
int sit_speed_spectrum(sit_ctx *ctx, const double *positions, int64_t F, const int64_t *atoms, int64_t n_sel,
                       const double *freqs, const uint8_t *fmask, int64_t workspace_bytes, double *avg,
                       double *band_power, double *spectrum, double *speeds);

/* MeanSquaredDisplacement: per selected atom, Cartesian axis and lag tau the mean squared displacement
 * msd(tau) = (1 / (F - tau)) sum_{t < F - tau} (y[t + tau] - y[t])^2 of the series y[t] = x_u[t] - x_u[0].  With
 * unwrap != 0, x_u is the trajectory unwrapped under the context's cell: a step d = x[t] - x[t-1] crosses
 * n_a = nearbyint((d . cell^-1)_a) images (0 where that is not finite), the image counts N[t] = -sum_{s<=t} n[s] are exact
 * int32 sums and x_u[t] = x[t] + N_0 c_0 + N_1 c_1 + N_2 c_2 (x[t] itself, bit for bit, where N[t] = 0); *max_residual is
 * the largest |(d . cell^-1)_a - n_a| over all finite steps, in [0, 0.5]: the unwrapping is the true one while every true
 * step stays below half a cell vector.  With unwrap == 0, x_u = x and *max_residual = 0.
 * positions: host [F, n_sel, 3], or NULL for the frames resident after sit_set_frames, of which `atoms` [n_sel] names the
 * columns (F must then be the context's).
 * lags == NULL: all lags 0 .. max_lag (n_lags is taken as max_lag + 1) by msd = S1 - 2 acf / (F - tau), the autocorrelation
 * through a zero-padded float64 transform of length 2^m >= 2 F - 1 per (atom, axis), S1 from prefix sums of y^2; r4 must be
 * NULL.  lags != NULL: the n_lags lags listed (each in [0, F - 1], duplicates allowed) by the sums themselves, and
 * r4 [n_sel, n_lags] (optional) = (1 / (F - tau)) sum_t (|y[t + tau] - y[t]|^2)^2.  Lag 0 is exactly 0.
 * msd [n_sel, 3, n_lags].  collective != 0: coll [3, n_lags] = the same of Y[t] = sum_i y_i[t] (atoms added in selection
 * order), divided by n_sel.  images [n_sel, F, 3] (optional, int32): N[t].
 * workspace_bytes: cap on the device buffers of a batch of atoms (0: SITATOR_SPECTRUM_WORKSPACE_MB, default 1024); an
 * atom's results do not depend on the batch or on the other atoms.  Reads only: frames, rows, labels and their validity
 * stay as they are.  SIT_ERR_INVALID: F < 2 or > 2^29, a lag or max_lag outside [0, F - 1], r4 without lags, coll without
 * collective or the reverse, an atom outside [0, A), F other than the resident frames', a cap below one atom's buffers, a
 * degenerate cell with unwrap.                                                                             */
int sit_msd(sit_ctx *ctx, const double *positions, int64_t F, const int64_t *atoms, int64_t n_sel, int unwrap,
            int64_t max_lag, const int64_t *lags, int64_t n_lags, int collective, int64_t workspace_bytes, double *msd,
            double *r4, double *coll, int32_t *images, double *max_residual);

/* GenerateClampedTrajectory (misc/GenerateClampedTrajectory.pyx:92-126): out[F, A, 3] (host) holds for every frame and
 * atom, by role[a]: -1 the atom's real position, -2 fixed_pos[a], m >= 0 the centre of the site that column m of the
 * resident labels [F, M] names at that frame - as given with wrap != 0, with wrap == 0 the periodic image of the centre
 * nearest the atom's real position (27-image search between the wrapped position and the wrapped centre, then crystal
 * centre + floor(crystal position) + image, back to real space, in the reference's operation order: bit-equal).
 * positions: host [F, A, 3], or NULL for the frames resident after sit_set_frames / sit_upload_fill_fit (F and A must then
 * be the context's); it is not looked at when no element needs a real position (wrap != 0, no role -1 and
 * pass_through_unassigned == 0).  fixed_pos [A, 3]; centers [K, 3].  Frames are processed in chunks whose device buffers
 * (the output, on the host path the staged positions too) fit workspace_bytes (0: SITATOR_CLAMP_WORKSPACE_MB, default
 * 1024); a frame's result does not depend on the chunking.  A label of -1 on a clamped ion: with pass_through_unassigned
 * the real position is written; without, the call returns SIT_ERR_UNASSIGNED, *first_unassigned (optional; -1 otherwise)
 * is the smallest frame * M + column found and nothing is promised about out.  Every label is looked at before anything
 * is indexed with it: a label >= K fails like sit_jump_analysis (SIT_ERR_INVALID, message starting "index ", IndexError in
 * Python); a label < -1, a role outside [-2, M), two atoms with the same column, an F or A other than the resident
 * labels' / frames', a cap below one frame fail with SIT_ERR_INVALID.  Reads only: frames, rows, labels and their
 * validity stay as they are.                                                                               */
int sit_clamp_trajectory(sit_ctx *ctx, const double *positions, int64_t F, int64_t A, const int32_t *role,
                         const double *fixed_pos, const double *centers, int64_t K, int wrap,
                         int pass_through_unassigned, int64_t workspace_bytes, double *out, int64_t *first_unassigned);

/* ---- per-site point clouds (SiteTrajectory.real_positions_for_site, SiteTrajectory.py:160-184, for all sites at once) ---- */

/* A stable grouping of the assigned entries of the resident labels [F, M] by site.  Entry e = frame * M + column with
 * label s >= 0 belongs to site s; the grouped order is sites ascending and, inside a site, ascending e: the order of
 * real_traj[:, mobile_mask][traj == s].  Entries with label -1 are left out.  Per grouped element the context keeps the
 * position (three doubles copied bit for bit), the confidence and e; offsets[K + 1] comes back (offsets[s + 1] - offsets[s]
 * is what sit_site_counts returns).  positions: host [F, A, 3] of which mobile_idx [M] names the label columns' atoms,
 * staged in chunks of frames that fit workspace_bytes (0: 1 GiB; a cap below one frame is SIT_ERR_INVALID); or NULL for
 * the frames resident after sit_set_frames / sit_upload_fill_fit with the context's own mobile columns (mobile_idx is not
 * looked at).  A counting sort in three passes (histogram per chunk of entries, scan, scatter; csrc/group_plan.h); the rank
 * of an entry among equal labels comes from the entry order, so two ions on one site in one frame keep their order.
 * Every label is looked at before anything is indexed with it: a label >= K fails like sit_jump_analysis (SIT_ERR_INVALID,
 * message starting "index ", IndexError in Python), a label < -1, an F, A or M other than the resident ones with
 * SIT_ERR_INVALID; more than 2^31 entries with SIT_ERR_CAPACITY.  Reads only: labels, rows, frames and their validity stay
 * as they are.  The grouping stays in the context until the next call or sit_destroy and is tied to the labels it was made
 * from: once they are rewritten (sit_predict, sit_fill with assign, sit_set_assignments, sit_assign_last_known, new frames)
 * the sit_grouped_* calls fail with SIT_ERR_INVALID and a message starting "stale".                                   */
int sit_group_by_site(sit_ctx *ctx, const double *positions, int64_t F, int64_t A, const int64_t *mobile_idx, int64_t M,
                      int64_t K, int64_t workspace_bytes, int64_t *offsets);
/* Elements [first, first + n) of the grouping: pts [n, 3], confs [n], entries [n]; each may be NULL.              */
int sit_grouped_fetch(sit_ctx *ctx, int64_t first, int64_t n, double *pts, double *confs, int64_t *entries);
/* NAvgsPerSite (misc/NAvgsPerSite.py:55-62): centers_out[(s * n_avg + i), 3] = PBCCalculator.average (util/PBCCalculator.pyx:
 * 106-139) of the elements of site s at ranks i, i + n_avg, ... - weighted by their confidences, the anchor being the
 * first element of maximal weight, or unweighted, the anchor being the first element.  The shifted and wrapped points are
 * the reference's bit for bit; they are summed per thread in index order and then by a fixed tree of 256, so a bucket's
 * result depends on its own elements only.  Sites with at most n_avg elements are not averaged: NaN.  anchors_out
 * (optional) [K * n_avg]: the grouped index of every bucket's anchor, -1 where not averaged.                       */
int sit_grouped_bucket_averages(sit_ctx *ctx, int64_t n_avg, int weighted, double *centers_out, int64_t *anchors_out);
/* Step i of SiteVolumes.compute_accessable_volumes' recentring (site_descriptors/SiteVolumes.py:58-62) for all sites at
 * once, on a working copy of the grouped positions that step 0 makes: per site offset = centroid - copy[anchor], anchor =
 * (int64)((double)i * ((double)len / (double)n_recenterings)), then copy += offset and wrap_points - cumulative, as the
 * reference works in place.  Steps come in order from 0.  pts_out (optional) [N, 3]: the copy after the step, bit-equal
 * to the reference's array.  A site without elements fails as the reference's pos[0] does (SIT_ERR_INVALID, message
 * starting "index ", IndexError in Python).                                                                          */
int sit_grouped_recenter_step(sit_ctx *ctx, int64_t i, int64_t n_recenterings, double *pts_out);
/* The plan for n_entries entries and K sites, no context needed: out4 = {entries per chunk, chunks, 1 if a chunk's
 * per-site cursors are kept in LDS, the largest K for which they are}.                                              */
int sit_group_plan(int64_t n_entries, int64_t K, int64_t *out4);
/* Of the context's last grouping: [0] grouped elements, [1] K, [2] chunks, [3] LDS form, and device time (ms, HIP events)
 * of the last [4] sit_group_by_site (from its first kernel to its last, the host's part in between included),
 * [5] bucket-average kernel, [6] pair of recentring kernels, [7] hull kernel (sit_grouped_hull_volumes).              */
int sit_group_info(sit_ctx *ctx, double *out, int n);
/* Convex hulls of every site's points in the working copy as the last sit_grouped_recenter_step left it (the hulls
 * SiteVolumes.py:63-69 asks qhull for), one workgroup per site, the copy is only read: volumes[K], status[K],
 * n_facets[K] (triangles found, also where the site did not close) and, optional, vertex_mask[N]: 1 for the grouped
 * elements that are vertices of their site's hull (of equal points the first).  Gift wrapping with a certified
 * orientation test (csrc/hull_predicates.h: double arithmetic with a forward error bound, never a decision from a
 * determinant inside its bound).  status 0: the hull closed (every directed edge met its reverse once, V - E + F = 2)
 * and volumes[s] is its volume - the tetrahedra against the first vertex summed in the order the facets were found, the
 * same bytes in every run; 1: fewer than 4 points; 2: an uncertain test was met (coplanar or nearly coplanar points);
 * 3: more than the facet or open-edge capacity of sit_hull_plan; 4: the hull did not close.  volumes[s] is NaN unless
 * status[s] is 0: the caller takes such a site elsewhere (sit_grouped_work_fetch).  SIT_ERR_INVALID before step 0 of a
 * recentring, and for a stale grouping as the other sit_grouped_* calls.                                              */
int sit_grouped_hull_volumes(sit_ctx *ctx, double *volumes, int32_t *status, int32_t *n_facets, uint8_t *vertex_mask);
/* Elements [first, first + n) of the working copy: pts [n, 3].  SIT_ERR_INVALID before step 0 of a recentring.       */
int sit_grouped_work_fetch(sit_ctx *ctx, int64_t first, int64_t n, double *pts);
/* The plan of sit_grouped_hull_volumes, no context needed: out4 = {facet capacity, open-edge capacity, threads per
 * workgroup, LDS bytes per workgroup} (csrc/hull_plan.h).                                                            */
int sit_hull_plan(int64_t *out4);

/* ---- the site graph under periodic boundaries (network/DiffusionPathwayAnalysis.py) ------------------------------------ */

/* Connected components of the site graph of conn[K, K] (conn[from * K + to] != 0: connected; the reference's thresholded
 * n_ij, :71) with centers[K, 3], for n_images = 27 of the 3 x 3 x 3 supercell graph of _build_mic_connmat (:175-228), for
 * n_images = 1 of the plain K-node graph (true_periodic_pathways = False).  code[K, K] (optional, NULL): per connected
 * pair 100 i + 10 j + k of min_image(centers[from], centers[to]) as sit_min_image gives it, 0 elsewhere.  Node = image * K +
 * site, the images in the order of itertools.product(range(-1, 2), repeat = 3) (home image: 13); an edge with code 111
 * stays inside every image, any other goes from image s to s + (digits - 1) and is dropped where that leaves [-1, 1]
 * (:218-224).  Edges are undirected for the components (weak connection, :76-78).  root[n_images * K]: per node the LOWEST
 * node index of its component - ranking the distinct values gives scipy's component numbers.  The labelling hooks roots
 * with atomic minima and compresses by pointer jumping in rounds of ordinary launches (csrc/pathway_graph.h); its fixed
 * point does not depend on the order of arrival, so the result is the same on every call.  *rounds: rounds taken, the
 * last of which changed nothing (0 without a connected pair).  SIT_ERR_INVALID: a missing array, K < 0, K > 16384 (the mask
 * is K * K bytes and the codes 4 K * K on the device), n_images other than 1 or 27; SIT_ERR_CAPACITY: no fixed point within
 * n_images * K rounds (cannot happen: every round before the last lowers a label).  Reads nothing of the context but its
 * cell: frames, rows, labels and their validity stay as they are.                                          */
int sit_pathway_components(sit_ctx *ctx, int64_t K, const uint8_t *conn, const double *centers, int n_images,
                           int32_t *code, int32_t *root, int64_t *rounds);

/* ---- energy barriers between sites (network/MergeSitesByBarrier.py) ---------------------------------------------------------- */

/* The energies of ONE mobile atom driven along the straight path of every candidate pair, in the frozen lattice static_pos[S, 3]
 * under the context's cell, and the verdict of :116-125 on them.  The potential is a truncated and shifted 12-6 pair term of
 * the mobile atom with every coordinating atom s and all its periodic images (csrc/barrier_plan.h): with d2 the squared
 * distance, s6 = (sigma[s]^2 / d2)^3, phi = 4 eps[s] s6 (s6 - 1) - e0[s] for d2 <= rc^2, e0[s] the same expression at
 * d2 = rc^2; d2 = 0 gives +inf.  Everything else of the total energy the reference's calculator returns (:113) is constant
 * along a path and is left out.  pairs[P, 2] (int32) names sites of centers[K, 3]; per pair (i, j) the point pos[j] is moved to
 * its image nearest pos[i] as sit_min_image does (code[P], optional: its 100 i + 10 j + k), vector = moved - pos[i], and image m
 * of n sits at vector * coeffs[m] + pos[i] (the product rounded before the sum, :110-112; the caller passes
 * np.linspace(0, 1, n)).  energies[P, n] (optional).  verdict[P, 3] (uint8): [0] the first maximum of the pair's energies (np.argmax)
 * is neither its first nor its last image, [1] maximum - first <= threshold, [2] maximum - last <= threshold.  Complete for any
 * cell shape, cells shorter than rc, and atoms or driven points outside the cell; the sum runs in a fixed order (no atomics):
 * the same bytes on every call.  SIT_ERR_INVALID: a missing array, S < 1, n < 3, K > 16384, a pair index outside [0, K), a
 * non-positive (or not finite) eps, sigma or rc, rc beyond 255 perpendicular heights of the cell, a position that is not finite
 * or more than 2^20 cells from the origin, a coefficient outside [-2, 2].  P = 0 is SIT_OK and touches nothing.  Reads nothing
 * of the context but its cell: frames, rows, labels and their validity stay as they are.                                  */
int sit_barrier_energies(sit_ctx *ctx, const double *static_pos, const double *eps, const double *sigma, int64_t S, double rc,
                         const double *centers, int64_t K, const int32_t *pairs, int64_t P, const double *coeffs, int64_t n,
                         double threshold, double *energies, uint8_t *verdict, int32_t *code);
/* The plan of sit_barrier_energies for cell[9] (rows are the cell vectors) and rc, no context needed: out6 = {the translations
 * |t_a| <= out6[a] along the three cell vectors that can hold a term within rc once the difference of two points is brought
 * into the cell (floor(rc / h_a) + 1, h_a the perpendicular height), static atoms per LDS tile, threads per workgroup, LDS
 * bytes per workgroup}.  SIT_ERR_INVALID: a degenerate cell, rc not positive or beyond 255 heights.                        */
int sit_barrier_plan(const double *cell, double rc, int64_t *out6);

/* ---- Voronoi nodes of the static lattice (voronoi.py, which asks the Zeo++ `network` binary) --------------------------------- */

/* The periodic Voronoi nodes of static_pos[S, 3] (any periodic image) under the context's cell, for a tolerance tau in Angstrom
 * (csrc/voronoi_plan.h).  A node is a sphere (c, r) with no atom image closer to c than r - tau and at least four atom images,
 * not coplanar, within [r - tau, r + tau]; its vertices are the static indices of all atom images in that shell, unique and
 * ascending - one degenerate sphere is one node with all of its atoms, and in a cell so small that images of one atom share a
 * sphere a node has fewer than 4 vertices.  Two-call convention: every call sets *n_nodes and *n_indices (the sizes needed),
 * status[S] (0 done, 1 the search radius would have to grow further, 2 an uncertain test was met, 3 a capacity of
 * sit_voronoi_plan was exceeded), nbr_count[S] (atom images within the atom's last search radius) and info8 = {rounds of the
 * search radius, the last radius, the largest neighbour count, records before the merge, kernel milliseconds (HIP events), the
 * first radius, the status of the merge (2: two record centres between 16 tau and 64 tau apart), 0}; when n_nodes <= node_cap
 * and n_indices <= index_cap it also fills centers[n_nodes, 3] (wrapped into the cell), radii[n_nodes], offsets[n_nodes + 1] and
 * indices[n_indices] (CSR of the vertices).  The result of the last call is kept with the context: the fill call after a size
 * call with the same input computes nothing.  Unless every status is 0 and the merge is unambiguous there are no nodes
 * (n_nodes = 0): a partial network is never returned.  Nodes come in the order of their first record (atoms ascending, the
 * enumeration of voronoi_plan.h inside an atom); nothing depends on arrival: the same bytes on every call.  status, nbr_count,
 * info8 and the four result arrays are optional.  SIT_ERR_INVALID: a missing array, S < 1, tau not positive, a degenerate cell, a
 * position that is not finite or more than 2^20 cells from the origin.  Reads nothing of the context but its cell.            */
int sit_voronoi_nodes(sit_ctx *ctx, const double *static_pos, int64_t S, double tau, int64_t node_cap, int64_t index_cap,
                      int64_t *n_nodes, int64_t *n_indices, double *centers, double *radii, int64_t *offsets, int32_t *indices,
                      int32_t *status, int32_t *nbr_count, double *info8);
/* The plan of sit_voronoi_nodes for cell[9] (rows are the cell vectors) and S atoms, no context needed: out8 = {neighbour cap,
 * record cap per atom, atom images per sphere, threads per workgroup, LDS bytes per workgroup, rounds at most, bytes of a
 * record, 1 / VP_SHAPE_MIN}; radius2 (optional) = {the first search radius, the growth factor}.                             */
int sit_voronoi_plan(const double *cell, int64_t S, int64_t *out8, double *radius2);

/* ---- Coordination environments of sites (site_descriptors/SiteCoordinationEnvironment.py, which asks pymatgen's ChemEnv) ------ */

/* For each of centers[K, 3], alone with static_pos[S, 3] and all its periodic images under the context's cell
 * (csrc/coordenv_plan.h): the static images that coordinate the site - the face neighbours of the site's Voronoi cell (certified
 * empty spheres through the site, tolerance tau) with distance / smallest distance <= distance_cutoff and solid angle / largest
 * solid angle >= angle_cutoff - and the continuous shape measure S (0 - 100, Pinsky & Avnir) of their polyhedron, the site at the
 * origin, against every library shape of that coordination number, minimised over all n! vertex assignments.  Two-call
 * convention: every call sets *n_indices, status[K] (0 done, 1 the search radius would have to grow further, 2 an uncertain test
 * was met or an atom lies on the site, 3 a capacity of sit_coordenv_plan was exceeded), flags[K] (bit 0: a ratio within 1e-9
 * relative of its cutoff; the comparison still decided), n[K] (coordinating images), shape[K] (library index of the environment:
 * the smallest S if below max_csm, else -1), csm_best[K] (NaN without a library shape), csm_all[K, 3] (the shapes of that n in
 * library order, NaN padded), confidence[K] (w_best / sum w, w = (1 - S / max_csm)^2 below max_csm) and info8 = {rounds of the
 * search radius, the last radius, the largest neighbour count, the largest n, milliseconds of k_coordenv_cell and of
 * k_coordenv_csm (HIP events), the first radius, 1 if this call computed and 0 if it returned the kept result}; when
 * n_indices <= index_cap it also fills the CSR offsets[K + 1], indices[n_indices] (static index; ordered by distance, static
 * index, image; an index repeats when two images of one atom coordinate), norm_distance and norm_angle.  The result of the last
 * call is kept with the context: the fill call after a size call with the same input computes nothing.  Nothing depends on
 * arrival: the same bytes on every call.  Every output but n_indices is optional.  SIT_ERR_INVALID: a missing array, S < 1,
 * K < 1, tau or max_csm not positive, distance_cutoff < 1, angle_cutoff outside (0, 1], a degenerate cell, a value that is not
 * finite or a position more than 2^20 cells from the origin; SIT_ERR_CAPACITY: 2^24 atoms or sites, or more.  Reads nothing of the
 * context but its cell, device and stream.                                                                                    */
int sit_coordination_environments(sit_ctx *ctx, const double *static_pos, int64_t S, const double *centers, int64_t K, double tau,
                                  double distance_cutoff, double angle_cutoff, double max_csm, int64_t index_cap, int64_t *n_indices,
                                  int32_t *status, int32_t *flags, int32_t *n, int64_t *offsets, int32_t *indices, double *norm_distance,
                                  double *norm_angle, int32_t *shape, double *csm_best, double *csm_all, double *confidence, double *info8);
/* The plan of sit_coordination_environments, no context needed: out8 = {neighbour cap, cell vertices per site, vertices per face,
 * coordinating images per site, the largest n with a shape measure, threads per workgroup, LDS bytes of the cell kernel, shapes
 * in the library}; shape_n[12] (optional) the coordination number of each library shape (S:1, L:2, TL:3, T:4, S:4, T:5, S:5, O:6,
 * T:6, PB:7, C:8, SA:8, in this order); coords[12, 8, 3] (optional) their unit vertices, rows beyond n zero.                   */
int sit_coordenv_plan(int64_t *out8, int32_t *shape_n, double *coords);

/* ---- SOAP site descriptors (site_descriptors/SOAP.py, which asks QUIP or DScribe) --------------------------------------------- */

/* The SOAP power spectrum of every centre of centers[P, 3] in the lattice static_pos[S, 3] under the context's cell
 * (csrc/soap_plan.h; the GTO construction of Himanen et al. 2020 - agreement with a DScribe or QUIP
 * installation is not claimed).  species_idx[S] (int32) is the index of an atom's species in the environment list, -1: not in the
 * environment.  Per environment species Z the density is a Gaussian of width sigma on every periodic image of every atom of Z
 * within cutoff of the centre (hard cut; with width = cutoff_transition_width > 0 weighted by 1 up to cutoff - width and
 * 0.5 (1 + cos(pi (d - cutoff + width) / width)) beyond); it is expanded in g_nl(r) = sum_n' beta[l][n][n'] r^l exp(-alpha[l][n'] r^2)
 * times real orthonormal spherical harmonics - alpha[(l_max + 1), n_max] and beta[(l_max + 1), n_max, n_max] are the caller's
 * tables - and out[P, n_dim] holds p = pi sqrt(8 / (2 l + 1)) sum_m c_Z1,nlm c_Z2,n'lm: species pairs outermost in the order of the
 * environment list (crossover: all Z1 <= Z2, else Z1 = Z2), then n, then n' (n' >= n when Z1 = Z2), then l.  n_dim must be the
 * length sit_soap_plan reports.  nbr_count[P] (optional, int32): the images within the cutoff.  Complete for any cell shape,
 * cells shorter than the cutoff and positions outside the cell; a centre on an atom is an ordinary input; every sum runs in a
 * fixed order (no floating-point atomics): the same bytes on every call.  SIT_ERR_INVALID: a missing array, a species index
 * >= n_species, a cutoff, sigma or exponent that is not positive, width outside [0, cutoff], a cutoff beyond 255 perpendicular
 * heights of the cell, a position that is not finite or more than 2^20 cells from the origin; SIT_ERR_CAPACITY (the message names
 * the limit): l_max > 8, n_max > 8, more than 4 species.  P = 0 is SIT_OK and touches nothing.  Reads nothing of the context but
 * its cell: frames, rows, labels and their validity stay as they are.                                                          */
int sit_soap_vectors(sit_ctx *ctx, const double *static_pos, const int32_t *species_idx, int64_t S, const double *centers, int64_t P,
                     double cutoff, double width, double sigma, int64_t n_species, int64_t n_max, int64_t l_max, int crossover,
                     const double *alpha, const double *beta, int64_t n_dim, double *out, int32_t *nbr_count);
/* The plan of the SOAP entry points for cell[9] (rows are the cell vectors), no context needed: out12 = {the translations
 * |t_a| <= out12[a] as in sit_barrier_plan, threads per workgroup, neighbours staged at once (longer lists are taken in rounds),
 * LDS bytes per workgroup, the largest l_max, n_max and number of species, coefficients per environment, n_dim without and with
 * crossover}.  SIT_ERR_INVALID: a degenerate cell, a cutoff not positive or beyond 255 heights; SIT_ERR_CAPACITY: beyond a limit
 * (the first nine values are set).                                                                                              */
int sit_soap_plan(const double *cell, double cutoff, int64_t n_species, int64_t n_max, int64_t l_max, int64_t *out12);
/* SOAPDescriptorAverages (SOAP.py:248-320) on the resident labels [F, M]: one SOAP vector per assigned mobile ion per strided frame
 * (frame % stepsize == 0), taken among the static atoms static_idx[S] (columns of the frame, with species_idx[S] as above) OF ITS
 * OWN FRAME, multiplied by 1 / averagings[site] and added to its row.  positions: a host [F, A, 3] array, staged in chunks of
 * strided frames within workspace_bytes (0: 1 GiB; a cap below one frame is SIT_ERR_INVALID), or NULL for the resident frames;
 * mobile_idx[M] names the atoms of the label columns.  The bucket plan (csrc/soap_plan.h): counts[K] = strided frames in which a
 * site holds at least one ion; of several ions on one site in one frame the last in ion order contributes; averaging is the
 * argument, or floor(mean(counts) / avg_descriptors_per_site) with 0 made 1 (exactly one of the two is positive);
 * nr_of_descs[K] = max(counts / averaging, 1), averagings = averaging, or counts where counts < averaging; the k-th frame of a
 * site goes to row first_row + k / averagings while that is one of its rows; a site never visited keeps one zero row.  The
 * vectors of a row are added in ascending frame order; nothing depends on arrival.  Every call sets *n_rows, counts and
 * nr_of_descs; when descs is given and *n_rows <= row_cap it also fills descs[*n_rows, n_dim].  info4 (optional) = {kernel
 * milliseconds (HIP events), contributing environments, chunks, the averaging used (0: it came out as 0 and 1 was taken)}.
 * Labels are looked at before anything is indexed with them, as in sit_clamp_trajectory.  Errors as sit_soap_vectors.  Reads
 * only: frames, rows, labels and their validity stay as they are.                                                            */
int sit_soap_site_averages(sit_ctx *ctx, const double *positions, int64_t F, int64_t A, const int64_t *static_idx,
                           const int32_t *species_idx, int64_t S, const int64_t *mobile_idx, int64_t M, int64_t K, int64_t stepsize,
                           int64_t averaging, int64_t avg_descriptors_per_site, double cutoff, double width, double sigma,
                           int64_t n_species, int64_t n_max, int64_t l_max, int crossover, const double *alpha, const double *beta,
                           int64_t n_dim, int64_t workspace_bytes, int64_t row_cap, int64_t *n_rows, int64_t *counts,
                           int64_t *nr_of_descs, double *descs, double *info4);

/* ---- SiteTypeAnalysis (site_descriptors/SiteTypeAnalysis.py, which asks sklearn's PCA and pydpc) ---------------------------- */

/* The plan of the density-peak entry points for points of d coordinates (csrc/dpc_plan.h), no context
 * needed: out12 = {threads per workgroup, points per tile, digit bits and passes of the radix select, the largest d, LDS bytes per
 * workgroup at this d, segments of the density and delta sums, the largest N; of the PCA entry points: rows per chunk, the edge of
 * a workgroup's block of covariance entries, the largest D and N}.  SIT_ERR_INVALID: d < 1; SIT_ERR_CAPACITY: d > 32 (everything
 * but the LDS bytes is set).                                                                                                   */
int sit_dpc_plan(int64_t d, int64_t *out12);
/* Column means and covariance of the rows X[N, D] (PCA.fit, SiteTypeAnalysis.py:83-84): mean[D] = sum / N, cov[D, D] = the sum
 * over rows of (x - mean)(x - mean)^T / max(N - 1, 1), in float64.  Every sum runs in a fixed order (rows in chunks of 1024, a
 * chunk's rows one by one, the chunks one by one; no atomics): the same bytes on every call, and cov is symmetric bit for bit.
 * The eigen-decomposition of cov is the caller's (numpy.linalg.eigh).  SIT_ERR_INVALID: a missing array, N < 1 or D < 1, a value
 * that is not finite or beyond 1e150; SIT_ERR_CAPACITY (the message names the limit): D > 4096, N > 2^25, chunk sums beyond
 * 8 GiB.  Reads nothing of the context but its device and stream: frames, rows, labels and their validity stay as they are.    */
int sit_pca_covariance(sit_ctx *ctx, const double *X, int64_t N, int64_t D, double *mean, double *cov);
/* The projection Y[N, d] = (X - mean) comps^T for comps[d, D] (PCA.transform): Y[r, k] = the sum over ascending c of
 * (X[r, c] - mean[c]) comps[k, c], one thread per entry.  Errors and context as sit_pca_covariance; d > 32 is SIT_ERR_CAPACITY. */
int sit_pca_project(sit_ctx *ctx, const double *X, int64_t N, int64_t D, const double *mean, const double *comps, int64_t d,
                    double *Y);
/* What pydpc.Cluster(Y, fraction) computes (SiteTypeAnalysis.py:99) for the points Y[N, d], without its N x N distance matrix
 * (csrc/dpc_plan.h; Rodriguez & Laio 2014; agreement with a pydpc installation is not claimed).  d(i, j) = sqrt(sum_k (y_ik -
 * y_jk)^2), k ascending, no contraction.  *kernel_size = the distance of rank min(floor(0.5 + fraction n), n - 1) among the
 * n = N (N - 1) / 2 distances i < j, found exactly by a radix select on the bit pattern (eight counting passes with integer
 * atomics).  density[i] = sum over j != i of exp(-(d(i, j) / kernel_size)^2) in a fixed order (kernel_size 0: the number of points
 * that coincide with i).  j is above i iff density[j] > density[i], or they are equal and j < i; delta[i] = the smallest distance
 * to a point above i, neighbour[i] (int32) = that point, of equal distances the highest; the top point has neighbour -1 and the
 * largest delta of the others.  The same bytes on every call.  info2 (optional) = {milliseconds from the first kernel to the last
 * (HIP events; the eight 2 KiB read-backs of the select lie in between), n}.  SIT_ERR_INVALID: a missing array, N < 2, d < 1,
 * fraction outside (0, 1), a coordinate that is not finite or beyond 1e150; SIT_ERR_CAPACITY (the message names the limit):
 * d > 32, N > 2^24.  Reads nothing of the context but its device and stream.                                                  */
int sit_dpc_graph(sit_ctx *ctx, const double *Y, int64_t N, int64_t d, double fraction, double *kernel_size, double *density,
                  double *delta, int32_t *neighbour, double *info2);
/* pydpc's Cluster.assign(min_density, min_delta) and the votes of SiteTypeAnalysis.py:143-147.  Centres are the points with
 * density > min_density and delta > min_delta: clusters[N] (int32) receives their indices in ascending order, *n_clusters their
 * number.  membership[N] (int32): a centre its number, every other point the membership of its neighbour, transitively (pointer
 * jumping in rounds of plain launches); a chain that ends at a point that is no centre and has no neighbour gives -1.  votes
 * (optional, with K > 0 and K * *n_clusters <= votes_cap): votes[K, *n_clusters] = the points of site dvecs_to_site[i] with
 * membership m, counted with integer atomics.  SIT_ERR_INVALID: a missing array, N < 2, a density or delta that is not finite,
 * a threshold that is NaN, a neighbour outside [-1, N) or chains that close on themselves, a site index outside [0, K);
 * SIT_ERR_CAPACITY: N > 2^24.  Reads nothing of the context but its device and stream.                                        */
int sit_dpc_assign(sit_ctx *ctx, const double *density, const double *delta, const int32_t *neighbour, int64_t N,
                   double min_density, double min_delta, const int64_t *dvecs_to_site, int64_t K, int32_t *membership,
                   int32_t *clusters, int64_t *n_clusters, int64_t *votes, int64_t votes_cap);

/* ---- frame sharding across GPUs ------------------------------------ */

/* The reference has no communication layer (it is single-process); these are the exchange steps a frame-sharded
 * run() adds between one process per GPU: RCCL collectives over xGMI on the context's device and stream.  The buffers
 * of sit_comm_allreduce / _allgather / _broadcast are HOST buffers (small per-rank statistics: first-offender keys,
 * counts, site-centre sums; payloads of up to 512 bytes go through the context's pinned block); the large statistics of
 * the mcl plugin - the D x D Gram matrix of landmark/cluster/mcl.py:55, the weighted row sums of :114-122 - never leave
 * the device: see sit_comm_attach.  librccl.so is loaded on the first call.                               */
int sit_comm_unique_id(uint8_t *id128);                 /* ncclGetUniqueId: rank 0 makes it, every rank gets it */
int sit_comm_create(sit_ctx *ctx, const uint8_t *id128, int rank, int world);
int sit_comm_destroy(sit_ctx *ctx);
/* What the communicator says about itself: out6 = {ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclGetVersion,
 * the world size and the rank sit_comm_create was given}.  bench.py prints it from every rank.            */
int sit_comm_info(sit_ctx *ctx, int32_t *out6);
/* In place on buf[count]; dtype 0 = float64, 1 = int64, 2 = uint64; op 0 = sum, 1 = min, 2 = max.       */
int sit_comm_allreduce(sit_ctx *ctx, void *buf, int64_t count, int dtype, int op);
/* recv[world * nbytes] = every rank's send[nbytes] in rank order.                                        */
int sit_comm_allgather(sit_ctx *ctx, const void *send, void *recv, int64_t nbytes);
int sit_comm_broadcast(sit_ctx *ctx, void *buf, int64_t nbytes, int root);
int sit_comm_barrier(sit_ctx *ctx);
/* The communicator of `comm_ctx` (same device) reduces `ctx`'s mcl statistics where they are: after this call
 * sit_gram / sit_gram_limbs / sit_weighted_row_sums(_limbs) of `ctx` return the sums over all ranks (the exact
 * 128-bit accumulators are split into three int64 words on the device, all-reduced with one ncclAllReduce on
 * `ctx`'s stream and joined with their carries: the same bits for any number of ranks, no host round trip).
 * comm_ctx = NULL detaches.  (landmark/cluster/mcl.py:53-59,114-122 in a frame-sharded run.)              */
int sit_comm_attach(sit_ctx *ctx, sit_ctx *comm_ctx);

/* ---- measurement --------------------------------------------------------------------- */

/* Device time (ms, HIP events on the library's stream) of the last call of each stage:
 * [0] fill (+assign)  [1] fit  [2] predict  [3] gram  [4] site centres  [5] occupancy
 * [6] H2D of frames, [7] unused.  With n = 24: [8, 16) the sums over all calls of each
 * stage so far and [16, 24) their numbers - a caller that times a loop reads them before
 * and after instead of once per pass.                                                     */
int sit_timers(sit_ctx *ctx, double *ms, int n);
/* Diagnostics of the pruning tables and the last fill: [0] row width (loose table), [1] mean
 * candidates per bin (loose), [2] longest tight list, [3] mean candidates per bin (tight),
 * [4] delta (sampled static displacement bound, A), [5] frames of the last fill that exceeded
 * delta, [6..8] loose grid, [9..11] tight grid, [12] frames per workgroup of the last fill,
 * [13] steps (speculate / walk / verify / commit) / [14] rows applied one at a time (cluster-founding rows and the
 * rows at a cut) / [15] steps cut short by a wrong speculation, summed over the speculative fits of the context,
 * [16] generation of the fill kernel the last sit_fill launched (1 or 3), [17] survivor slots per wave and
 * [18] waves per workgroup of that launch, [19] capacity bits that ended a speculative fit (0: none) and
 * [20] the row it stopped at, [21] task-table entries per wave of that launch, [22] 1 if the last sit_fill assigned the narrow rows inside the fill kernel, [23] diagonal cells: groups of passes of the last fill that fell inside the error band of the cheap cut-off decision and were repeated with the reference's arithmetic, [24..27] work census of a SITATOR_DEBUG_STOP=9 fill,
 * [28] the window form of k_fill3 in the last sit_fill: 0 = the flat task space, otherwise the slot form (a D0 lane per
 * (ion, slot of its candidate list)) and the widest slots per ion a window of that launch could take (8: every list fits
 * eight slots; 16 / 32 / 64: a frame that meets a longer list runs that many slots per ion).                 */
int sit_info(sit_ctx *ctx, double *out, int n);
/* Diagnostic read-back of a pruning table as it lies on the device (which = 0: the loose table of sit_set_basis, 1: the
 * tight table the first sit_fill over the frames of a basis builds).  Always written (each may be NULL): G3[3] the grid,
 * *displacement the static displacement the table was built for, *rb the covering radius of a bin it was built with,
 * *total its entries.  off [G3[0] * G3[1] * G3[2] + 1] (bin (x, y, z) is index (x * G3[1] + y) * G3[2] + z), list [total]
 * the landmarks of every bin, ascending, and crit [total] the critical vertex of every entry are copied when given
 * (list_cap counts the elements of list and of crit); a call with all three NULL sizes the second.  SIT_ERR_INVALID with
 * a message: no basis, a capacity too small, or that table does not exist (a tight table is dropped by sit_set_basis
 * and by new frames).  Not part of any hot path (tests/test_gpu_candidates.py).                              */
int sit_candidate_table(sit_ctx *ctx, int which, int32_t *G3, double *displacement, double *rb, int64_t *total,
                        int64_t off_cap, int32_t *off, int64_t list_cap, int32_t *list, uint8_t *crit);
int sit_synchronize(sit_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* SITATOR_HIP_H */
