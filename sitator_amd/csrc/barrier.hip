// MergeSitesByBarrier (network/MergeSitesByBarrier.py) on the device: for every candidate pair of sites the energies of one
// mobile atom driven along the straight path between the two centres, in a frozen lattice under a truncated and shifted
// Lennard-Jones potential, and the verdict of :116-125 on them.  The reference asks an ASE calculator for the total energy of
// the whole structure once per image in a Python loop (:109-113); everything but the mobile atom's own energy is constant along
// the path, so only that is summed here.  barrier_plan.h has every decision - the pair term, the translations that can lie
// within the cutoff, the driven point, the verdict, the order of the sum; this file has the launches.
//
// One workgroup per pair.  The static atoms pass through LDS in tiles of BP_TILE records; the four waves take the images in
// turn (image w, w + 4, ...), the 64 lanes of a wave the atoms of the tile, each lane all translations of its atom; a wave's
// 64 partial sums meet in a butterfly, lane 0 adds the tile's sum to the image's energy.  No atomics: the same bytes on every
// call.  Float64 throughout.
#include "sit_internal.h"
#include "pathway_graph.h"
#include "barrier_plan.h"

// the staged form of the static atoms (bp_atom): rec[s * BP_REC ...]
__global__ __launch_bounds__(BP_BLOCK) void k_barrier_atoms(Pbc pbc, const double *pos, const double *eps, const double *sigma, double rc, i64 S,
                                                            double *rec)
{
    const i64 s = (i64)blockIdx.x * BP_BLOCK + threadIdx.x;
    if (s >= S) return;
    const double p[3] = {pos[3 * s], pos[3 * s + 1], pos[3 * s + 2]};
    double r[BP_REC];
    bp_atom(pbc, p, eps[s], sigma[s], rc, r);
    for (int k = 0; k < BP_REC; k++) rec[s * BP_REC + k] = r[k];
}

__global__ __launch_bounds__(BP_BLOCK) void k_barrier_energies(Pbc pbc, BarrierPlan pl, Images27 I, const double *rec, i64 S, const double *centers,
                                                               const i32 *pairs, const double *coeffs, int n, double threshold,
                                                               double *energies, unsigned char *verdict, i32 *code)
{
    __shared__ double tile[BP_TILE * BP_REC];
    __shared__ double path[6];                                   // pos[i], then the vector to the nearest image of pos[j]
    const i64 p = blockIdx.x;
    const int lane = threadIdx.x & (BP_WAVE - 1), wave = threadIdx.x / BP_WAVE;
    if (threadIdx.x == 0) {
        const i64 i = pairs[2 * p], j = pairs[2 * p + 1];
        const double from[3] = {centers[3 * i], centers[3 * i + 1], centers[3 * i + 2]};
        double to[3] = {centers[3 * j], centers[3 * j + 1], centers[3 * j + 2]};
        code[p] = pg_min_image(I.img, from, to);                 // :104-106
        for (int k = 0; k < 3; k++) { path[k] = from[k]; path[3 + k] = to[k] - from[k]; }   // :108
    }
    __syncthreads();
    const double from[3] = {path[0], path[1], path[2]}, vector[3] = {path[3], path[4], path[5]};
    double *e_pair = energies + p * (i64)n;

    for (i64 first = 0; first < S; first += BP_TILE) {
        const int count = (int)(S - first < BP_TILE ? S - first : BP_TILE);
        if (first) __syncthreads();                              // every wave is done with the tile before
        for (int k = threadIdx.x; k < count * BP_REC; k += BP_BLOCK) tile[k] = rec[first * BP_REC + k];
        __syncthreads();
        for (int image = wave; image < n; image += BP_WAVES) {
            double x[3], fx[3];
            bp_driven(from, vector, coeffs[image], x);           // :110-112
            cp_to_cell(pbc, x, fx);
            double part = 0.0;
            for (int a = lane; a < count; a += BP_WAVE) part += bp_atom_energy(pbc, pl, tile + a * BP_REC, x, fx);
            for (int off = BP_WAVE / 2; off; off >>= 1) part += __shfl_xor(part, off);
            if (lane == 0) e_pair[image] = (first ? e_pair[image] : 0.0) + part;
        }
    }
    __syncthreads();                                             // the image energies of the other waves (workgroup-scope fence)
    if (threadIdx.x == 0) {
        uint8_t v[3];
        bp_verdict(e_pair, n, threshold, v);                     // :116-125
        verdict[3 * p] = v[0]; verdict[3 * p + 1] = v[1]; verdict[3 * p + 2] = v[2];
    }
}

extern "C" int sit_barrier_plan(const double *cell, double rc, i64 *out6)
{
    if (!cell || !out6) return SIT_ERR_INVALID;
    struct { double cm[9]; } c;                                  // bp_plan reads the cell vectors only
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) c.cm[3 * k + j] = cell[3 * j + k];
    BarrierPlan pl;
    if (!bp_plan(c, rc, pl)) return SIT_ERR_INVALID;
    out6[0] = pl.n[0]; out6[1] = pl.n[1]; out6[2] = pl.n[2];
    out6[3] = BP_TILE; out6[4] = BP_BLOCK; out6[5] = BP_LDS_BYTES;
    return SIT_OK;
}

extern "C" int sit_barrier_energies(sit_ctx *c, const double *static_pos, const double *eps, const double *sigma, i64 S, double rc,
                                    const double *centers, i64 K, const i32 *pairs, i64 P, const double *coeffs, i64 n, double threshold,
                                    double *energies, uint8_t *verdict, i32 *code)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, P >= 0, "sit_barrier_energies: negative count");
    if (P == 0) return SIT_OK;
    SIT_REQUIRE(c, static_pos && eps && sigma && centers && pairs && coeffs && verdict, "sit_barrier_energies: missing array");
    SIT_REQUIRE(c, S >= 1, "sit_barrier_energies: no coordinating atom");
    SIT_REQUIRE(c, n >= 3, "sit_barrier_energies: fewer than 3 driven images");
    SIT_REQUIRE(c, K >= 0 && K <= BP_MAX_SITES, "sit_barrier_energies: more than 16384 sites");
    SIT_REQUIRE(c, P < ((i64)1 << 31) && n < ((i64)1 << 31) && S < ((i64)1 << 31), "sit_barrier_energies: more than 2^31 pairs, images or atoms");
    SIT_REQUIRE(c, rc > 0.0 && rc < INFINITY, "sit_barrier_energies: rc is not positive");
    BarrierPlan pl;
    SIT_REQUIRE(c, bp_plan(c->pbc, rc, pl), "sit_barrier_energies: degenerate cell, or rc beyond 255 perpendicular heights of the cell");
    for (i64 s = 0; s < S; s++) {
        SIT_REQUIRE(c, eps[s] > 0.0 && eps[s] < INFINITY && sigma[s] > 0.0 && sigma[s] < INFINITY,
                    "sit_barrier_energies: a non-positive epsilon or sigma");
        double f[3];
        cp_to_cell(c->pbc, static_pos + 3 * s, f);
        SIT_REQUIRE(c, fabs(f[0]) <= BP_MAX_FRAC && fabs(f[1]) <= BP_MAX_FRAC && fabs(f[2]) <= BP_MAX_FRAC,
                    "sit_barrier_energies: a coordinating atom that is not finite or more than 2^20 cells from the origin");
    }
    for (i64 k = 0; k < K; k++) {
        double f[3];
        cp_to_cell(c->pbc, centers + 3 * k, f);
        SIT_REQUIRE(c, fabs(f[0]) <= BP_MAX_FRAC && fabs(f[1]) <= BP_MAX_FRAC && fabs(f[2]) <= BP_MAX_FRAC,
                    "sit_barrier_energies: a site centre that is not finite or more than 2^20 cells from the origin");
    }
    for (i64 p = 0; p < 2 * P; p++)
        SIT_REQUIRE(c, pairs[p] >= 0 && (i64)pairs[p] < K, "sit_barrier_energies: a pair index outside the sites");
    for (i64 k = 0; k < n; k++) SIT_REQUIRE(c, fabs(coeffs[k]) <= 2.0, "sit_barrier_energies: an interpolation coefficient outside [-2, 2]");
    HIP_TRY(c, hipSetDevice(c->device));

    // scratch, every piece on a 64-byte boundary: records | raw positions | eps | sigma | centres | pairs | coefficients |
    // energies | verdicts | codes
    double *d_rec, *d_pos, *d_eps, *d_sig, *d_cen, *d_coef, *d_en;
    i32 *d_pair, *d_code;
    unsigned char *d_ver;
    int rc_ = carve_scratch(c, [&](Carve &cv) {
        d_rec = cv.take<double>(S * BP_REC, 64); d_pos = cv.take<double>(3 * S, 64); d_eps = cv.take<double>(S, 64);
        d_sig = cv.take<double>(S, 64); d_cen = cv.take<double>(3 * K, 64); d_pair = cv.take<i32>(2 * P, 64);
        d_coef = cv.take<double>(n, 64); d_en = cv.take<double>(P * n, 64); d_ver = cv.take<unsigned char>(3 * P, 64);
        d_code = cv.take<i32>(P, 64);
    });
    if (rc_) return rc_;
    if ((rc_ = copy_to_device(c, d_pos, static_pos, (size_t)S * 24))) return rc_;
    if ((rc_ = copy_to_device(c, d_eps, eps, (size_t)S * 8))) return rc_;
    if ((rc_ = copy_to_device(c, d_sig, sigma, (size_t)S * 8))) return rc_;
    if ((rc_ = copy_to_device(c, d_cen, centers, (size_t)K * 24))) return rc_;
    if ((rc_ = copy_to_device(c, d_pair, pairs, (size_t)P * 8))) return rc_;
    if ((rc_ = copy_to_device(c, d_coef, coeffs, (size_t)n * 8))) return rc_;
    Images27 I;
    cp_images(c->pbc, I.img);
    k_barrier_atoms<<<dim3((unsigned)((S + BP_BLOCK - 1) / BP_BLOCK)), dim3(BP_BLOCK), 0, c->stream>>>(c->pbc, d_pos, d_eps, d_sig, rc, S, d_rec);
    k_barrier_energies<<<dim3((unsigned)P), dim3(BP_BLOCK), 0, c->stream>>>(c->pbc, pl, I, d_rec, S, d_cen, d_pair, d_coef, (int)n, threshold,
                                                                            d_en, d_ver, d_code);
    HIP_TRY(c, hipGetLastError());
    if (energies && (rc_ = copy_to_host(c, energies, d_en, (size_t)(P * n) * 8))) return rc_;
    if ((rc_ = copy_to_host(c, verdict, d_ver, (size_t)P * 3))) return rc_;
    if (code && (rc_ = copy_to_host(c, code, d_code, (size_t)P * 4))) return rc_;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}
