// SOAP site descriptors (site_descriptors/SOAP.py) on the device.  The reference hands every environment to QUIP or DScribe; here
// the power spectrum of soap_plan.h is evaluated by one workgroup per environment.  soap_plan.h has every decision and every
// per-point formula - the translations, the solid harmonics, the primitive, the switch, the contraction, the capacities, the
// bucket plan of SOAPDescriptorAverages; this file has the launches.
//
// k_soap, one workgroup per environment, three phases:
//   find      a lane per static atom of a tile of SP_BLOCK atoms counts its periodic images within the cutoff, a workgroup scan
//             gives every image its place, and the images are written to the LDS list in (atom, m0, m1, m2) order;
//   expand    per listed neighbour the (l_max + 1)^2 solid harmonics and the n_max (l_max + 1) radial values are written to LDS
//             once; every lane then adds, neighbour by neighbour in list order, to the coefficients (Z, n, l, m) it owns - in
//             registers, across the rounds of a list longer than SP_NBR_CAP;
//   contract  a lane per feature walks the feature table and sums over m ascending.
// No floating-point atomics: the same bytes on every call.  Float64 throughout.
#include <algorithm>

#include "sit_internal.h"
#include "soap_plan.h"

struct SoapArgs {
    Pbc pbc;
    BarrierPlan pl;
    SoapShape sh;
    double cutoff, width;
    const double *K, *gam, *beta, *norm;               // [l][n'], [l][n'], [l][n][n'], [L2]
    const i32 *feat;
    i64 n_dim;
    const double *pos;                                 // the static atoms: pos + slot * frame_stride + 3 * static_cols[s]
    i64 frame_stride;
    const i32 *static_cols;                            // nullptr: s itself
    const i32 *species;                                // [S], < 0: not in the environment
    i64 S;
    const double *centers;                             // [P, 3], or nullptr: the ion of the entry in its frame
    const i64 *entry;                                  // frame * M + ion
    const i32 *mobile_cols;
    i64 M, stepsize, slot0;
    const double *scale;                               // per environment, or nullptr
    double *out;                                       // [P, n_dim]
    i32 *nbr_count;                                    // [P] or nullptr
    unsigned *status;                                  // [0] != 0: a position that is not finite or too far from the origin
};

// harmonics and radial values of the n staged neighbours, then every lane's coefficients += its neighbours in list order
__device__ __forceinline__ void soap_accumulate(const SoapShape &sh, int n, const double *nb, const int *nbz, double *harm, double *rad,
                                                const double *tK, const double *tg, const double *tb, const double *norm,
                                                const int (&own)[SP_MAX_OWN], double (&acc)[SP_MAX_OWN])
{
    const int items = n * (sh.l_max + 2);
    for (int it = threadIdx.x; it < items; it += SP_BLOCK) {
        if (it < n) {
            sp_solid_harmonics(nb[SP_NBR_REC * it], nb[SP_NBR_REC * it + 1], nb[SP_NBR_REC * it + 2], sh.l_max, norm, harm + it * sh.L2);
        } else {
            const int i = (it - n) / (sh.l_max + 1), l = (it - n) % (sh.l_max + 1);
            const double *p = nb + SP_NBR_REC * i;
            const double d2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2], w = p[3];
            double e[SP_MAX_N];
#pragma unroll
            for (int k = 0; k < SP_MAX_N; k++) e[k] = k < sh.n_max ? sp_primitive(tK[l * sh.n_max + k], tg[l * sh.n_max + k], d2) : 0.0;
            for (int m = 0; m < sh.n_max; m++) {
                const double *b = tb + (l * sh.n_max + m) * sh.n_max;
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < SP_MAX_N; k++)
                    if (k < sh.n_max) s += b[k] * e[k];
                rad[i * sh.NR + m * (sh.l_max + 1) + l] = w * s;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SP_MAX_OWN; k++) {
        if (own[k] < 0) continue;
        const int z = own[k] >> 16, r = (own[k] >> 8) & 255, lm = own[k] & 255;
        double s = acc[k];
        for (int i = 0; i < n; i++)
            if (nbz[i] == z) s += rad[i * sh.NR + r] * harm[i * sh.L2 + lm];
        acc[k] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SP_BLOCK) void k_soap(SoapArgs a)
{
    extern __shared__ double lds[];
    const SoapShape sh = a.sh;
    const int tab = (sh.l_max + 1) * sh.n_max;
    double *nb = lds;
    double *harm = nb + SP_NBR_CAP * SP_NBR_REC;
    double *rad = harm + SP_NBR_CAP * sh.L2;
    double *coef = rad + SP_NBR_CAP * sh.NR;
    double *tK = coef + sh.n_coef, *tg = tK + tab, *tb = tg + tab;
    int *nbz = (int *)(tb + tab * sh.n_max), *wsum = nbz + SP_NBR_CAP;
    const i64 p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (SP_WAVE - 1), wave = tid / SP_WAVE;

    for (int k = tid; k < tab; k += SP_BLOCK) { tK[k] = a.K[k]; tg[k] = a.gam[k]; }
    for (int k = tid; k < tab * sh.n_max; k += SP_BLOCK) tb[k] = a.beta[k];

    const double *sp = a.pos;
    double x[3], fx[3];
    if (a.centers) {
        for (int k = 0; k < 3; k++) x[k] = a.centers[3 * p + k];
    } else {
        const i64 e = a.entry[p], f = e / a.M, ion = e % a.M;
        sp += (f / a.stepsize - a.slot0) * a.frame_stride;
        for (int k = 0; k < 3; k++) x[k] = sp[3 * (i64)a.mobile_cols[ion] + k];
    }
    cp_to_cell(a.pbc, x, fx);
    bool bad = !(fabs(fx[0]) <= BP_MAX_FRAC && fabs(fx[1]) <= BP_MAX_FRAC && fabs(fx[2]) <= BP_MAX_FRAC);

    int own[SP_MAX_OWN];
    double acc[SP_MAX_OWN];
#pragma unroll
    for (int k = 0; k < SP_MAX_OWN; k++) {
        const int q = tid + k * SP_BLOCK;
        acc[k] = 0.0;
        own[k] = -1;
        if (q < sh.n_coef) {
            const int z = q / (sh.n_max * sh.L2), rem = q % (sh.n_max * sh.L2), n = rem / sh.L2, lm = rem % sh.L2;
            int l = 0;
            while ((l + 1) * (l + 1) <= lm) l++;
            own[k] = (z << 16) | ((n * (sh.l_max + 1) + l) << 8) | lm;
        }
    }

    int fill = 0;
    i64 found = 0;
    for (i64 first = 0; first < a.S; first += SP_BLOCK) {
        const i64 s = first + tid;
        int cnt = 0, z = -1, lo[3] = {1, 1, 1}, hi[3] = {0, 0, 0};
        double b[3] = {0.0, 0.0, 0.0};
        if (s < a.S) {
            const double *ps = sp + 3 * (a.static_cols ? (i64)a.static_cols[s] : s);
            const double q[3] = {ps[0], ps[1], ps[2]};
            double fs[3];
            cp_to_cell(a.pbc, q, fs);
            bad = bad || !(fabs(fs[0]) <= BP_MAX_FRAC && fabs(fs[1]) <= BP_MAX_FRAC && fabs(fs[2]) <= BP_MAX_FRAC);
            z = a.species[s];
            if (z >= 0 && !bad) {
                for (int k = 0; k < 3; k++) {
                    b[k] = q[k] - x[k];
                    bp_axis_range(fx[k] - fs[k], a.pl.q[k], a.pl.n[k], &lo[k], &hi[k]);
                }
                if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) { lo[0] = 1; hi[0] = 0; }
            }
        }
        // the image (m0, m1, m2) of the lane's atom relative to the centre, and whether it lies within the cutoff
        auto image = [&](int m0, int m1, int m2, double pv[3]) -> bool {
            pv[0] = b[0] + (((double)m0 * a.pbc.cm[0] + (double)m1 * a.pbc.cm[1]) + (double)m2 * a.pbc.cm[2]);
            pv[1] = b[1] + (((double)m0 * a.pbc.cm[3] + (double)m1 * a.pbc.cm[4]) + (double)m2 * a.pbc.cm[5]);
            pv[2] = b[2] + (((double)m0 * a.pbc.cm[6] + (double)m1 * a.pbc.cm[7]) + (double)m2 * a.pbc.cm[8]);
            return (pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2] <= a.pl.rc2;
        };
        for (int m0 = lo[0]; m0 <= hi[0]; m0++)
            for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                    double pv[3];
                    if (image(m0, m1, m2, pv)) cnt++;
                }
        // where the lane's images go: an exclusive scan over the workgroup in lane order
        int incl = cnt;
        for (int off = 1; off < SP_WAVE; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        __syncthreads();                                         // the scan words of the tile before are read
        if (lane == SP_WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        int off = incl - cnt, total = 0;
        for (int w = 0; w < SP_BLOCK / SP_WAVE; w++) {
            if (w < wave) off += wsum[w];
            total += wsum[w];
        }
        found += total;
        int done = 0;
        while (done < total) {                                   // uniform: total, done and fill are the same in every lane
            const int room = SP_NBR_CAP - fill;
            if (cnt && off < done + room && off + cnt > done) {
                int j = off;
                for (int m0 = lo[0]; m0 <= hi[0]; m0++)
                    for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                        for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                            double pv[3];
                            if (!image(m0, m1, m2, pv)) continue;
                            if (j >= done && j < done + room) {
                                const int slot = fill + (j - done);
                                const double d = sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]);
                                nb[SP_NBR_REC * slot] = pv[0]; nb[SP_NBR_REC * slot + 1] = pv[1]; nb[SP_NBR_REC * slot + 2] = pv[2];
                                nb[SP_NBR_REC * slot + 3] = sp_switch(d, a.cutoff, a.width);
                                nbz[slot] = z;
                            }
                            j++;
                        }
            }
            const int take = total - done < room ? total - done : room;
            fill += take; done += take;
            __syncthreads();
            if (fill == SP_NBR_CAP) {
                soap_accumulate(sh, fill, nb, nbz, harm, rad, tK, tg, tb, a.norm, own, acc);
                fill = 0;
            }
        }
    }
    if (fill) soap_accumulate(sh, fill, nb, nbz, harm, rad, tK, tg, tb, a.norm, own, acc);
    if (bad) atomicOr(a.status, 1u);

#pragma unroll
    for (int k = 0; k < SP_MAX_OWN; k++)
        if (own[k] >= 0) coef[tid + k * SP_BLOCK] = acc[k];
    __syncthreads();
    const double scale = a.scale ? a.scale[p] : 1.0;
    for (i64 f = tid; f < a.n_dim; f += SP_BLOCK) {
        const double v = sp_contract(coef + a.feat[3 * f] * sh.L2, coef + a.feat[3 * f + 1] * sh.L2, a.feat[3 * f + 2]);
        a.out[p * a.n_dim + f] = a.scale ? v * scale : v;
    }
    if (a.nbr_count && tid == 0) a.nbr_count[p] = (i32)(found < 0x7fffffff ? found : 0x7fffffff);
}

// descs[row] += the vectors of its contributors of this chunk, in their order: one workgroup per touched row
__global__ __launch_bounds__(256) void k_soap_rows(const i64 *crow, const i64 *cptr, const i64 *cidx, const double *vec, i64 n_dim, double *descs)
{
    const i64 row = crow[blockIdx.x], lo = cptr[blockIdx.x], hi = cptr[blockIdx.x + 1];
    for (i64 f = threadIdx.x; f < n_dim; f += 256) {
        double s = descs[row * n_dim + f];
        for (i64 j = lo; j < hi; j++) s += vec[cidx[j] * n_dim + f];
        descs[row * n_dim + f] = s;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct SoapHost {
    SoapShape sh;
    BarrierPlan pl;
    std::vector<double> K, gam, norm;
    std::vector<i32> feat;
    i64 n_dim = 0;
    size_t lds_bytes = 0;
};

struct SoapDev {
    double *K, *gam, *beta, *norm;
    i32 *feat;
    unsigned *status;
};

static int soap_capacity(std::string &msg, const char *who, int what)
{
    char text[160];
    snprintf(text, sizeof(text), "%s: %s", who, what == 1 ? "l_max beyond the capacity of 8" : what == 2 ? "n_max outside [1, 8]"
                                                : "more than 4 environment species (or none)");
    msg = text;
    return SIT_ERR_CAPACITY;
}

static int soap_prepare(sit_ctx *c, const char *who, double cutoff, double width, double sigma, i64 n_species, i64 n_max, i64 l_max,
                        int crossover, const double *alpha, const double *beta, SoapHost &h)
{
    int what = 0;
    if (!sp_shape((int)std::min<i64>(std::max<i64>(n_species, -1), 1000), (int)std::min<i64>(std::max<i64>(n_max, -1), 1000),
                  (int)std::min<i64>(std::max<i64>(l_max, -1), 1000), h.sh, &what))
        return soap_capacity(c->msg, who, what);
    SIT_REQUIRE(c, alpha && beta, "sit_soap: missing radial tables");
    SIT_REQUIRE(c, cutoff > 0.0 && cutoff < INFINITY, "sit_soap: cutoff is not positive");
    SIT_REQUIRE(c, width >= 0.0 && width <= cutoff, "sit_soap: cutoff_transition_width outside [0, cutoff]");
    SIT_REQUIRE(c, sigma > 0.0 && sigma < INFINITY, "sit_soap: atom_sigma is not positive");
    SIT_REQUIRE(c, bp_plan(c->pbc, cutoff, h.pl), "sit_soap: degenerate cell, or cutoff beyond 255 perpendicular heights of the cell");
    const int tab = (h.sh.l_max + 1) * h.sh.n_max;
    const double a = 1.0 / (2.0 * sigma * sigma);
    h.K.resize(tab); h.gam.resize(tab); h.norm.resize(h.sh.L2);
    for (int l = 0; l <= h.sh.l_max; l++)
        for (int n = 0; n < h.sh.n_max; n++) {
            const double al = alpha[l * h.sh.n_max + n];
            SIT_REQUIRE(c, al > 0.0 && al < INFINITY, "sit_soap: an exponent of the radial basis that is not positive");
            sp_prim_consts(a, al, l, &h.K[l * h.sh.n_max + n], &h.gam[l * h.sh.n_max + n]);
        }
    for (int k = 0; k < tab * h.sh.n_max; k++) SIT_REQUIRE(c, fabs(beta[k]) < INFINITY, "sit_soap: a radial coefficient that is not finite");
    sp_harmonic_norms(h.sh.l_max, h.norm.data());
    h.n_dim = sp_n_dim(h.sh.n_species, h.sh.n_max, h.sh.l_max, crossover);
    h.feat.resize((size_t)(3 * h.n_dim));
    sp_feature_table(h.sh.n_species, h.sh.n_max, h.sh.l_max, crossover, h.feat.data());
    h.lds_bytes = (size_t)sp_lds_doubles(h.sh) * 8;
    return SIT_OK;
}

static void soap_take(Carve &cv, const SoapHost &h, SoapDev &d)
{
    const int tab = (h.sh.l_max + 1) * h.sh.n_max;
    d.K = cv.take<double>(tab, 64); d.gam = cv.take<double>(tab, 64); d.beta = cv.take<double>(tab * h.sh.n_max, 64);
    d.norm = cv.take<double>(h.sh.L2, 64); d.feat = cv.take<i32>(3 * h.n_dim, 64); d.status = cv.take<unsigned>(16, 64);
}

static int soap_upload(sit_ctx *c, const SoapHost &h, const double *beta, const SoapDev &d, SoapArgs &a, double cutoff, double width)
{
    const int tab = (h.sh.l_max + 1) * h.sh.n_max;
    int rc;
    if ((rc = copy_to_device(c, d.K, h.K.data(), (size_t)tab * 8))) return rc;
    if ((rc = copy_to_device(c, d.gam, h.gam.data(), (size_t)tab * 8))) return rc;
    if ((rc = copy_to_device(c, d.beta, beta, (size_t)tab * h.sh.n_max * 8))) return rc;
    if ((rc = copy_to_device(c, d.norm, h.norm.data(), (size_t)h.sh.L2 * 8))) return rc;
    if ((rc = copy_to_device(c, d.feat, h.feat.data(), (size_t)h.n_dim * 12))) return rc;
    HIP_TRY(c, hipMemsetAsync(d.status, 0, 64, c->stream));
    HIP_TRY(c, lds_limit((const void *)k_soap, h.lds_bytes, c->device));
    a.pbc = c->pbc; a.pl = h.pl; a.sh = h.sh; a.cutoff = cutoff; a.width = width;
    a.K = d.K; a.gam = d.gam; a.beta = d.beta; a.norm = d.norm; a.feat = d.feat; a.n_dim = h.n_dim; a.status = d.status;
    return SIT_OK;
}

// the status word of the launches so far (the stream is waited for)
static int soap_status(sit_ctx *c, const SoapDev &d)
{
    unsigned *h_status = (unsigned *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_status, d.status, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    SIT_REQUIRE(c, h_status[0] == 0, "sit_soap: a position that is not finite or more than 2^20 cells from the origin");
    return SIT_OK;
}

extern "C" int sit_soap_plan(const double *cell, double cutoff, i64 n_species, i64 n_max, i64 l_max, i64 *out12)
{
    if (!cell || !out12) return SIT_ERR_INVALID;
    struct { double cm[9]; } c;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) c.cm[3 * k + j] = cell[3 * j + k];
    BarrierPlan pl;
    if (!bp_plan(c, cutoff, pl)) return SIT_ERR_INVALID;
    out12[0] = pl.n[0]; out12[1] = pl.n[1]; out12[2] = pl.n[2];
    out12[3] = SP_BLOCK; out12[4] = SP_NBR_CAP; out12[6] = SP_MAX_L; out12[7] = SP_MAX_N; out12[8] = SP_MAX_SPECIES;
    out12[5] = out12[9] = out12[10] = out12[11] = 0;
    SoapShape sh;
    int what;
    if (n_species > 1000 || n_max > 1000 || l_max > 1000 || n_species < -1 || n_max < -1 || l_max < -1 ||
        !sp_shape((int)n_species, (int)n_max, (int)l_max, sh, &what))
        return SIT_ERR_CAPACITY;
    out12[5] = (i64)sp_lds_doubles(sh) * 8; out12[9] = sh.n_coef;
    out12[10] = sp_n_dim(sh.n_species, sh.n_max, sh.l_max, 0); out12[11] = sp_n_dim(sh.n_species, sh.n_max, sh.l_max, 1);
    return SIT_OK;
}

extern "C" int sit_soap_vectors(sit_ctx *c, const double *static_pos, const i32 *species_idx, i64 S, const double *centers, i64 P,
                                double cutoff, double width, double sigma, i64 n_species, i64 n_max, i64 l_max, int crossover,
                                const double *alpha, const double *beta, i64 n_dim, double *out, i32 *nbr_count)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, P >= 0 && S >= 0, "sit_soap_vectors: negative count");
    if (P == 0) return SIT_OK;
    SIT_REQUIRE(c, (S == 0 || (static_pos && species_idx)) && centers && out, "sit_soap_vectors: missing array");
    SIT_REQUIRE(c, P < ((i64)1 << 31) && S < ((i64)1 << 31), "sit_soap_vectors: more than 2^31 centres or atoms");
    SoapHost h;
    int rc = soap_prepare(c, "sit_soap_vectors", cutoff, width, sigma, n_species, n_max, l_max, crossover, alpha, beta, h);
    if (rc) return rc;
    SIT_REQUIRE(c, n_dim == h.n_dim, "sit_soap_vectors: n_dim is not the length of a vector (sit_soap_plan)");
    for (i64 s = 0; s < S; s++) SIT_REQUIRE(c, species_idx[s] < h.sh.n_species, "sit_soap_vectors: a species index beyond the environment");
    HIP_TRY(c, hipSetDevice(c->device));

    SoapDev d;
    double *d_pos, *d_cen;
    i32 *d_spec, *d_cnt;
    rc = carve_scratch(c, [&](Carve &cv) {
        soap_take(cv, h, d);
        d_pos = cv.take<double>(3 * S, 64); d_cen = cv.take<double>(3 * P, 64); d_spec = cv.take<i32>(S, 64); d_cnt = cv.take<i32>(P, 64);
    });
    if (rc) return rc;
    SoapArgs a = SoapArgs();
    if ((rc = soap_upload(c, h, beta, d, a, cutoff, width))) return rc;
    if (S > 0 && (rc = copy_to_device(c, d_pos, static_pos, (size_t)S * 24))) return rc;
    if (S > 0 && (rc = copy_to_device(c, d_spec, species_idx, (size_t)S * 4))) return rc;
    if ((rc = copy_to_device(c, d_cen, centers, (size_t)P * 24))) return rc;
    Scoped buf(c);
    HIP_TRY(c, sit_dmalloc(c, &buf.p, (size_t)(P * h.n_dim) * 8));
    a.pos = d_pos; a.frame_stride = 0; a.static_cols = nullptr; a.species = d_spec; a.S = S; a.centers = d_cen;
    a.M = 1; a.stepsize = 1; a.slot0 = 0; a.out = (double *)buf.p; a.nbr_count = d_cnt;
    k_soap<<<dim3((unsigned)P), dim3(SP_BLOCK), h.lds_bytes, c->stream>>>(a);
    HIP_TRY(c, hipGetLastError());
    if ((rc = soap_status(c, d))) return rc;
    if ((rc = copy_to_host(c, out, buf.p, (size_t)(P * h.n_dim) * 8))) return rc;
    if (nbr_count && (rc = copy_to_host(c, nbr_count, d_cnt, (size_t)P * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

static i64 soap_default_workspace() { return (i64)1 << 30; }

extern "C" int sit_soap_site_averages(sit_ctx *c, const double *positions, i64 F, i64 A, const i64 *static_idx, const i32 *species_idx,
                                      i64 S, const i64 *mobile_idx, i64 M, i64 K, i64 stepsize, i64 averaging,
                                      i64 avg_descriptors_per_site, double cutoff, double width, double sigma, i64 n_species, i64 n_max,
                                      i64 l_max, int crossover, const double *alpha, const double *beta, i64 n_dim, i64 workspace_bytes,
                                      i64 row_cap, i64 *n_rows, i64 *counts, i64 *nr_of_descs, double *descs, double *info4)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_soap_site_averages: assignments needed");
    SIT_REQUIRE(c, F >= 0 && A >= 0 && S >= 0 && M >= 0 && K >= 0 && workspace_bytes >= 0 && row_cap >= 0, "sit_soap_site_averages: negative count");
    SIT_REQUIRE(c, F == c->F && M == c->M, "sit_soap_site_averages: F, M are not the shape of the resident labels");
    SIT_REQUIRE(c, A < ((i64)1 << 31) && F * M < ((i64)1 << 40), "sit_soap_site_averages: more than 2^31 atoms or 2^40 labels");
    SIT_REQUIRE(c, stepsize >= 1, "sit_soap_site_averages: stepsize is not positive");
    SIT_REQUIRE(c, (averaging >= 1) != (avg_descriptors_per_site >= 1), "sit_soap_site_averages: one of averaging and avg_descriptors_per_site");
    SIT_REQUIRE(c, n_rows && counts && nr_of_descs && (S == 0 || (static_idx && species_idx)) && (M == 0 || mobile_idx),
                "sit_soap_site_averages: missing array");
    if (!positions) {
        SIT_REQUIRE(c, c->d_frames && c->A > 0, "sit_soap_site_averages: no resident frames (sit_set_frames first)");
        SIT_REQUIRE(c, A == c->A, "sit_soap_site_averages: A is not the number of atoms of the resident frames");
    }
    SoapHost h;
    int rc = soap_prepare(c, "sit_soap_site_averages", cutoff, width, sigma, n_species, n_max, l_max, crossover, alpha, beta, h);
    if (rc) return rc;
    SIT_REQUIRE(c, n_dim == h.n_dim, "sit_soap_site_averages: n_dim is not the length of a vector (sit_soap_plan)");
    std::vector<i32> scols((size_t)S), mcols((size_t)M);
    for (i64 s = 0; s < S; s++) {
        SIT_REQUIRE(c, static_idx[s] >= 0 && static_idx[s] < A, "sit_soap_site_averages: a static atom outside the frame");
        SIT_REQUIRE(c, species_idx[s] < h.sh.n_species, "sit_soap_site_averages: a species index beyond the environment");
        scols[(size_t)s] = (i32)static_idx[s];
    }
    for (i64 m = 0; m < M; m++) {
        SIT_REQUIRE(c, mobile_idx[m] >= 0 && mobile_idx[m] < A, "sit_soap_site_averages: a mobile atom outside the frame");
        mcols[(size_t)m] = (i32)mobile_idx[m];
    }
    HIP_TRY(c, hipSetDevice(c->device));

    // the labels, looked at before anything is indexed with them, and the bucket plan (soap_plan.h)
    std::vector<i64> labels((size_t)(F * M));
    if (F * M > 0) {
        if ((rc = copy_to_host(c, labels.data(), c->d_labels, (size_t)(F * M) * 8))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    u64 beyond = 0, below = 0;
    for (i64 e = 0; e < F * M; e++) {
        if (labels[(size_t)e] >= K) beyond = std::max<u64>(beyond, (u64)labels[(size_t)e] + 1);
        else if (labels[(size_t)e] < -1) below++;
    }
    if ((rc = label_status(c, "sit_soap_site_averages", beyond, below, K))) return rc;
    std::vector<i64> averagings((size_t)K), first_row((size_t)K), w0((size_t)K), w1((size_t)K), w2((size_t)K);
    sp_bucket_counts(labels.data(), F, M, K, stepsize, counts, w0.data());
    int was_zero = 0;
    const i64 avg = K > 0 ? sp_bucket_averaging(counts, K, averaging, avg_descriptors_per_site, &was_zero) : std::max<i64>(averaging, 1);
    const i64 R = sp_bucket_rows(counts, K, avg, nr_of_descs, averagings.data(), first_row.data());
    *n_rows = R;
    if (info4) { info4[0] = 0.0; info4[1] = 0.0; info4[2] = 0.0; info4[3] = (double)(was_zero ? 0 : avg); }
    if (!descs || row_cap < R) return SIT_OK;                    // the size call
    const i64 N = sp_bucket_contributors(labels.data(), F, M, K, stepsize, nr_of_descs, averagings.data(), first_row.data(), w0.data(),
                                         w1.data(), w2.data(), nullptr, nullptr, nullptr);
    std::vector<i64> entry((size_t)N), row((size_t)N), site((size_t)N);
    sp_bucket_contributors(labels.data(), F, M, K, stepsize, nr_of_descs, averagings.data(), first_row.data(), w0.data(), w1.data(),
                           w2.data(), entry.data(), row.data(), site.data());
    if (info4) info4[1] = (double)N;
    std::fill(descs, descs + R * h.n_dim, 0.0);
    if (N == 0 || R == 0) return SIT_OK;

    // strided frames per chunk: the vectors of its contributors (at most min(M, K) a frame), on the host path the staged frames
    const i64 G = (F + stepsize - 1) / stepsize;                 // strided frames
    const i64 cap = workspace_bytes > 0 ? workspace_bytes : soap_default_workspace();
    const i64 frame_bytes = A * 24, per_frame = std::min(M, K) * h.n_dim * 8 + (positions ? frame_bytes : 0);
    i64 Gc = cap / per_frame;
    SIT_REQUIRE(c, Gc >= 1, "sit_soap_site_averages: the workspace cap is below one frame");
    if (Gc > G) Gc = G;
    const i64 vec_cap = Gc * std::min(M, K);
    SIT_REQUIRE(c, vec_cap < ((i64)1 << 31), "sit_soap_site_averages: more than 2^31 environments in a chunk (lower workspace_bytes)");

    SoapDev d;
    i32 *d_scols, *d_mcols, *d_spec;
    i64 *d_entry, *d_crow, *d_cptr, *d_cidx;
    double *d_scale;
    rc = carve_scratch(c, [&](Carve &cv) {
        soap_take(cv, h, d);
        d_scols = cv.take<i32>(S, 64); d_mcols = cv.take<i32>(M, 64); d_spec = cv.take<i32>(S, 64);
        d_entry = cv.take<i64>(vec_cap, 64); d_scale = cv.take<double>(vec_cap, 64);
        d_crow = cv.take<i64>(vec_cap, 64); d_cptr = cv.take<i64>(vec_cap + 1, 64); d_cidx = cv.take<i64>(vec_cap, 64);
    });
    if (rc) return rc;
    SoapArgs a = SoapArgs();
    if ((rc = soap_upload(c, h, beta, d, a, cutoff, width))) return rc;
    if (S > 0 && (rc = copy_to_device(c, d_scols, scols.data(), (size_t)S * 4))) return rc;
    if (S > 0 && (rc = copy_to_device(c, d_spec, species_idx, (size_t)S * 4))) return rc;
    if ((rc = copy_to_device(c, d_mcols, mcols.data(), (size_t)M * 4))) return rc;
    Scoped buf_vec(c), buf_pos(c), buf_descs(c);
    HIP_TRY(c, sit_dmalloc(c, &buf_vec.p, (size_t)(vec_cap * h.n_dim) * 8));
    HIP_TRY(c, sit_dmalloc(c, &buf_descs.p, (size_t)(R * h.n_dim) * 8));
    if (positions) HIP_TRY(c, sit_dmalloc(c, &buf_pos.p, (size_t)(Gc * frame_bytes)));
    HIP_TRY(c, hipMemsetAsync(buf_descs.p, 0, (size_t)(R * h.n_dim) * 8, c->stream));
    hipEvent_t ev0, ev1;
    HIP_TRY(c, hipEventCreate(&ev0));
    HIP_TRY(c, hipEventCreate(&ev1));
    struct Events { hipEvent_t a, b; ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } events = {ev0, ev1};

    a.static_cols = d_scols; a.species = d_spec; a.S = S; a.centers = nullptr; a.entry = d_entry; a.mobile_cols = d_mcols;
    a.M = M; a.stepsize = stepsize; a.scale = d_scale; a.out = (double *)buf_vec.p; a.nbr_count = nullptr;
    std::vector<double> scale;
    std::vector<i64> order, crow, cptr;
    double kernel_ms = 0.0;
    i64 chunks = 0, i0 = 0;
    for (i64 g0 = 0; g0 < G && i0 < N; g0 += Gc, chunks++) {
        const i64 g1 = std::min(G, g0 + Gc);
        i64 i1 = i0;
        while (i1 < N && entry[(size_t)i1] / M < g1 * stepsize) i1++;
        const i64 n = i1 - i0;
        if (n == 0) continue;
        if (positions) {
            for (i64 g = g0; g < g1; g++)                        // the strided frames of the chunk, side by side
                if ((rc = copy_to_device(c, (char *)buf_pos.p + (g - g0) * frame_bytes, (const char *)positions + g * stepsize * frame_bytes,
                                         (size_t)frame_bytes)))
                    return rc;
            a.pos = (const double *)buf_pos.p; a.frame_stride = A * 3; a.slot0 = g0;
        } else {
            a.pos = c->d_frames; a.frame_stride = A * 3 * stepsize; a.slot0 = 0;
        }
        // the rows the chunk touches and, per row, its contributors in frame order
        scale.resize((size_t)n); order.resize((size_t)n);
        for (i64 i = 0; i < n; i++) { scale[(size_t)i] = 1.0 / (double)averagings[(size_t)site[(size_t)(i0 + i)]]; order[(size_t)i] = i; }
        std::stable_sort(order.begin(), order.end(), [&](i64 u, i64 v) { return row[(size_t)(i0 + u)] < row[(size_t)(i0 + v)]; });
        crow.clear(); cptr.clear();
        for (i64 i = 0; i < n; i++)
            if (i == 0 || row[(size_t)(i0 + order[(size_t)i])] != crow.back()) { crow.push_back(row[(size_t)(i0 + order[(size_t)i])]); cptr.push_back(i); }
        cptr.push_back(n);
        if ((rc = copy_to_device(c, d_entry, entry.data() + i0, (size_t)n * 8))) return rc;
        if ((rc = copy_to_device(c, d_scale, scale.data(), (size_t)n * 8))) return rc;
        if ((rc = copy_to_device(c, d_crow, crow.data(), crow.size() * 8))) return rc;
        if ((rc = copy_to_device(c, d_cptr, cptr.data(), cptr.size() * 8))) return rc;
        if ((rc = copy_to_device(c, d_cidx, order.data(), (size_t)n * 8))) return rc;
        HIP_TRY(c, hipEventRecord(ev0, c->stream));
        k_soap<<<dim3((unsigned)n), dim3(SP_BLOCK), h.lds_bytes, c->stream>>>(a);
        k_soap_rows<<<dim3((unsigned)crow.size()), dim3(256), 0, c->stream>>>(d_crow, d_cptr, d_cidx, (const double *)buf_vec.p, h.n_dim,
                                                                              (double *)buf_descs.p);
        HIP_TRY(c, hipEventRecord(ev1, c->stream));
        HIP_TRY(c, hipGetLastError());
        if ((rc = soap_status(c, d))) return rc;                 // waits: the chunk's tables are reused
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, ev0, ev1));
        kernel_ms += ms;
        i0 = i1;
    }
    if ((rc = copy_to_host(c, descs, buf_descs.p, (size_t)(R * h.n_dim) * 8))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (info4) { info4[0] = kernel_ms; info4[2] = (double)chunks; }
    return SIT_OK;
}
