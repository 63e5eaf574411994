// IntermediateScattering / StructureFactor: raw complex sums of the self and the coherent intermediate scattering function over
// q vectors commensurate with the cell, from the frames as they lie in device memory.  Every decision - the phase of an atom,
// the sine and cosine, the power step, the term, the origins and their blocks, the order of every sum, the batches, windows
// and runs a workspace cap allows, the pieces of a call's buffer (sc_layout) - is in scattering_plan.h.
//
//   k_series_frac    (series.h, with ScReduce) f = s - nearbyint(s), s = x . ci of the columns of the lists, as [frame][3][column]
//   k_sc_density     a run of frames against a tile of q: the three power tables of a tile of (frame, atom) entries are staged
//                    in LDS, a thread owns a q vector and walks the atoms in selection order; rho [selection][q][F]
//   k_sc_coherent    one q, one block of origins and a tile of lags: rho_a(t) is read once, the products of every lag are
//                    added by the tree of sc_tree in LDS; block partials
//   k_sc_self        one lag, one block of origins, a tile of q: for every (origin, atom) d, E and the power tables once, then
//                    two complex products and one complex addition per q; block partials
//   k_sc_reduce      the block partials of a (lag, q), added in block order
// No floating-point atomic anywhere: the same bytes on every call.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "series.h"
#include "scattering_plan.h"
#include "sitator_hip_scattering.h"

extern __shared__ __align__(16) double sc_lds[];      // sc_lds_bytes

struct ScTables { int H[3], off[3], row, tile; };     // off: where the table of an axis begins in an entry's row, in pairs

struct ScQ {
    const int32_t *q;              // [n_q][3]
    i64 q0, nq;                    // the batch: q vectors [q0, q0 + nq)
};

struct ScReduce { __device__ double operator()(double s) const { return sc_reduce(s); } };      // the last step of k_series_frac
static_assert(SERIES_FRAC_THREADS == SC_THREADS, "SC_MAX_FRAC counts workgroups of SC_THREADS for k_series_frac");

// the table of one axis of one entry of the tile, from the reduced coordinate
__device__ __forceinline__ void sc_stage(const ScTables &tb, int slot, int a, double f)
{
    double c, s;
    sc_sincos2pi(f, &c, &s);
    sc_powers(c, s, tb.H[a], sc_lds + ((i64)slot * tb.row + tb.off[a]) * 2);
}

__device__ __forceinline__ void sc_walk_one(const ScTables &tb, int slot, int h, int k, int l, double &re, double &im)
{
    const double *t = sc_lds + (i64)slot * tb.row * 2;
    double tr, ti;
    sc_term(t, t + 2 * tb.off[1], t + 2 * tb.off[2], h, k, l, &tr, &ti);
    re = re + tr;
    im = im + ti;
}

struct ScDensity {
    const double *frac;            // [frames held][3][n_cols]
    i64 n_cols, col0, n;           // the selection: columns [col0, col0 + n)
    i64 f0, nf, F;                 // the frames held: [f0, f0 + nf)
    double *rho;                   // [q of the batch][F][2] of this selection
};

// grid: (runs of SC_RUN frames of the window, tiles of q)
__global__ __launch_bounds__(SC_THREADS) void k_sc_density(ScDensity g, ScQ qs, ScTables tb)
{
    const i64 fr0 = (i64)blockIdx.x * SC_RUN;
    if (fr0 >= g.nf) return;
    const i64 nfr = g.nf - fr0 < SC_RUN ? g.nf - fr0 : SC_RUN, entries = nfr * g.n;
    const i64 j = (i64)blockIdx.y * SC_QTILE + threadIdx.x;
    const bool live = j < qs.nq;
    int h = 0, k = 0, l = 0;
    if (live) { const int32_t *q = qs.q + (qs.q0 + j) * 3; h = q[0]; k = q[1]; l = q[2]; }
    double re = 0.0, im = 0.0;
    i64 atom = 0, fr = 0;                                         // of the entry the walk is at
    for (i64 e0 = 0; e0 < entries; e0 += tb.tile) {
        const int ne = entries - e0 < tb.tile ? (int)(entries - e0) : tb.tile;
        __syncthreads();                                          // the tile before has been walked
        for (int job = threadIdx.x; job < ne * 3; job += SC_THREADS) {
            const int slot = job / 3, a = job - slot * 3;
            const i64 e = e0 + slot, f = e / g.n, i = e - f * g.n;
            sc_stage(tb, slot, a, g.frac[((fr0 + f) * 3 + a) * g.n_cols + g.col0 + i]);
        }
        __syncthreads();
        for (int slot = 0; slot < ne; slot++) {
            if (live) sc_walk_one(tb, slot, h, k, l, re, im);
            if (++atom == g.n) {                                  // the last atom of a frame
                if (live) { double *o = g.rho + (j * g.F + g.f0 + fr0 + fr) * 2; o[0] = re; o[1] = im; }
                re = 0.0; im = 0.0; atom = 0; fr++;
            }
        }
    }
}

struct ScLags {
    const i64 *lags;               // the lags of this launch
    i64 nl, F, stride, n_blocks, qb;
    double *partial;               // [nl][n_blocks][qb][2]
};

// grid: (blocks of origins, tiles of q, lags of the launch)
__global__ __launch_bounds__(SC_THREADS) void k_sc_self(SeriesSource src, i64 n_a, MsdCell cell, ScLags g, ScQ qs, ScTables tb)
{
    const i64 tau = g.lags[blockIdx.z];
    const i64 n_or = series_origins(g.F, tau, g.stride), o_lo = (i64)blockIdx.x * SC_BLOCK;
    if (o_lo >= n_or) return;                                     // the whole workgroup: k_sc_reduce reads no such block
    const i64 o_hi = o_lo + SC_BLOCK < n_or ? o_lo + SC_BLOCK : n_or, entries = (o_hi - o_lo) * n_a;
    const i64 j = (i64)blockIdx.y * SC_QTILE + threadIdx.x;
    const bool live = j < qs.nq;
    int h = 0, k = 0, l = 0;
    if (live) { const int32_t *q = qs.q + (qs.q0 + j) * 3; h = q[0]; k = q[1]; l = q[2]; }
    double re = 0.0, im = 0.0;
    for (i64 e0 = 0; e0 < entries; e0 += tb.tile) {
        const int ne = entries - e0 < tb.tile ? (int)(entries - e0) : tb.tile;
        __syncthreads();
        for (int job = threadIdx.x; job < ne * 3; job += SC_THREADS) {
            const int slot = job / 3, a = job - slot * 3;
            const i64 e = e0 + slot, o = e / n_a, i = e - o * n_a, t = (o_lo + o) * g.stride;
            const double *p = src.at(t, i), *p1 = src.at(t + tau, i);
            const double f_origin = sc_reduce(msd_frac(cell.ci, a, p[0], p[1], p[2]));
            const double f_later = sc_reduce(msd_frac(cell.ci, a, p1[0], p1[1], p1[2]));
            sc_stage(tb, slot, a, sc_delta(f_later, f_origin));
        }
        __syncthreads();
        if (live)
            for (int slot = 0; slot < ne; slot++) sc_walk_one(tb, slot, h, k, l, re, im);
    }
    if (live) {
        double *o = g.partial + ((((i64)blockIdx.z * g.n_blocks + blockIdx.x) * g.qb) + j) * 2;
        o[0] = re; o[1] = im;
    }
}

// grid: (blocks of origins, q of the batch, tiles of SC_LAG_TILE lags); rho_a, rho_b [q of the batch][F][2]
__global__ __launch_bounds__(SC_THREADS) void k_sc_coherent(const double *rho_a, const double *rho_b, ScLags g)
{
    const i64 o_lo = (i64)blockIdx.x * SC_BLOCK, j = blockIdx.y, l0 = (i64)blockIdx.z * SC_LAG_TILE;
    const int nl = g.nl - l0 < SC_LAG_TILE ? (int)(g.nl - l0) : SC_LAG_TILE;
    const int lane = threadIdx.x % SC_BLOCK, half = threadIdx.x / SC_BLOCK;        // two threads per origin: lags of either parity
    const i64 t = (o_lo + lane) * g.stride;
    double ar = 0.0, ai = 0.0;
    if (t < g.F) { const double *a = rho_a + (j * g.F + t) * 2; ar = a[0]; ai = a[1]; }
    for (int x = half; x < nl; x += SC_THREADS / SC_BLOCK) {
        const i64 tau = g.lags[l0 + x];
        double re = 0.0, im = 0.0;
        if (o_lo + lane < series_origins(g.F, tau, g.stride)) {
            const double *b = rho_b + (j * g.F + t + tau) * 2;
            sc_cross(ar, ai, b[0], b[1], &re, &im);
        }
        sc_lds[(x * SC_BLOCK + lane) * 2] = re;
        sc_lds[(x * SC_BLOCK + lane) * 2 + 1] = im;
    }
    for (int d = SC_BLOCK / 2; d >= 1; d >>= 1) {                 // sc_tree, real and imaginary parts apart
        __syncthreads();
        for (int job = threadIdx.x; job < nl * d; job += SC_THREADS) {
            const int x = job / d, i = job - x * d;
            double *v = sc_lds + (x * SC_BLOCK + i) * 2;
            v[0] = v[0] + v[2 * d];
            v[1] = v[1] + v[2 * d + 1];
        }
    }
    __syncthreads();
    if (threadIdx.x < nl && o_lo < series_origins(g.F, g.lags[l0 + threadIdx.x], g.stride)) {
        double *o = g.partial + ((((l0 + threadIdx.x) * g.n_blocks + blockIdx.x) * g.qb) + j) * 2;
        o[0] = sc_lds[threadIdx.x * SC_BLOCK * 2];
        o[1] = sc_lds[threadIdx.x * SC_BLOCK * 2 + 1];
    }
}

// a thread per (lag of the launch, q of the batch); out [n_lags][n_q][2] from the first lag of the launch on
__global__ __launch_bounds__(SC_THREADS) void k_sc_reduce(ScLags g, i64 nq, i64 q0, i64 n_q, double *out)
{
    const i64 i = (i64)blockIdx.x * SC_THREADS + threadIdx.x;
    if (i >= g.nl * nq) return;
    const i64 x = i / nq, j = i - x * nq;
    const i64 nb = sc_blocks(series_origins(g.F, g.lags[x], g.stride));
    double re = 0.0, im = 0.0;
    for (i64 b = 0; b < nb; b++) {
        const double *p = g.partial + ((x * g.n_blocks + b) * g.qb + j) * 2;
        re = re + p[0];
        im = im + p[1];
    }
    double *o = out + (x * n_q + q0 + j) * 2;
    o[0] = re; o[1] = im;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

static ScPlanIn sc_plan_in(i64 F, i64 n_a, i64 n_b, bool same, i64 n_q, const i64 *H, i64 n_lags, i64 stride, bool self_part,
                           bool coherent_part, i64 workspace_bytes)
{
    ScPlanIn in;
    in.F = F; in.n_a = n_a; in.n_b = n_b; in.n_q = n_q; in.n_lags = n_lags; in.stride = stride;
    for (int a = 0; a < 3; a++) in.H[a] = H[a];
    in.same = same; in.want_self = self_part; in.want_coherent = coherent_part; in.workspace_bytes = workspace_bytes;
    return in;
}

extern "C" int sit_scattering_plan(i64 F, i64 n_a, i64 n_b, int same, i64 n_q, const i64 *h_max, i64 n_lags, i64 origin_stride,
                                   int self_part, int coherent_part, i64 workspace_bytes, i64 *out12)
{
    if (!out12 || !h_max) return SIT_ERR_INVALID;
    const ScPlan p = sc_plan(sc_plan_in(F, n_a, n_b, same != 0, n_q, h_max, n_lags, origin_stride, self_part != 0, coherent_part != 0,
                                        workspace_bytes), sp_knobs_from_env().workspace);
    const i64 out[12] = {SC_THREADS, SC_MAX_H, SC_BLOCK, p.tile, p.lds_bytes, p.n_blocks, p.q_batch, p.n_q_batches, p.window,
                         p.lags_per_launch, p.workspace, SC_LAG_TILE};
    for (int i = 0; i < 12; i++) out12[i] = out[i];
    return p.err ? SIT_ERR_INVALID : SIT_OK;
}

extern "C" int sit_scattering(sit_ctx *c, const double *positions, i64 F, i64 A, const i64 *atoms_a, i64 n_a, const i64 *atoms_b, i64 n_b,
                              int same, const i64 *q_int, i64 n_q, const i64 *lags, i64 n_lags, i64 origin_stride, i64 workspace_bytes,
                              double *self_sums, double *coherent_sums)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, self_sums || coherent_sums, "sit_scattering: both outputs are NULL");
    SIT_REQUIRE(c, atoms_a && atoms_b && lags && q_int, "sit_scattering: missing array");
    SIT_REQUIRE(c, n_q >= 1 && n_q <= SC_MAX_Q, "sit_scattering: 1 to 2^16 q vectors are needed");
    i64 H[3];
    SIT_REQUIRE(c, sc_hmax(q_int, n_q, H), "sit_scattering: an index of a q vector is beyond 32");
    const ScPlanIn in = sc_plan_in(F, n_a, n_b, same != 0, n_q, H, n_lags, origin_stride, self_sums != nullptr, coherent_sums != nullptr,
                                   workspace_bytes);
    const ScPlan pl = sc_plan(in, sp_knobs_from_env().workspace);
    if (pl.err) { c->msg = std::string("sit_scattering: ") + pl.err; return SIT_ERR_INVALID; }
    int rc;
    MsdCell cell;
    if ((rc = series_lags(c, "sit_scattering", lags, n_lags, F)) || (rc = series_cell(c, "sit_scattering", &cell, "a degenerate cell"))) return rc;
    if (!positions && (rc = series_resident(c, "sit_scattering", F, A))) return rc;
    SIT_REQUIRE(c, A >= 1, "sit_scattering: no atom in a frame");
    if ((rc = series_atoms_in_range(c, "sit_scattering", atoms_a, n_a, A)) || (rc = series_atoms_in_range(c, "sit_scattering", atoms_b, n_b, A)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    Scoped work(c), upload(c);
    ScPieces w;
    if ((rc = carve_scratch(c, [&](Carve &cv) { w = sc_layout(cv, pl, in); }, &work))) return rc;
    std::vector<int32_t> q32((size_t)(3 * n_q));
    for (i64 i = 0; i < 3 * n_q; i++) q32[(size_t)i] = (int32_t)q_int[i];
    HIP_TRY(c, hipMemcpyAsync(w.atoms, atoms_a, (size_t)n_a * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.atoms + n_a, atoms_b, (size_t)n_b * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.lags, lags, (size_t)n_lags * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.q, q32.data(), (size_t)(3 * n_q) * 4, hipMemcpyHostToDevice, c->stream));
    SeriesSource src;
    if ((rc = series_frames(c, positions, F, A, w.atoms, upload, &src))) return rc;
    ScTables tb;
    for (int a = 0; a < 3; a++) tb.H[a] = (int)H[a];
    tb.off[0] = 0; tb.off[1] = tb.H[0] + 1; tb.off[2] = tb.H[0] + tb.H[1] + 2;
    tb.row = (int)pl.row; tb.tile = (int)pl.tile;
    const size_t lds = (size_t)pl.lds_bytes;
    HIP_TRY(c, lds_limit((const void *)k_sc_density, lds, c->device));
    HIP_TRY(c, lds_limit((const void *)k_sc_self, lds, c->device));
    HIP_TRY(c, lds_limit((const void *)k_sc_coherent, lds, c->device));
    ScLags g;
    g.F = F; g.stride = origin_stride; g.n_blocks = pl.n_blocks; g.qb = pl.q_batch; g.partial = w.partial;
    const auto reduce = [&](const ScQ &qs, i64 l0, double *out) -> int {
        k_sc_reduce<<<dim3((unsigned)((g.nl * qs.nq + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, c->stream>>>(
            g, qs.nq, qs.q0, n_q, out + l0 * n_q * 2);
        HIP_TRY(c, hipGetLastError());
        return SIT_OK;
    };
    for (i64 q0 = 0; q0 < n_q; q0 += pl.q_batch) {
        const ScQ qs = {w.q, q0, n_q - q0 < pl.q_batch ? n_q - q0 : pl.q_batch};
        const unsigned q_tiles = (unsigned)((qs.nq + SC_QTILE - 1) / SC_QTILE);
        if (coherent_sums) {
            for (i64 f0 = 0; f0 < F; f0 += pl.window) {
                const i64 nf = F - f0 < pl.window ? F - f0 : pl.window;
                if ((rc = series_frac<ScReduce>(c, src, 0, pl.n_cols, f0, nf, cell, w.frac))) return rc;
                for (i64 sel = 0; sel < pl.n_sel; sel++) {
                    ScDensity d;
                    d.frac = w.frac; d.n_cols = pl.n_cols; d.col0 = sel ? n_a : 0; d.n = sel ? n_b : n_a;
                    d.f0 = f0; d.nf = nf; d.F = F; d.rho = w.rho + sel * pl.q_batch * F * 2;
                    k_sc_density<<<dim3((unsigned)((nf + SC_RUN - 1) / SC_RUN), q_tiles), dim3(SC_THREADS), lds, c->stream>>>(d, qs, tb);
                    HIP_TRY(c, hipGetLastError());
                }
            }
            const double *rho_b = w.rho + (pl.n_sel - 1) * pl.q_batch * F * 2;
            for (i64 l0 = 0; l0 < n_lags; l0 += pl.lags_per_launch) {
                g.lags = w.lags + l0; g.nl = n_lags - l0 < pl.lags_per_launch ? n_lags - l0 : pl.lags_per_launch;
                k_sc_coherent<<<dim3((unsigned)pl.n_blocks, (unsigned)qs.nq, (unsigned)((g.nl + SC_LAG_TILE - 1) / SC_LAG_TILE)),
                                dim3(SC_THREADS), lds, c->stream>>>(w.rho, rho_b, g);
                HIP_TRY(c, hipGetLastError());
                if ((rc = reduce(qs, l0, w.coherent_sums))) return rc;
            }
        }
        if (self_sums) {
            for (i64 l0 = 0; l0 < n_lags; l0 += pl.lags_per_launch) {
                g.lags = w.lags + l0; g.nl = n_lags - l0 < pl.lags_per_launch ? n_lags - l0 : pl.lags_per_launch;
                k_sc_self<<<dim3((unsigned)pl.n_blocks, q_tiles, (unsigned)g.nl), dim3(SC_THREADS), lds, c->stream>>>(src, n_a, cell, g, qs, tb);
                HIP_TRY(c, hipGetLastError());
                if ((rc = reduce(qs, l0, w.self_sums))) return rc;
            }
        }
    }
    const size_t table = (size_t)(n_lags * n_q) * 16;
    if (self_sums) HIP_TRY(c, hipMemcpyAsync(self_sums, w.self_sums, table, hipMemcpyDeviceToHost, c->stream));
    if (coherent_sums) HIP_TRY(c, hipMemcpyAsync(coherent_sums, w.coherent_sums, table, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (self_sums)
        for (i64 x = 0; x < n_lags; x++)
            if (lags[x] == 0)                                     // every term is 1: origins x n_a, exactly
                for (i64 j = 0; j < n_q; j++) {
                    self_sums[(x * n_q + j) * 2] = (double)(series_origins(F, 0, origin_stride) * n_a);
                    self_sums[(x * n_q + j) * 2 + 1] = 0.0;
                }
    return SIT_OK;
}
