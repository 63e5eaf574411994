// The front of the frame-series operators (spectrum.hip, msd.hip, vanhove.hip, scattering.hip, density.hip): the checks every
// one of them makes of its cell, its lags, its atom lists and the resident frames, where the selected atoms' positions come
// from, and the tile that turns them into per-atom series that are contiguous along the frames.  A refusal differs between the
// entry points by `who` alone; the plain arithmetic is in series_plan.h.  A selection is n_sel columns: column c of a host
// [F, n_sel, 3] array that is uploaded as it is (A = n_sel, no atom list; series_source), or atom atoms[c] of whole frames of A
// atoms, resident in device memory or uploaded as they are (series_frames); the kernels read either through a SeriesSource.
#pragma once
#include "sit_internal.h"
#include "series_plan.h"

struct MsdCell { double cm[9], ci[9]; };

// The context's cell as a launch reads it.  `what` says why a degenerate one is refused; null: any cell will do.
static inline int series_cell(sit_ctx *c, const char *who, MsdCell *cell, const char *what)
{
    for (int i = 0; i < 9; i++) { cell->cm[i] = c->pbc.cm[i]; cell->ci[i] = c->pbc.ci[i]; }
    if (what) SIT_REQUIRE(c, series_cell_ok(cell->cm, cell->ci), std::string(who) + ": " + what);
    return SIT_OK;
}

static inline int series_lags(sit_ctx *c, const char *who, const i64 *lags, i64 n_lags, i64 F)
{
    const i64 bad = series_first_outside(lags, n_lags, 0, F - 1);
    if (bad < 0) return SIT_OK;
    char text[128];
    snprintf(text, sizeof(text), "%s: lag %lld is outside [0, %lld]", who, (long long)lags[bad], (long long)(F - 1));
    c->msg = text;
    return SIT_ERR_INVALID;
}

static inline int series_atoms_in_range(sit_ctx *c, const char *who, const i64 *list, i64 n, i64 A)
{
    const i64 bad = series_first_outside(list, n, 0, A - 1);
    if (bad < 0) return SIT_OK;
    char text[128];
    snprintf(text, sizeof(text), "%s: atom %lld is outside the %lld atoms of a frame", who, (long long)list[bad], (long long)A);
    c->msg = text;
    return SIT_ERR_INVALID;
}

// A call without a host array reads the resident frames: there are some, and - the second form - F and A are theirs
static inline int series_resident(sit_ctx *c, const char *who)
{
    SIT_REQUIRE(c, c->d_frames && c->A > 0, std::string(who) + ": no resident frames (sit_set_frames first)");
    return SIT_OK;
}

static inline int series_resident(sit_ctx *c, const char *who, i64 F, i64 A)
{
    if (const int rc = series_resident(c, who)) return rc;
    SIT_REQUIRE(c, F == c->F && A == c->A, std::string(who) + ": F or A is not that of the resident frames");
    return SIT_OK;
}

struct SeriesSource {
    const double *pos;             // [F][A][3]
    i64 A;
    const i64 *atoms;              // [n_sel] columns of a frame, or null: the columns themselves
    __device__ i64 atom(i64 c) const { return atoms ? atoms[c] : c; }
    __device__ const double *at(i64 t, i64 c) const { return pos + (t * A + atom(c)) * 3; }
};

// The source of a call: a host array goes into `upload` as it is; the resident frames need F to be theirs and an atom list
// within them, which goes into d_atoms (room for n_sel).  On the context's stream; the messages differ by `who` alone.
static inline int series_source(sit_ctx *c, const char *who, const double *positions, i64 F, const i64 *atoms, i64 n_sel, i64 *d_atoms,
                                Scoped &upload, SeriesSource *src)
{
    if (positions) {
        HIP_TRY(c, sit_dmalloc(c, &upload.p, (size_t)(F * n_sel) * 24));
        HIP_TRY(c, hipMemcpyAsync(upload.p, positions, (size_t)(F * n_sel) * 24, hipMemcpyHostToDevice, c->stream));
        *src = {(const double *)upload.p, n_sel, nullptr};
        return SIT_OK;
    }
    int rc;
    if ((rc = series_resident(c, who))) return rc;
    SIT_REQUIRE(c, F == c->F, std::string(who) + ": F is not the number of resident frames");
    SIT_REQUIRE(c, atoms, std::string(who) + ": the resident frames need an atom list");
    if ((rc = series_atoms_in_range(c, who, atoms, n_sel, c->A))) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_atoms, atoms, (size_t)n_sel * 8, hipMemcpyHostToDevice, c->stream));
    *src = {c->d_frames, c->A, d_atoms};
    return SIT_OK;
}

// The source over whole frames of A atoms and a device atom list: a host [F, A, 3] array goes into `upload` as it is, on the
// context's stream; without one the resident frames are read, which series_resident has looked at
static inline int series_frames(sit_ctx *c, const double *positions, i64 F, i64 A, const i64 *d_atoms, Scoped &upload, SeriesSource *src)
{
    *src = {c->d_frames, A, d_atoms};
    if (positions) {
        HIP_TRY(c, sit_dmalloc(c, &upload.p, (size_t)(F * A) * 24));
        HIP_TRY(c, hipMemcpyAsync(upload.p, positions, (size_t)(F * A) * 24, hipMemcpyHostToDevice, c->stream));
        src->pos = (const double *)upload.p;
    }
    return SIT_OK;
}

// out [frame][3][column] = last(s), s = x . ci (msd_frac) of columns [c0, c0 + n) of the source in frames [f0, f0 + nf): a
// thread per (frame, column), SERIES_FRAC_THREADS to a workgroup
#define SERIES_FRAC_THREADS 256
struct SeriesFracAsIs { __device__ double operator()(double s) const { return s; } };

template <class Last>
__global__ __launch_bounds__(SERIES_FRAC_THREADS) void k_series_frac(SeriesSource src, i64 c0, i64 n, i64 f0, i64 nf, MsdCell cell, double *out)
{
    const i64 i = (i64)blockIdx.x * SERIES_FRAC_THREADS + threadIdx.x;
    if (i >= nf * n) return;
    const i64 f = i / n, col = i - f * n;
    const double *p = src.at(f0 + f, c0 + col);
    const double x = p[0], y = p[1], z = p[2];
    for (int a = 0; a < 3; a++) out[(f * 3 + a) * n + col] = Last()(msd_frac(cell.ci, a, x, y, z));
}

template <class Last = SeriesFracAsIs>
static int series_frac(sit_ctx *c, const SeriesSource &src, i64 c0, i64 n, i64 f0, i64 nf, const MsdCell &cell, double *out)
{
    if (nf <= 0) return SIT_OK;
    k_series_frac<Last><<<dim3((unsigned)((nf * n + SERIES_FRAC_THREADS - 1) / SERIES_FRAC_THREADS)), dim3(SERIES_FRAC_THREADS), 0, c->stream>>>(
        src, c0, n, f0, nf, cell, out);
    HIP_TRY(c, hipGetLastError());
    return SIT_OK;
}

// One 32 x 32 tile of a batch: frames [32 blockIdx.x, +32) of nt, columns [32 blockIdx.y, +32) of the nb that start at
// column a0 of the selection; 256 threads.  load(t, column, v) gives the NV values of an element and is called with the
// atoms across lanes (neighbours in a frame); store(t, c, v) takes them with the frames across lanes (a series is written
// as one run), c counted within the batch.  The 33rd column keeps the transposed read off one bank.
template <int NV, typename T, class Load, class Store>
__device__ __forceinline__ void series_tile(i64 a0, i64 nb, i64 nt, Load load, Store store)
{
    __shared__ T tile[NV][32][33];
    const i64 t0 = (i64)blockIdx.x * 32, c0 = (i64)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    T v[NV];
    for (int r = ty; r < 32; r += 8) {
        const i64 t = t0 + r, c = c0 + tx;
        if (t < nt && c < nb) {
            load(t, a0 + c, v);
            for (int k = 0; k < NV; k++) tile[k][r][tx] = v[k];
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const i64 c = c0 + r, t = t0 + tx;
        if (t < nt && c < nb) {
            for (int k = 0; k < NV; k++) v[k] = tile[k][tx][r];
            store(t, c, v);
        }
    }
}
