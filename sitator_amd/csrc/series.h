// The front of the frame-series operators (spectrum.hip, msd.hip): where the selected atoms' positions come from, and the
// tile that turns them into per-atom series that are contiguous along the frames.  A selection is n_sel columns: column c
// of a host [F, n_sel, 3] array that is uploaded as it is (A = n_sel, no atom list), or atom atoms[c] of the frames resident
// in device memory (A = the atoms of a frame); the kernels read either through a SeriesSource.
#pragma once
#include "sit_internal.h"

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
    SIT_REQUIRE(c, c->d_frames && c->A > 0, std::string(who) + ": no resident frames (sit_set_frames first)");
    SIT_REQUIRE(c, F == c->F, std::string(who) + ": F is not the number of resident frames");
    SIT_REQUIRE(c, atoms, std::string(who) + ": the resident frames need an atom list");
    for (i64 i = 0; i < n_sel; i++)
        if (atoms[i] < 0 || atoms[i] >= c->A) {
            char text[128];
            snprintf(text, sizeof(text), "%s: atom %lld is outside the %lld atoms of a frame", who, (long long)atoms[i], (long long)c->A);
            c->msg = text;
            return SIT_ERR_INVALID;
        }
    HIP_TRY(c, hipMemcpyAsync(d_atoms, atoms, (size_t)n_sel * 8, hipMemcpyHostToDevice, c->stream));
    *src = {c->d_frames, c->A, d_atoms};
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
