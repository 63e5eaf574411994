// MeanSquaredDisplacement: the tracer and the collective mean squared displacement of chosen atoms against the lag, per
// Cartesian axis, from the frames as they lie in device memory.  Every decision - the image of a step, the operation
// order of an unwrapped position, the chunks and the order of the scans, S1, the combination, the pieces of a call's buffer
// (msd_layout) - is in msd_plan.h.  Where the selected atoms come from and the tile that k_msd_shift and k_msd_series read
// them through are in series.h, shared with spectrum.hip.
//
//   k_msd_shift      the image shift of every step and the largest distance of a step from a whole image
//   k_msd_scan_*     sums along the frames in chunks: the totals of the chunks, their exclusive sums, the apply pass
//                    (int32: the shifts become the image counts N; float64: P[k] = sum_{t<k} y[t]^2)
//   k_msd_series     y[t] = x_u[t] - x_u[0] as [atom][axis][F]; k_msd_collective adds the atoms of a batch, in order, to Y
//   all lags         msd(tau) = S1(tau) - 2 acf(tau) / (F - tau): the autocorrelation is the inverse transform of the
//                    squared modulus of the transform of y zero-padded to M >= 2 F - 1 (k_spec_pass of spectrum.hip, one
//                    transform pair per series), S1 comes from P
//   k_msd_direct     chosen lags: the sums themselves, one workgroup per (lag, atom), with the fourth moment
// An atom's arithmetic does not depend on which atoms share a launch; only the maximum of the residual is taken over all.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "series.h"
#include "spectrum_pass.h"
#include "msd_plan.h"
#include "msd_series.h"

// shift[c][a][t] = -image of the step t-1 -> t of atom c along cell vector a (0 at t = 0), through the tile of series.h
// (the scans read a series as one run), and behind it the largest residual of the steps the workgroup looked at.
__global__ __launch_bounds__(256) void k_msd_shift(SeriesSource src, i64 a0, i64 nb, i64 F, MsdCell cell, i32 *shift, u64 *max_residual_bits)
{
    __shared__ double red[256];
    double worst = 0.0;
    series_tile<3, i32>(a0, nb, F,
        [&](i64 t, i64 column, i32 *n) {
            n[0] = n[1] = n[2] = 0;
            if (t == 0) return;
            const double *p1 = src.at(t, column), *p0 = p1 - src.A * 3;
            const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
            for (int a = 0; a < 3; a++) {
                double res;
                n[a] = -msd_image(msd_frac(cell.ci, a, dx, dy, dz), &res);
                if (res > worst) worst = res;
            }
        },
        [&](i64 t, i64 c, const i32 *n) { for (int a = 0; a < 3; a++) shift[(c * 3 + a) * F + t] = n[a]; });
    red[threadIdx.x] = worst;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
        __syncthreads();
    }
    // a maximum does not depend on order; doubles that are not negative compare as their bit patterns do
    if (threadIdx.x == 0 && red[0] > 0.0) atomicMax((unsigned long long *)max_residual_bits, (unsigned long long)__double_as_longlong(red[0]));
}

// ---- the scans (msd_plan.h: chunks of MSD_CHUNK, four elements per thread, Hillis-Steele over the threads' totals) ----

struct ScanImages {                               // in place over [series][F] int32
    typedef i32 T;
    i32 *v; i64 F;
    __device__ T load(i64 series, i64 t) const { return v[series * F + t]; }
    __device__ void store(i64 series, i64 t, T s) const { v[series * F + t] = s; }
};
struct ScanSquares {                              // y [series][F] -> P [series][F + 1], P[t + 1] = the inclusive sum at t
    typedef double T;
    const double *y; double *P; i64 F;
    __device__ T load(i64 series, i64 t) const { const double q = y[series * F + t]; return q * q; }
    __device__ void store(i64 series, i64 t, T s) const { P[series * (F + 1) + t + 1] = s; }
};

// the elements of thread `tid` of chunk `chunk`: local[i] = their running sum; lds[0 .. MSD_THREADS) ends up holding the
// inclusive scan of the threads' totals
template <class Op> __device__ __forceinline__ void msd_chunk_scan(const Op &op, i64 series, i64 chunk, typename Op::T *local, typename Op::T *lds)
{
    typedef typename Op::T T;
    const int tid = threadIdx.x;
    const i64 e0 = chunk * MSD_CHUNK + (i64)tid * MSD_GROUP;
    T run = (T)0;
    for (int i = 0; i < MSD_GROUP; i++) {
        const T v = e0 + i < op.F ? op.load(series, e0 + i) : (T)0;
        run = i == 0 ? v : run + v;
        local[i] = run;
    }
    lds[tid] = run;
    __syncthreads();
    for (int d = 1; d < MSD_THREADS; d <<= 1) {
        const T mine = lds[tid], before = tid >= d ? lds[tid - d] : (T)0;
        __syncthreads();
        if (tid >= d) lds[tid] = before + mine;
        __syncthreads();
    }
}

template <class Op> __global__ __launch_bounds__(MSD_THREADS) void k_msd_scan_totals(Op op, i64 n_chunks, typename Op::T *totals)
{
    typedef typename Op::T T;
    __shared__ T lds[MSD_THREADS];
    T local[MSD_GROUP];
    const i64 chunk = blockIdx.x, series = blockIdx.y;
    msd_chunk_scan(op, series, chunk, local, lds);
    if (threadIdx.x == 0) totals[series * n_chunks + chunk] = lds[MSD_THREADS - 1];
}

// the chunk totals of a series, one after the other, in place: totals[c] <- the sum of the chunks before c
template <typename T> __global__ void k_msd_scan_offsets(T *totals, i64 n_chunks, i64 n_series)
{
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_series) return;
    T *row = totals + s * n_chunks;
    T run = (T)0;
    for (i64 c = 0; c < n_chunks; c++) { const T v = row[c]; row[c] = run; run = c == 0 ? v : run + v; }
}

template <class Op> __global__ __launch_bounds__(MSD_THREADS) void k_msd_scan_apply(Op op, i64 n_chunks, const typename Op::T *offsets)
{
    typedef typename Op::T T;
    __shared__ T lds[MSD_THREADS];
    T local[MSD_GROUP];
    const i64 chunk = blockIdx.x, series = blockIdx.y;
    const int tid = threadIdx.x;
    msd_chunk_scan(op, series, chunk, local, lds);
    const T before = tid > 0 ? lds[tid - 1] : (T)0, offset = offsets[series * n_chunks + chunk];
    const i64 e0 = chunk * MSD_CHUNK + (i64)tid * MSD_GROUP;
    for (int i = 0; i < MSD_GROUP; i++)
        if (e0 + i < op.F) op.store(series, e0 + i, msd_scan_value(offset, before, local[i]));
}

template <typename T> __global__ void k_msd_zero_first(T *P, i64 stride, i64 n_series)
{
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_series) P[s * stride] = (T)0;
}

// y[c][a][t] = x_u[t] - x_u[0] (images: null with unwrap off); the same tile, three coordinates deep.  `first`: x[0] of
// the tile's 32 columns, left by whoever loads the tile's first frame.
__global__ __launch_bounds__(256) void k_msd_series(SeriesSource src, i64 a0, i64 nb, i64 F, MsdCell cell, const i32 *images, double *y)
{
    __shared__ double first[3][32];
    series_tile<3, double>(a0, nb, F,
        [&](i64 t, i64 column, double *x) {
            const double *p = src.at(t, column);
            x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
            if (t == (i64)blockIdx.x * 32) { const double *q = src.at(0, column); for (int a = 0; a < 3; a++) first[a][threadIdx.x & 31] = q[a]; }
        },
        [&](i64 t, i64 c, const double *x) {
            i32 n0 = 0, n1 = 0, n2 = 0;
            if (images) { n0 = images[(c * 3) * F + t]; n1 = images[(c * 3 + 1) * F + t]; n2 = images[(c * 3 + 2) * F + t]; }
            for (int a = 0; a < 3; a++)                                      // N[0] = 0: x_u[0] is x[0]
                y[(c * 3 + a) * F + t] = msd_unwrap(x[a], n0, n1, n2, cell.cm, a) - first[a][c & 31];
        });
}

// Y[a][t] (+)= y of the nb atoms of the batch, one after the other; the first atom of the selection starts the sum
__global__ void k_msd_collective(const double *y, i64 nb, i64 F, int start, double *Y)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y;
    if (t >= F) return;
    double s = start ? y[(i64)a * F + t] : Y[(i64)a * F + t];
    for (i64 c = start ? 1 : 0; c < nb; c++) s += y[(c * 3 + a) * F + t];
    Y[(i64)a * F + t] = s;
}

// One workgroup per (lag, atom): every thread sums dx^2, dy^2, dz^2 and (|d|^2)^2 over its t in index order, a fixed
// tree over the workgroup, one division.  out[c][a][l], r4[c][l] (null: not wanted).
__global__ __launch_bounds__(256) void k_msd_direct(const double *y, i64 F, const i64 *lags, i64 n_lags, double *out, double *r4)
{
    __shared__ double red[4][256];
    const i64 l = blockIdx.x, c = blockIdx.y, lag = lags[l], count = F - lag;
    const int tid = threadIdx.x;
    const double *yx = y + (c * 3) * F, *yy = yx + F, *yz = yy + F;
    double sx = 0.0, sy = 0.0, sz = 0.0, s4 = 0.0;
    for (i64 t = tid; t < count; t += 256) {
        const double dx = yx[t + lag] - yx[t], dy = yy[t + lag] - yy[t], dz = yz[t + lag] - yz[t];
        const double xx = dx * dx, yy2 = dy * dy, zz = dz * dz, q = (xx + yy2) + zz;
        sx += xx; sy += yy2; sz += zz; s4 += q * q;
    }
    red[0][tid] = sx; red[1][tid] = sy; red[2][tid] = sz; red[3][tid] = s4;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 4; k++) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
    if (tid < 3) out[(c * 3 + tid) * n_lags + l] = lag == 0 ? 0.0 : red[tid][0] / (double)count;
    if (tid == 3 && r4) r4[c * n_lags + l] = lag == 0 ? 0.0 : red[3][0] / (double)count;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

template <class Op> static int msd_scan(sit_ctx *c, Op op, i64 n_chunks, i64 n_series, typename Op::T *totals)
{
    typedef typename Op::T T;
    k_msd_scan_totals<Op><<<dim3((unsigned)n_chunks, (unsigned)n_series), dim3(MSD_THREADS), 0, c->stream>>>(op, n_chunks, totals);
    HIP_TRY(c, hipGetLastError());
    k_msd_scan_offsets<T><<<dim3((unsigned)((n_series + 63) / 64)), dim3(64), 0, c->stream>>>(totals, n_chunks, n_series);
    HIP_TRY(c, hipGetLastError());
    k_msd_scan_apply<Op><<<dim3((unsigned)n_chunks, (unsigned)n_series), dim3(MSD_THREADS), 0, c->stream>>>(op, n_chunks, totals);
    HIP_TRY(c, hipGetLastError());
    return SIT_OK;
}

int msd_series_launch(sit_ctx *c, const SeriesSource &src, i64 a0, i64 nb, i64 F, const MsdCell &cell, bool unwrap, i64 n_chunks,
                      i32 *images, void *totals, double *y, u64 *status)
{
    const dim3 tiles((unsigned)((F + 31) / 32), (unsigned)((nb + 31) / 32));
    if (unwrap) {
        k_msd_shift<<<tiles, dim3(256), 0, c->stream>>>(src, a0, nb, F, cell, images, status);
        HIP_TRY(c, hipGetLastError());
        ScanImages si; si.v = images; si.F = F;
        if (const int rc = msd_scan(c, si, n_chunks, 3 * nb, (i32 *)totals)) return rc;
    }
    k_msd_series<<<tiles, dim3(256), 0, c->stream>>>(src, a0, nb, F, cell, unwrap ? images : nullptr, y);
    HIP_TRY(c, hipGetLastError());
    return SIT_OK;
}

// msd of n_series series y [n_series][F] at the lags 0 .. n_lags - 1 into d_out [n_series][n_lags]
static int msd_all_lags(sit_ctx *c, const MsdPlan &pl, const double2 *root, const double *d_y, double *d_psum, double *d_totals,
                        double2 *d_buf, double *d_out, i64 F, i64 n_lags, i64 n_series)
{
    int rc;
    k_msd_zero_first<double><<<dim3((unsigned)((n_series + 63) / 64)), dim3(64), 0, c->stream>>>(d_psum, F + 1, n_series);
    HIP_TRY(c, hipGetLastError());
    ScanSquares sq; sq.y = d_y; sq.P = d_psum; sq.F = F;
    if ((rc = msd_scan(c, sq, pl.n_chunks, n_series, d_totals))) return rc;
    SpArgs a = SpArgs();
    a.buf = d_buf; a.speeds = d_y; a.root = root; a.psum = d_psum; a.msd = d_out; a.n = F; a.M = pl.sp.M; a.nbins = n_lags;
    a.inv_m = 1.0 / (double)pl.sp.M;
    const int p = pl.sp.npass;
    for (int i = 0; i < p - 1; i++)
        if ((rc = sp_launch(c, pl.sp, i, a, i == 0 ? SP_LOAD_REAL : SP_LOAD_PLAIN, SP_MID_FWD, SP_STORE_TWIDDLE, n_series))) return rc;
    if ((rc = sp_launch(c, pl.sp, p - 1, a, p == 1 ? SP_LOAD_REAL : SP_LOAD_PLAIN, SP_MID_POWER, p == 1 ? SP_STORE_MSD : SP_STORE_PLAIN, n_series)))
        return rc;
    for (int i = p - 2; i >= 0; i--)
        if ((rc = sp_launch(c, pl.sp, i, a, SP_LOAD_UNTWIDDLE, SP_MID_INV, i == 0 ? SP_STORE_MSD : SP_STORE_PLAIN, n_series))) return rc;
    return SIT_OK;
}

extern "C" int sit_msd(sit_ctx *c, const double *positions, i64 F, const i64 *atoms, i64 n_sel, int unwrap, i64 max_lag,
                       const i64 *lags, i64 n_lags, int collective, i64 workspace_bytes, double *msd, double *r4, double *coll,
                       i32 *images, double *max_residual)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, F >= 2, "sit_msd: at least two frames needed");
    SIT_REQUIRE(c, F <= MSD_MAX_F, "sit_msd: more than 2^29 frames");
    SIT_REQUIRE(c, n_sel >= 0 && workspace_bytes >= 0, "sit_msd: negative count");
    const bool direct = lags != nullptr;
    if (direct) {
        SIT_REQUIRE(c, n_lags >= 1, "sit_msd: an empty lag list");
        if (const int rc = series_lags(c, "sit_msd", lags, n_lags, F)) return rc;
    } else {
        SIT_REQUIRE(c, max_lag >= 0 && max_lag <= F - 1, "sit_msd: max_lag is outside [0, F - 1]");
        SIT_REQUIRE(c, !r4, "sit_msd: the fourth moment comes with an explicit lag list only");
        n_lags = max_lag + 1;
    }
    SIT_REQUIRE(c, !coll || collective, "sit_msd: coll without collective");
    SIT_REQUIRE(c, !collective || coll, "sit_msd: collective without coll");
    if (max_residual) *max_residual = 0.0;
    if (n_sel == 0) return SIT_OK;
    SIT_REQUIRE(c, msd, "sit_msd: missing array");
    int rc;
    MsdCell cell;
    if ((rc = series_cell(c, "sit_msd", &cell, unwrap ? "a degenerate cell cannot unwrap a trajectory" : nullptr))) return rc;
    MsdPlanIn in;
    in.F = F; in.n_sel = n_sel; in.n_lags = n_lags; in.direct = direct; in.collective = collective != 0; in.workspace_bytes = workspace_bytes;
    const MsdPlan pl = msd_plan(in, sp_knobs_from_env());
    if (pl.err) { c->msg = std::string("sit_msd: ") + pl.err; return SIT_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    const double2 *root = nullptr;
    if (!direct && (rc = sp_roots(c, pl.sp.M, &root))) return rc;
    const i64 B = pl.atoms_per_batch;
    Scoped work(c), upload(c);
    MsdPieces w;
    if ((rc = carve_scratch(c, [&](Carve &cv) { w = msd_layout(cv, pl, in, B); }, &work))) return rc;
    HIP_TRY(c, hipMemsetAsync(w.status, 0, 8, c->stream));
    SeriesSource src;
    if ((rc = series_source(c, "sit_msd", positions, F, atoms, n_sel, w.atoms, upload, &src))) return rc;
    if (direct) HIP_TRY(c, hipMemcpyAsync(w.lags, lags, (size_t)n_lags * 8, hipMemcpyHostToDevice, c->stream));
    std::vector<i32> img_host(images ? (size_t)(3 * B * F) : 0);
    for (i64 a0 = 0; a0 < n_sel; a0 += B) {
        const i64 nb = a0 + B < n_sel ? B : n_sel - a0, n_series = 3 * nb;
        if ((rc = msd_series_launch(c, src, a0, nb, F, cell, unwrap != 0, pl.n_chunks, w.images, w.totals, w.y, w.status))) return rc;
        if (collective) {
            k_msd_collective<<<dim3((unsigned)((F + 255) / 256), 3), dim3(256), 0, c->stream>>>(w.y, nb, F, a0 == 0 ? 1 : 0, w.coll_y);
            HIP_TRY(c, hipGetLastError());
        }
        if (direct) {
            k_msd_direct<<<dim3((unsigned)n_lags, (unsigned)nb), dim3(256), 0, c->stream>>>(w.y, F, w.lags, n_lags, w.out, r4 ? w.r4 : nullptr);
            HIP_TRY(c, hipGetLastError());
            if (r4) HIP_TRY(c, hipMemcpyAsync(r4 + a0 * n_lags, w.r4, (size_t)(nb * n_lags) * 8, hipMemcpyDeviceToHost, c->stream));
        } else if ((rc = msd_all_lags(c, pl, root, w.y, w.psum, (double *)w.totals, (double2 *)w.buf, w.out, F, n_lags, n_series))) return rc;
        HIP_TRY(c, hipMemcpyAsync(msd + a0 * 3 * n_lags, w.out, (size_t)(n_series * n_lags) * 8, hipMemcpyDeviceToHost, c->stream));
        if (images) {
            if (unwrap) HIP_TRY(c, hipMemcpyAsync(img_host.data(), w.images, (size_t)(n_series * F) * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (i64 i = 0; i < nb; i++)
                for (i64 t = 0; t < F; t++)
                    for (int a = 0; a < 3; a++)
                        images[((a0 + i) * F + t) * 3 + a] = unwrap ? img_host[(size_t)((i * 3 + a) * F + t)] : 0;
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (collective) {
        // the three series of Y through the same kernels, in the first atom's place of the workspace
        if (direct) {
            k_msd_direct<<<dim3((unsigned)n_lags, 1), dim3(256), 0, c->stream>>>(w.coll_y, F, w.lags, n_lags, w.out, nullptr);
            HIP_TRY(c, hipGetLastError());
        } else if ((rc = msd_all_lags(c, pl, root, w.coll_y, w.psum, (double *)w.totals, (double2 *)w.buf, w.out, F, n_lags, 3))) return rc;
        HIP_TRY(c, hipMemcpyAsync(coll, w.out, (size_t)(3 * n_lags) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (i64 i = 0; i < 3 * n_lags; i++) coll[i] /= (double)n_sel;
    }
    u64 bits = 0;
    HIP_TRY(c, hipMemcpyAsync(&bits, w.status, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (max_residual) { double v; memcpy(&v, &bits, 8); *max_residual = v; }
    return SIT_OK;
}
