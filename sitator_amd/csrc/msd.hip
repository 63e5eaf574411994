// MeanSquaredDisplacement: the tracer and the collective mean squared displacement of chosen atoms against the lag, per
// Cartesian axis, from the frames as they lie in device memory.  Every decision - the image of a step, the operation
// order of an unwrapped position, the chunks and the order of the scans, S1, the combination - is in msd_plan.h.
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

#include "sit_internal.h"
#include "msd_plan.h"

struct MsdCell { double cm[9], ci[9]; };

// shift[c][a][t] = -image of the step t-1 -> t of atom c along cell vector a (0 at t = 0).  A 32 x 32 tile: read with the
// atoms across lanes (neighbours in a frame), written with the frames across lanes (the scans read a series as one run).
__global__ __launch_bounds__(256) void k_msd_shift(const double *pos, i64 A, const i64 *atoms, i64 a0, i64 nb, i64 F, MsdCell cell,
                                                   i32 *shift, u64 *max_residual_bits)
{
    __shared__ i32 tile[3][32][33];
    __shared__ double red[256];
    const i64 t0 = (i64)blockIdx.x * 32, c0 = (i64)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double worst = 0.0;
    for (int r = ty; r < 32; r += 8) {
        const i64 t = t0 + r, c = c0 + tx;
        if (t < F && c < nb) {
            i32 n[3] = {0, 0, 0};
            if (t > 0) {
                const i64 atom = atoms ? atoms[a0 + c] : a0 + c;
                const double *p1 = pos + (t * A + atom) * 3, *p0 = p1 - A * 3;
                const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
                for (int a = 0; a < 3; a++) {
                    double res;
                    n[a] = -msd_image(msd_frac(cell.ci, a, dx, dy, dz), &res);
                    if (res > worst) worst = res;
                }
            }
            tile[0][r][tx] = n[0]; tile[1][r][tx] = n[1]; tile[2][r][tx] = n[2];
        }
    }
    red[threadIdx.x] = worst;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const i64 c = c0 + r, t = t0 + tx;
        if (t < F && c < nb)
            for (int a = 0; a < 3; a++) shift[(c * 3 + a) * F + t] = tile[a][tx][r];
    }
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

// y[c][a][t] = x_u[t] - x_u[0] (images: null with unwrap off); the tile of k_msd_shift, three coordinates deep
__global__ __launch_bounds__(256) void k_msd_series(const double *pos, i64 A, const i64 *atoms, i64 a0, i64 nb, i64 F, MsdCell cell,
                                                    const i32 *images, double *y)
{
    __shared__ double tile[3][32][33];
    __shared__ double first[3][32];
    const i64 t0 = (i64)blockIdx.x * 32, c0 = (i64)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const i64 t = t0 + r, c = c0 + tx;
        if (t < F && c < nb) {
            const i64 atom = atoms ? atoms[a0 + c] : a0 + c;
            const double *p = pos + (t * A + atom) * 3;
            tile[0][r][tx] = p[0]; tile[1][r][tx] = p[1]; tile[2][r][tx] = p[2];
            if (r == 0) { const double *q = pos + atom * 3; first[0][tx] = q[0]; first[1][tx] = q[1]; first[2][tx] = q[2]; }
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const i64 c = c0 + r, t = t0 + tx;
        if (t < F && c < nb) {
            i32 n0 = 0, n1 = 0, n2 = 0;
            if (images) { n0 = images[(c * 3) * F + t]; n1 = images[(c * 3 + 1) * F + t]; n2 = images[(c * 3 + 2) * F + t]; }
            for (int a = 0; a < 3; a++)                                      // N[0] = 0: x_u[0] is x[0]
                y[(c * 3 + a) * F + t] = msd_unwrap(tile[a][tx][r], n0, n1, n2, cell.cm, a) - first[a][r];
        }
    }
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
        for (i64 i = 0; i < n_lags; i++)
            if (lags[i] < 0 || lags[i] > F - 1) {
                char text[128];
                snprintf(text, sizeof(text), "sit_msd: lag %lld is outside [0, %lld]", (long long)lags[i], (long long)(F - 1));
                c->msg = text;
                return SIT_ERR_INVALID;
            }
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
    i64 A = n_sel;
    if (!positions) {
        SIT_REQUIRE(c, c->d_frames && c->A > 0, "sit_msd: no resident frames (sit_set_frames first)");
        SIT_REQUIRE(c, F == c->F, "sit_msd: F is not the number of resident frames");
        SIT_REQUIRE(c, atoms, "sit_msd: the resident frames need an atom list");
        A = c->A;
        for (i64 i = 0; i < n_sel; i++)
            if (atoms[i] < 0 || atoms[i] >= A) {
                char text[128];
                snprintf(text, sizeof(text), "sit_msd: atom %lld is outside the %lld atoms of a frame", (long long)atoms[i], (long long)A);
                c->msg = text;
                return SIT_ERR_INVALID;
            }
    }
    MsdCell cell;
    for (int i = 0; i < 9; i++) { cell.cm[i] = c->pbc.cm[i]; cell.ci[i] = c->pbc.ci[i]; }
    if (unwrap) {
        const double *m = cell.cm;
        const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
        bool ok = std::isfinite(det) && det != 0.0;
        for (int i = 0; i < 9; i++) ok = ok && std::isfinite(cell.ci[i]);
        SIT_REQUIRE(c, ok, "sit_msd: a degenerate cell cannot unwrap a trajectory");
    }
    MsdPlanIn in;
    in.F = F; in.n_sel = n_sel; in.n_lags = n_lags; in.direct = direct; in.collective = collective != 0; in.workspace_bytes = workspace_bytes;
    const MsdPlan pl = msd_plan(in, sp_knobs_from_env());
    if (pl.err) { c->msg = std::string("sit_msd: ") + pl.err; return SIT_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    const double2 *root = nullptr;
    if (!direct && (rc = sp_roots(c, pl.sp.M, &root))) return rc;
    const i64 B = pl.atoms_per_batch;
    // one buffer: a status word, the atom list, the lag list, then the plan's workspace
    const i64 head = 256 + msd_round256(n_sel * 8) + msd_round256(direct ? n_lags * 8 : 0);
    Scoped work(c), upload(c);
    HIP_TRY(c, sit_dmalloc(c, &work.p, (size_t)(head + pl.workspace)));
    char *w = (char *)work.p;
    u64 *d_res = (u64 *)w; w += 256;
    i64 *d_atoms = (i64 *)w; w += msd_round256(n_sel * 8);
    i64 *d_lags = (i64 *)w; w += msd_round256(direct ? n_lags * 8 : 0);
    double *d_coll_y = (double *)w; w += pl.fixed_bytes;
    double *d_y = (double *)w; w += 3 * B * pl.series_bytes;
    i32 *d_img = (i32 *)w; w += 3 * B * pl.image_bytes;
    double *d_psum = (double *)w; w += 3 * B * pl.psum_bytes;
    void *d_totals = (void *)w; w += 3 * B * pl.chunk_bytes;
    double2 *d_buf = (double2 *)w; w += direct ? 0 : 3 * B * pl.sp.M * 16;
    double *d_out = (double *)w; w += 3 * B * msd_round256(n_lags * 8);
    double *d_r4 = (double *)w;
    HIP_TRY(c, hipMemsetAsync(d_res, 0, 256, c->stream));
    const double *d_pos = c->d_frames;
    if (positions) {
        HIP_TRY(c, sit_dmalloc(c, &upload.p, (size_t)(F * n_sel) * 24));
        HIP_TRY(c, hipMemcpyAsync(upload.p, positions, (size_t)(F * n_sel) * 24, hipMemcpyHostToDevice, c->stream));
        d_pos = (const double *)upload.p;
    } else {
        HIP_TRY(c, hipMemcpyAsync(d_atoms, atoms, (size_t)n_sel * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (direct) HIP_TRY(c, hipMemcpyAsync(d_lags, lags, (size_t)n_lags * 8, hipMemcpyHostToDevice, c->stream));
    std::vector<i32> img_host(images ? (size_t)(3 * B * F) : 0);
    for (i64 a0 = 0; a0 < n_sel; a0 += B) {
        const i64 nb = a0 + B < n_sel ? B : n_sel - a0, n_series = 3 * nb;
        const dim3 tiles((unsigned)((F + 31) / 32), (unsigned)((nb + 31) / 32));
        if (unwrap) {
            k_msd_shift<<<tiles, dim3(256), 0, c->stream>>>(d_pos, A, positions ? nullptr : d_atoms, a0, nb, F, cell, d_img, d_res);
            HIP_TRY(c, hipGetLastError());
            ScanImages si; si.v = d_img; si.F = F;
            if ((rc = msd_scan(c, si, pl.n_chunks, n_series, (i32 *)d_totals))) return rc;
        }
        k_msd_series<<<tiles, dim3(256), 0, c->stream>>>(d_pos, A, positions ? nullptr : d_atoms, a0, nb, F, cell, unwrap ? d_img : nullptr, d_y);
        HIP_TRY(c, hipGetLastError());
        if (collective) {
            k_msd_collective<<<dim3((unsigned)((F + 255) / 256), 3), dim3(256), 0, c->stream>>>(d_y, nb, F, a0 == 0 ? 1 : 0, d_coll_y);
            HIP_TRY(c, hipGetLastError());
        }
        if (direct) {
            k_msd_direct<<<dim3((unsigned)n_lags, (unsigned)nb), dim3(256), 0, c->stream>>>(d_y, F, d_lags, n_lags, d_out, r4 ? d_r4 : nullptr);
            HIP_TRY(c, hipGetLastError());
            if (r4) HIP_TRY(c, hipMemcpyAsync(r4 + a0 * n_lags, d_r4, (size_t)(nb * n_lags) * 8, hipMemcpyDeviceToHost, c->stream));
        } else if ((rc = msd_all_lags(c, pl, root, d_y, d_psum, (double *)d_totals, d_buf, d_out, F, n_lags, n_series))) return rc;
        HIP_TRY(c, hipMemcpyAsync(msd + a0 * 3 * n_lags, d_out, (size_t)(n_series * n_lags) * 8, hipMemcpyDeviceToHost, c->stream));
        if (images) {
            if (unwrap) HIP_TRY(c, hipMemcpyAsync(img_host.data(), d_img, (size_t)(n_series * F) * 4, hipMemcpyDeviceToHost, c->stream));
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
            k_msd_direct<<<dim3((unsigned)n_lags, 1), dim3(256), 0, c->stream>>>(d_coll_y, F, d_lags, n_lags, d_out, nullptr);
            HIP_TRY(c, hipGetLastError());
        } else if ((rc = msd_all_lags(c, pl, root, d_coll_y, d_psum, (double *)d_totals, d_buf, d_out, F, n_lags, 3))) return rc;
        HIP_TRY(c, hipMemcpyAsync(coll, d_out, (size_t)(3 * n_lags) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (i64 i = 0; i < 3 * n_lags; i++) coll[i] /= (double)n_sel;
    }
    u64 bits = 0;
    HIP_TRY(c, hipMemcpyAsync(&bits, d_res, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (max_residual) { double v; memcpy(&v, &bits, 8); *max_residual = v; }
    return SIT_OK;
}
