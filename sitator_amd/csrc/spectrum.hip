// AverageVibrationalFrequency (dynamics/AverageVibrationalFrequency.py:30-61): the power spectrum of every selected atom's
// speed |x(t+1) - x(t)| and the power-weighted mean frequency over a band, on the device.
//
// The transform length n = frames - 1 is arbitrary, so the DFT is Bluestein's: with the chirp w_j = exp(-i pi j^2 / n)
//     X_k = w_k  sum_j (s_j w_j) conj(w_{k-j}),
// a circular convolution of length M = 2^m >= 2n - 1 - a forward transform of a_j = s_j w_j (zero-padded), a product with
// the transformed filter B, an inverse transform.  spectrum_plan.h factors M = L_1 ... L_p (p <= 3, L_i <= 1024); pass i
// transforms, in LDS, the L_i points that lie S_i = L_{i+1} ... L_p apart inside every block of L_i S_i points, and the
// four-step twiddle W_{L_i S_i}^{s k} goes with it.  Forward passes are radix-2 decimation in frequency, in place, and leave
// a line in bit-reversed order; inverse passes are the stage-by-stage inverses (decimation in time), run from the last
// level to the first, and take exactly that order back to the natural one.  Nothing is ever permuted: B is made by the same
// forward passes, so it lies in the same order as the transformed a, and a product does not care.
//
// One kernel, k_spec_pass, is every pass; what it fuses is chosen per launch:
//   load   plain | speeds x chirp with the zero padding (first forward pass) | conj twiddle (inverse passes)
//   middle forward | inverse | forward, x B, inverse (the last level: its lines are transformed there and back in one go)
//   store  plain | twiddle (forward passes) | x w_k / M, re^2 + im^2, the band sums (last inverse pass)
// and, for the autocorrelation of a real series (msd.hip; the existing values keep their numbers and their code):
//   load   a real series with the zero padding | middle forward, re^2 + im^2, inverse | store S1 - 2 re / (M (F - lag))
// M <= 2^10: one launch per batch of atoms; M <= 2^20: three; M <= 2^30: five.  Every atom's transform is its own - an
// atom's arithmetic does not depend on which atoms share a launch - and the band sums are reduced in a fixed order:
// per thread in index order, a tree over the workgroup, the workgroups of an atom one after the other.
//
// Where the selected atoms come from and the tile that makes their speeds are in series.h (shared with msd.hip), the pieces
// of a call's buffer in sp_layout (spectrum_plan.h), what msd.hip needs of the pass kernel in spectrum_pass.h.
#include <cmath>

#include "series.h"
#include "spectrum_pass.h"
#include "msd_plan.h"

// speeds[c][t] = |x[t+1][atom_c] - x[t][atom_c]| for the atoms [a0, a0 + nb) of the selection, in the reference's
// operation order (a plain difference, sqrt((dx^2 + dy^2) + dz^2)), through the tile of series.h (the transform reads an
// atom's speeds as one run).
__global__ __launch_bounds__(256) void k_spec_speeds(SeriesSource src, i64 a0, i64 nb, i64 n, double *speeds)
{
    series_tile<1, double>(a0, nb, n,
        [&](i64 t, i64 column, double *v) {
            const double *p0 = src.at(t, column), *p1 = p0 + src.A * 3;
            const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
            v[0] = sqrt((dx * dx + dy * dy) + dz * dz);
        },
        [&](i64 t, i64 c, const double *v) { speeds[c * n + t] = v[0]; });
}

__device__ __forceinline__ i64 sp_bitrev(i64 l, int bits) { return bits ? (i64)(__brev((unsigned)l) >> (32 - bits)) : 0; }

__global__ __launch_bounds__(SP_THREADS) void k_spec_pass(SpArgs a)
{
    extern __shared__ double sp_lds[];
    const int tid = threadIdx.x, T = a.lines, bits = a.bits;
    const i64 L = a.L, LP = L + a.pad, half = L >> 1;
    double *re = sp_lds, *im = re + T * LP, *twr = im + T * LP, *twi = twr + (half > 0 ? half : 1), *red = twi + (half > 0 ? half : 1);
    const i64 atom = blockIdx.y, q0 = (i64)blockIdx.x * T;
    double2 *buf = a.buf + atom * a.M;
    const bool tfast = a.S >= T;                      // the T lines are adjacent columns: a row of the tile is one run
    const i64 points = (i64)T * L;
    const i64 tw_step = a.M >> (bits + a.log_s);      // root index of W_{L S}^1

    for (i64 e = tid; e < half; e += SP_THREADS) {    // W_L^e
        const double2 w = a.root[e * (a.M >> bits)];
        twr[e] = w.x; twi[e] = w.y;
    }
    for (i64 idx = tid; idx < points; idx += SP_THREADS) {
        int t; i64 l;
        if (tfast) { t = (int)(idx & (T - 1)); l = idx >> a.log_lines; } else { l = idx & (L - 1); t = (int)(idx >> bits); }
        const i64 q = q0 + t, blk = q >> a.log_s, s = q & (a.S - 1);
        const i64 g = ((blk << bits) + l) * a.S + s;
        double xr = 0.0, xi = 0.0;
        if (a.load == SP_LOAD_FIRST) {
            if (g < a.n) {
                const double sp = a.speeds[atom * a.n + g];
                const double2 c = a.chirp[g];
                xr = sp * c.x; xi = sp * c.y;
            }
        } else if (a.load == SP_LOAD_REAL) {                                // a real series, zero-padded to M
            if (g < a.n) xr = a.speeds[atom * a.n + g];
        } else {
            const double2 v = buf[g];
            xr = v.x; xi = v.y;
            if (a.load == SP_LOAD_UNTWIDDLE && a.S > 1) {                   // x conj(W_{L S}^{s k}), k = bitrev(l)
                const double2 w = a.root[s * sp_bitrev(l, bits) * tw_step];
                const double yr = xr * w.x + xi * w.y, yi = xi * w.x - xr * w.y;
                xr = yr; xi = yi;
            }
        }
        re[t * LP + l] = xr; im[t * LP + l] = xi;
    }
    __syncthreads();

    const i64 flies = (i64)T * half;
    if (a.mid & SP_MID_FWD) {
        for (int st = bits - 1; st >= 0; st--) {                             // decimation in frequency, h = 2^st
            const i64 h = (i64)1 << st;
            for (i64 idx = tid; idx < flies; idx += SP_THREADS) {
                const i64 t = idx >> (bits - 1), b = idx & (half - 1), p = b & (h - 1);
                const i64 i = t * LP + ((b >> st) << (st + 1)) + p, j = i + h, e = p << (bits - 1 - st);
                const double ar = re[i], ai = im[i], br = re[j], bi = im[j], wr = twr[e], wi = twi[e];
                const double dr = ar - br, di = ai - bi;
                re[i] = ar + br; im[i] = ai + bi;
                re[j] = dr * wr - di * wi; im[j] = dr * wi + di * wr;
            }
            __syncthreads();
        }
    }
    if (a.mid == SP_MID_CONV) {
        for (i64 idx = tid; idx < points; idx += SP_THREADS) {
            int t; i64 l;
            if (tfast) { t = (int)(idx & (T - 1)); l = idx >> a.log_lines; } else { l = idx & (L - 1); t = (int)(idx >> bits); }
            const i64 q = q0 + t, blk = q >> a.log_s, s = q & (a.S - 1);
            const double2 f = a.filter[((blk << bits) + l) * a.S + s];
            const i64 o = t * LP + l;
            const double xr = re[o], xi = im[o];
            re[o] = xr * f.x - xi * f.y; im[o] = xr * f.y + xi * f.x;
        }
        __syncthreads();
    }
    if (a.mid == SP_MID_POWER) {                                             // |X|^2: the transform of the autocorrelation
        for (i64 idx = tid; idx < points; idx += SP_THREADS) {
            int t; i64 l;
            if (tfast) { t = (int)(idx & (T - 1)); l = idx >> a.log_lines; } else { l = idx & (L - 1); t = (int)(idx >> bits); }
            const i64 o = t * LP + l;
            const double xr = re[o], xi = im[o];
            re[o] = xr * xr + xi * xi; im[o] = 0.0;
        }
        __syncthreads();
    }
    if (a.mid & SP_MID_INV) {
        for (int st = 0; st < bits; st++) {                                  // the inverse of every stage above, last one first
            const i64 h = (i64)1 << st;
            for (i64 idx = tid; idx < flies; idx += SP_THREADS) {
                const i64 t = idx >> (bits - 1), b = idx & (half - 1), p = b & (h - 1);
                const i64 i = t * LP + ((b >> st) << (st + 1)) + p, j = i + h, e = p << (bits - 1 - st);
                const double ar = re[i], ai = im[i], br = re[j], bi = im[j], wr = twr[e], wi = twi[e];
                const double cr = br * wr + bi * wi, ci = bi * wr - br * wi;
                re[i] = ar + cr; im[i] = ai + ci;
                re[j] = ar - cr; im[j] = ai - ci;
            }
            __syncthreads();
        }
    }

    double num = 0.0, den = 0.0;
    for (i64 idx = tid; idx < points; idx += SP_THREADS) {
        int t; i64 l;
        if (tfast) { t = (int)(idx & (T - 1)); l = idx >> a.log_lines; } else { l = idx & (L - 1); t = (int)(idx >> bits); }
        const i64 q = q0 + t, blk = q >> a.log_s, s = q & (a.S - 1);
        const i64 g = ((blk << bits) + l) * a.S + s;
        double xr = re[t * LP + l], xi = im[t * LP + l];
        if (a.store == SP_STORE_BAND) {
            // the first level: g is the bin.  X_k = w_k conv_k / M (the stage-by-stage inverses leave a factor M, a power of two)
            if (g < a.nbins) {
                const double2 c = a.chirp[g];
                xr *= a.inv_m; xi *= a.inv_m;
                const double yr = xr * c.x - xi * c.y, yi = xr * c.y + xi * c.x;
                if (a.spec) a.spec[atom * a.nbins + g] = make_double2(yr, yi);
                if (a.fmask[g]) {
                    const double pw = yr * yr + yi * yi;
                    num += a.freqs[g] * pw; den += pw;
                }
            }
        } else if (a.store == SP_STORE_MSD) {
            // the first level: g is the lag.  `re` is M times the autocorrelation of the series (msd_plan.h)
            if (g < a.nbins) a.msd[atom * a.nbins + g] = msd_combine(msd_s1(a.psum + atom * (a.n + 1), a.n, g), xr, a.inv_m, a.n, g);
        } else {
            if (a.store == SP_STORE_TWIDDLE && a.S > 1) {                    // x W_{L S}^{s k}, k = bitrev(l)
                const double2 w = a.root[s * sp_bitrev(l, bits) * tw_step];
                const double yr = xr * w.x - xi * w.y, yi = xr * w.y + xi * w.x;
                xr = yr; xi = yi;
            }
            buf[g] = make_double2(xr, xi);
        }
    }
    if (a.store == SP_STORE_BAND) {
        red[tid] = num; red[SP_THREADS + tid] = den;
        __syncthreads();
        for (int s = SP_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) { red[tid] += red[tid + s]; red[SP_THREADS + tid] += red[SP_THREADS + tid + s]; }
            __syncthreads();
        }
        if (tid == 0) {
            double *o = a.partial + (atom * a.tiles + blockIdx.x) * 2;
            o[0] = red[0]; o[1] = red[SP_THREADS];
        }
    }
}

// the workgroups' band sums of an atom, one after the other; result[atom] = {num / den, den}
__global__ void k_spec_finish(const double *partial, i64 tiles, i64 nb, double *result)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nb) return;
    double num = 0.0, den = 0.0;
    for (i64 w = 0; w < tiles; w++) { num += partial[(c * tiles + w) * 2]; den += partial[(c * tiles + w) * 2 + 1]; }
    result[2 * c] = num / den; result[2 * c + 1] = den;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

// What a context keeps between calls: the chirp and the transformed filter of the last transform length, and the one
// table of M-th roots of unity that every pass reads (sp_roots).  The buffers of a call are pool buffers of that call.
struct SpState {
    i64 n = 0;                                  // the length chirp and filter were made for (0: none)
    double2 *chirp = nullptr, *filter = nullptr;
    i64 roots_m = 0;                            // the M the roots were made for (0: none)
    double2 *roots = nullptr;
};

void spectrum_free(sit_ctx *c)
{
    SpState *st = (SpState *)c->spectrum;
    if (!st) return;
    for (void *p : {(void *)st->chirp, (void *)st->filter, (void *)st->roots}) if (p) sit_dfree(c, p);
    delete st;
    c->spectrum = nullptr;
}

static int sp_log2(i64 v) { int b = 0; while (((i64)1 << b) < v) b++; return b; }

int sp_launch(sit_ctx *c, const SpPlan &pl, int level, SpArgs a, int load, int mid, int store, i64 nb)
{
    const SpPass &q = pl.pass[level];
    a.L = q.L; a.S = q.S; a.bits = q.bits; a.log_s = sp_log2(q.S); a.lines = q.lines; a.log_lines = sp_log2(q.lines);
    a.pad = q.pad; a.tiles = q.tiles; a.load = load; a.mid = mid; a.store = store;
    HIP_TRY(c, lds_limit((const void *)k_spec_pass, q.lds, c->device));
    k_spec_pass<<<dim3((unsigned)q.tiles, (unsigned)nb), dim3(SP_THREADS), q.lds, c->stream>>>(a);
    HIP_TRY(c, hipGetLastError());
    return SIT_OK;
}

// The M-th roots of unity that every pass reads, the spectrum's and the autocorrelation's of msd.hip: one table,
// tab[e] = exp(-2 pi i e / M) in extended precision and rounded once, kept with the context until another M is asked for -
// so whoever launches a pass asks for it first, on every call.
int sp_roots(sit_ctx *c, i64 M, const double2 **root)
{
    if (!c->spectrum) c->spectrum = new SpState();
    SpState *st = (SpState *)c->spectrum;
    if (st->roots_m != M) {
        st->roots_m = 0;
        int rc;
        if ((rc = dev_alloc(c, &st->roots, M))) return rc;
        const long double pi = 3.141592653589793238462643383279502884L;
        std::vector<double2> tab((size_t)M);
        for (i64 e = 0; e < M; e++) {
            const long double ph = 2.0L * pi * ((long double)e / (long double)M);
            tab[(size_t)e] = make_double2((double)cosl(ph), (double)-sinl(ph));
        }
        HIP_TRY(c, hipMemcpyAsync(st->roots, tab.data(), (size_t)M * 16, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        st->roots_m = M;
    }
    *root = st->roots;
    return SIT_OK;
}

// The tables of length n, made on the host in extended precision and rounded once: the chirp with its phase reduced in
// integers (j^2 mod 2n; j^2 pi / n in floating point is already 1e-11 off at j = 1e5) and the filter conj(w_j) wrapped
// round M, which the forward passes then transform where it lies, with the roots of sp_roots.
static int sp_tables(sit_ctx *c, SpState *st, const SpPlan &pl, i64 n, const double2 *root)
{
    if (st->n == n) return SIT_OK;
    st->n = 0;
    const i64 M = pl.M;
    int rc;
    if ((rc = dev_alloc(c, &st->chirp, n)) || (rc = dev_alloc(c, &st->filter, M))) return rc;
    const long double pi = 3.141592653589793238462643383279502884L;
    std::vector<double2> chirp((size_t)n), tab((size_t)M, make_double2(0.0, 0.0));
    for (i64 j = 0; j < n; j++) {
        const u64 r = ((u64)j * (u64)j) % (u64)(2 * n);
        const long double ph = pi * (long double)r / (long double)n;
        chirp[(size_t)j] = make_double2((double)cosl(ph), (double)-sinl(ph));
    }
    HIP_TRY(c, hipMemcpyAsync(st->chirp, chirp.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    for (i64 j = 0; j < n; j++) {
        const double2 b = make_double2(chirp[(size_t)j].x, -chirp[(size_t)j].y);
        tab[(size_t)j] = b;
        if (j > 0) tab[(size_t)(M - j)] = b;
    }
    HIP_TRY(c, hipMemcpyAsync(st->filter, tab.data(), (size_t)M * 16, hipMemcpyHostToDevice, c->stream));
    SpArgs a = SpArgs();
    a.buf = st->filter; a.root = root; a.n = n; a.M = M; a.nbins = pl.nbins;
    for (int i = 0; i < pl.npass; i++)
        if ((rc = sp_launch(c, pl, i, a, SP_LOAD_PLAIN, SP_MID_FWD, SP_STORE_TWIDDLE, 1))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    st->n = n;
    return SIT_OK;
}

extern "C" int sit_speed_spectrum(sit_ctx *c, const double *positions, i64 F, const i64 *atoms, i64 n_sel, const double *freqs,
                                  const unsigned char *fmask, i64 workspace_bytes, double *avg, double *band_power,
                                  double *spectrum, double *speeds)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, F >= 2, "sit_speed_spectrum: at least two frames needed");
    SIT_REQUIRE(c, F - 1 <= SP_MAX_N, "sit_speed_spectrum: more than 2^29 + 1 frames");
    SIT_REQUIRE(c, n_sel >= 0 && workspace_bytes >= 0, "sit_speed_spectrum: negative count");
    if (n_sel == 0) return SIT_OK;
    SIT_REQUIRE(c, freqs && fmask && avg && band_power, "sit_speed_spectrum: missing array");
    const i64 n = F - 1;
    SpPlanIn in;
    in.n = n; in.n_sel = n_sel; in.workspace_bytes = workspace_bytes; in.want_spectrum = spectrum != nullptr;
    const SpPlan pl = sp_plan(in, sp_knobs_from_env());
    if (pl.err) { c->msg = std::string("sit_speed_spectrum: ") + pl.err; return SIT_ERR_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    const double2 *root = nullptr;
    if ((rc = sp_roots(c, pl.M, &root))) return rc;
    SpState *st = (SpState *)c->spectrum;                                    // sp_roots made it
    if ((rc = sp_tables(c, st, pl, n, root))) return rc;
    const i64 nbins = pl.nbins, B = pl.atoms_per_batch, tiles = pl.pass[0].tiles;
    Scoped work(c), upload(c);
    SpPieces w;
    if ((rc = carve_scratch(c, [&](Carve &cv) { w = sp_layout(cv, pl, in, B); }, &work))) return rc;
    HIP_TRY(c, hipMemcpyAsync(w.freqs, freqs, (size_t)nbins * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.fmask, fmask, (size_t)nbins, hipMemcpyHostToDevice, c->stream));
    SeriesSource src;
    if ((rc = series_source(c, "sit_speed_spectrum", positions, F, atoms, n_sel, w.atoms, upload, &src))) return rc;
    std::vector<double> result((size_t)(2 * B));
    SpArgs a = SpArgs();
    a.buf = (double2 *)w.buf; a.speeds = w.speeds; a.chirp = st->chirp; a.root = root; a.filter = st->filter; a.freqs = w.freqs;
    a.fmask = w.fmask; a.partial = w.partial; a.spec = (double2 *)w.spec; a.n = n; a.M = pl.M; a.nbins = nbins; a.inv_m = 1.0 / (double)pl.M;
    const int p = pl.npass;
    for (i64 a0 = 0; a0 < n_sel; a0 += B) {
        const i64 nb = a0 + B < n_sel ? B : n_sel - a0;
        k_spec_speeds<<<dim3((unsigned)((n + 31) / 32), (unsigned)((nb + 31) / 32)), dim3(256), 0, c->stream>>>(src, a0, nb, n, w.speeds);
        HIP_TRY(c, hipGetLastError());
        for (int i = 0; i < p - 1; i++)
            if ((rc = sp_launch(c, pl, i, a, i == 0 ? SP_LOAD_FIRST : SP_LOAD_PLAIN, SP_MID_FWD, SP_STORE_TWIDDLE, nb))) return rc;
        if ((rc = sp_launch(c, pl, p - 1, a, p == 1 ? SP_LOAD_FIRST : SP_LOAD_PLAIN, SP_MID_CONV, p == 1 ? SP_STORE_BAND : SP_STORE_PLAIN, nb)))
            return rc;
        for (int i = p - 2; i >= 0; i--)
            if ((rc = sp_launch(c, pl, i, a, SP_LOAD_UNTWIDDLE, SP_MID_INV, i == 0 ? SP_STORE_BAND : SP_STORE_PLAIN, nb))) return rc;
        k_spec_finish<<<dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, c->stream>>>(w.partial, tiles, nb, w.result);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(result.data(), w.result, (size_t)nb * 16, hipMemcpyDeviceToHost, c->stream));
        if (spectrum) HIP_TRY(c, hipMemcpyAsync(spectrum + a0 * nbins * 2, w.spec, (size_t)(nb * nbins) * 16, hipMemcpyDeviceToHost, c->stream));
        if (speeds) HIP_TRY(c, hipMemcpyAsync(speeds + a0 * n, w.speeds, (size_t)(nb * n) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (i64 i = 0; i < nb; i++) { avg[a0 + i] = result[(size_t)(2 * i)]; band_power[a0 + i] = result[(size_t)(2 * i + 1)]; }
    }
    return SIT_OK;
}
