// SiteCoordinationEnvironment on the device: the coordinating atoms of every site and the continuous shape measure of their
// polyhedron against the shape library, which the reference asks pymatgen's ChemEnv for, one site at a time in a Python loop
// (sitator/site_descriptors/SiteCoordinationEnvironment.py).  coordenv_plan.h has every decision; this file has the launches.
//
// k_coordenv_cell: one workgroup per site.  The neighbour walk and the bitonic sort of k_voronoi_neighbours with the site as the
// centre, the list staying in LDS; then the enumeration of k_voronoi_spheres (pairs dealt to the threads in chunks, records placed
// by a prefix sum: the cell's vertices land in LDS in enumeration order); then one thread per neighbour orders its face and sums
// its solid angle, and the coordinating images are written through a second prefix sum in the neighbour order.
// k_coordenv_csm: one workgroup per (site, shape of its n).  q and p sit in LDS, a thread unranks the first assignment of its chunk
// and steps through the rest, keeping its best t in a register; the maximum meets by wave shuffles and then over the four waves
// in LDS.  A maximum does not depend on arrival: two calls return the same bytes.  Float64 throughout.
#include <string.h>
#include <algorithm>

#include "sit_internal.h"
#include "coordenv_plan.h"

static_assert(VP_NBR_CAP == CE_BLOCK, "the sort holds one key per thread");
static_assert(sizeof(CeVertex) == 64, "a vertex is 64 bytes of LDS");
static_assert(CE_REC_CAP <= 256 && VP_NBR_CAP <= 256, "vertices and members are named by bytes");

__global__ __launch_bounds__(CE_BLOCK) void k_coordenv_cell(Pbc pbc, BarrierPlan pl, const double *pos, i64 S, const double *centers, const i32 *active,
                                                            double R, double tau, double dcut, double acut, CeSite *sites, i32 *csid, double *cq)
{
    __shared__ VpKey key[VP_NBR_CAP];
    __shared__ double q[VP_NBR_CAP * 3];
    __shared__ i32 sid[VP_NBR_CAP];
    __shared__ CeVertex rec[CE_REC_CAP];
    __shared__ double w[VP_NBR_CAP], dist[VP_NBR_CAP];
    __shared__ int touched[VP_NBR_CAP];
    __shared__ int scan[CE_BLOCK];
    __shared__ int cnt, s_far, s_flags, s_oct, s_status;
    const int t = threadIdx.x;
    const i64 slot = blockIdx.x;
    const i64 site = active[slot];
    CeSite *out = sites + slot;
    if (t == 0) { cnt = 0; s_far = 0; s_flags = 0; s_oct = 0; }
    key[t].d2 = INFINITY; key[t].s = 0x7fffffff; key[t].m[0] = key[t].m[1] = key[t].m[2] = 0;
    __syncthreads();
    const double pi[3] = {centers[3 * site], centers[3 * site + 1], centers[3 * site + 2]};
    double fi[3];
    cp_to_cell(pbc, pi, fi);
    const double R2 = R * R;
    for (i64 s = t; s < S; s += CE_BLOCK) {
        const double ps[3] = {pos[3 * s], pos[3 * s + 1], pos[3 * s + 2]};
        double fs[3];
        cp_to_cell(pbc, ps, fs);
        int lo[3], hi[3];
        bool any = true;
        for (int a = 0; a < 3; a++) {
            bp_axis_range(fi[a] - fs[a], pl.q[a], pl.n[a], &lo[a], &hi[a]);
            any = any && lo[a] <= hi[a];
        }
        if (!any) continue;
        for (int m0 = lo[0]; m0 <= hi[0]; m0++)
            for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                    double x[3];
                    const double d2 = vp_relative(pbc, pi, ps, m0, m1, m2, x);
                    if (d2 <= R2) {
                        const int at = atomicAdd(&cnt, 1);
                        if (at < VP_NBR_CAP) { key[at].d2 = d2; key[at].s = (i32)s; key[at].m[0] = m0; key[at].m[1] = m1; key[at].m[2] = m2; }
                    }
                }
    }
    __syncthreads();
    for (int k = 2; k <= VP_NBR_CAP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int other = t ^ j;
            if (other > t) {
                const VpKey x = key[t], y = key[other];
                const bool up = (t & k) == 0;
                if (up ? vp_key_less(y, x) : vp_key_less(x, y)) { key[t] = y; key[other] = x; }
            }
            __syncthreads();
        }
    const int count = cnt;
    if (count > VP_NBR_CAP) {                                        // the whole workgroup leaves
        if (t == 0) { out->status = VS_CAPACITY; out->flags = 0; out->n = 0; out->nbr = count; }
        return;
    }
    const int n = count;
    if (t < n) {
        const VpKey k = key[t];
        const double ps[3] = {pos[3 * (i64)k.s], pos[3 * (i64)k.s + 1], pos[3 * (i64)k.s + 2]};
        double x[3];
        vp_relative(pbc, pi, ps, k.m[0], k.m[1], k.m[2], x);
        q[3 * t] = x[0]; q[3 * t + 1] = x[1]; q[3 * t + 2] = x[2];
        sid[t] = k.s;
        dist[t] = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
        const int o = vp_octant(x);
        if (o >= 0) atomicOr(&s_oct, 1 << o);
    }
    __syncthreads();

    const int npairs = n * (n - 1) / 2;
    int base = 0;
    for (int p0 = 0; p0 < npairs; p0 += CE_BLOCK) {
        const int pr = p0 + t;
        int a = 0, b = 0, nf = 0, found[VP_PAIR_FOUND], far = 0, flags = 0;
        if (pr < npairs) {
            // pair index -> (a, b), a < b, lexicographic
            const double ww = (double)(2 * n - 1);
            int r = (int)((ww - sqrt(ww * ww - 8.0 * (double)pr)) * 0.5);
            if (r < 0) r = 0;
            if (r > n - 2) r = n - 2;
            while (r + 1 <= n - 2 && (r + 1) * (2 * n - (r + 1) - 1) / 2 <= pr) r++;
            while (r > 0 && r * (2 * n - r - 1) / 2 > pr) r--;
            a = r;
            b = r + 1 + (pr - r * (2 * n - r - 1) / 2);
            for (int c = b + 1; c < n; c++) {
                const int kind = ce_candidate(q, n, a, b, c, R, tau, nullptr);
                if (kind == VC_FAR) far++;
                else if (kind == VC_UNCERTAIN) flags |= 1;
                else if (kind == VC_CAPACITY) flags |= 2;
                else if (kind == VC_RECORD) {
                    if (nf < VP_PAIR_FOUND) found[nf++] = c;
                    else flags |= 2;
                }
            }
        }
        if (far) atomicAdd(&s_far, far);
        if (flags) atomicOr(&s_flags, flags);
        if (!__syncthreads_or(nf)) continue;
        scan[t] = nf;
        __syncthreads();
        for (int off = 1; off < CE_BLOCK; off <<= 1) {
            const int v = t >= off ? scan[t - off] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const int at = base + scan[t] - nf;
        for (int j = 0; j < nf; j++) {
            if (at + j < CE_REC_CAP) {
                CeVertex v;
                ce_candidate(q, n, a, b, found[j], R, tau, &v);
                rec[at + j] = v;
            } else atomicOr(&s_flags, 2);
        }
        base += scan[CE_BLOCK - 1];
        __syncthreads();
    }
    __syncthreads();
    if (t == 0) {
        int st = vp_status(0, s_flags & 2, s_oct, s_far, s_flags & 1);
        if (st == VS_OK && n > 0 && !(dist[0] > 0.0)) st = VS_UNCERTAIN;        // an atom on the site itself
        s_status = st;
        s_flags = 0;
    }
    __syncthreads();
    if (s_status != VS_OK) {
        if (t == 0) { out->status = s_status; out->flags = 0; out->n = 0; out->nbr = count; }
        return;
    }
    const int nrec = base < CE_REC_CAP ? base : CE_REC_CAP;

    int mine = 0, over = 0;
    if (t < n) {
        w[t] = ce_face_angle(q + 3 * t, rec, nrec, t, &mine, &over);
        touched[t] = mine;
    }
    if (over) atomicOr(&s_flags, 2);
    __syncthreads();
    double d_min = INFINITY, w_max = 0.0;
    for (int j = 0; j < n; j++)
        if (touched[j]) {
            if (dist[j] < d_min) d_min = dist[j];
            if (w[j] > w_max) w_max = w[j];
        }
    double nd = 0.0, na = 0.0;
    int in = 0, near = 0;
    if (t < n && mine) in = ce_select(dist[t], d_min, w[t], w_max, dcut, acut, &nd, &na, &near) ? 1 : 0;
    if (near) atomicOr(&s_flags, 1);
    scan[t] = in;
    __syncthreads();
    for (int off = 1; off < CE_BLOCK; off <<= 1) {
        const int v = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const int total = scan[CE_BLOCK - 1];
    const bool fits = total <= CE_COORD_CAP && !(s_flags & 2);
    if (in && fits) {
        const int at = scan[t] - 1;
        out->pos[at] = t; out->nd[at] = nd; out->na[at] = na;
        csid[slot * CE_COORD_CAP + at] = sid[t];
        if (at < CE_N_MAX) {
            double *o = cq + (slot * CE_N_MAX + at) * 3;
            o[0] = q[3 * t]; o[1] = q[3 * t + 1]; o[2] = q[3 * t + 2];
        }
    }
    if (t == 0) {
        out->status = fits ? VS_OK : VS_CAPACITY;
        out->flags = fits && (s_flags & 1) ? CF_NEAR_CUTOFF : 0;
        out->n = fits ? total : 0;
        out->nbr = count;
    }
}

__global__ __launch_bounds__(CE_BLOCK) void k_coordenv_csm(const CeSite *sites, const double *cq, const double *table, int use_bound, double *csm)
{
    __shared__ double q[CE_N_MAX * 3], p[CE_N_MAX * 3];
    __shared__ double part[CE_BLOCK / 64];
    const int t = threadIdx.x;
    const i64 site = blockIdx.x / CE_SHAPES_PER_N;
    const int col = blockIdx.x % CE_SHAPES_PER_N;
    const int n = sites[site].status == VS_OK ? sites[site].n : 0;
    int shapes[CE_SHAPES_PER_N];
    ce_shapes_of(n, shapes);
    const int s = shapes[col];
    if (s < 0 || n > CE_N_MAX) {                                     // uniform over the workgroup
        if (t == 0) csm[blockIdx.x] = NAN;
        return;
    }
    if (n == 1) {                                                    // S:1 is 0 by definition
        if (t == 0) csm[blockIdx.x] = 0.0;
        return;
    }
    if (t < 3 * n) { q[t] = cq[site * CE_N_MAX * 3 + t]; p[t] = table[s * CE_N_MAX * 3 + t]; }
    __syncthreads();
    const i64 total = ce_factorial(n), chunk = (total + CE_BLOCK - 1) / CE_BLOCK;
    const i64 first = (i64)t * chunk;
    const i64 count = first < total ? (first + chunk <= total ? chunk : total - first) : 0;
    double best = ce_best_t(q, p, n, first, count, use_bound);
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(best, off, 64);
        if (o > best) best = o;
    }
    if ((t & 63) == 0) part[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < CE_BLOCK / 64; k++)
            if (part[k] > best) best = part[k];
        csm[blockIdx.x] = ce_measure(best, ce_norm2(q, n), ce_norm2(p, n));
    }
}

// the result of the last sit_coordination_environments of a context, kept for the fill call that follows the size call
struct CoordEnvResult {
    std::vector<double> pos, centers;                                // the input it belongs to
    double par[4] = {0, 0, 0, 0};                                    // tau, distance cutoff, angle cutoff, max_csm
    std::vector<i32> status, flags, n, indices, shape;
    std::vector<i64> offsets;
    std::vector<double> nd, na, csm_best, csm_all, confidence;
    double info[8] = {0};
};

void coordenv_free(sit_ctx *c)
{
    delete (CoordEnvResult *)c->coordenv;
    c->coordenv = nullptr;
}

extern "C" int sit_coordenv_plan(int64_t *out8, int32_t *shape_n, double *coords)
{
    if (!out8) return SIT_ERR_INVALID;
    out8[0] = VP_NBR_CAP; out8[1] = CE_REC_CAP; out8[2] = CE_FACE_CAP; out8[3] = CE_COORD_CAP; out8[4] = CE_N_MAX; out8[5] = CE_BLOCK;
    out8[6] = CE_LDS_BYTES; out8[7] = CE_SHAPES;
    if (shape_n)
        for (int s = 0; s < CE_SHAPES; s++) shape_n[s] = ce_shape_n(s);
    if (coords) ce_shape_table(coords);
    return SIT_OK;
}

static int coordenv_compute(sit_ctx *c, const double *static_pos, i64 S, const double *centers, i64 K, const double par[4], CoordEnvResult &out)
{
    const double tau = par[0], dcut = par[1], acut = par[2], max_csm = par[3];
    const double vol = vp_volume(c->pbc);
    SIT_REQUIRE(c, vol > 0.0 && vol < INFINITY, "sit_coordination_environments: degenerate cell");
    for (int pass = 0; pass < 2; pass++) {
        const double *x = pass ? centers : static_pos;
        for (i64 s = 0; s < (pass ? K : S); s++) {
            double f[3];
            cp_to_cell(c->pbc, x + 3 * s, f);
            SIT_REQUIRE(c, fabs(f[0]) <= BP_MAX_FRAC && fabs(f[1]) <= BP_MAX_FRAC && fabs(f[2]) <= BP_MAX_FRAC,
                        "sit_coordination_environments: an atom or a site that is not finite or more than 2^20 cells from the origin");
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    out.pos.assign(static_pos, static_pos + 3 * S);
    out.centers.assign(centers, centers + 3 * K);
    memcpy(out.par, par, sizeof(out.par));
    out.status.assign((size_t)K, VS_GROW);
    out.flags.assign((size_t)K, 0);
    out.n.assign((size_t)K, 0);
    out.shape.assign((size_t)K, -1);
    out.csm_best.assign((size_t)K, NAN);
    out.csm_all.assign((size_t)K * CE_SHAPES_PER_N, NAN);
    out.confidence.assign((size_t)K, 0.0);
    out.offsets.assign((size_t)K + 1, 0);
    out.indices.clear(); out.nd.clear(); out.na.clear();
    for (double &v : out.info) v = 0.0;

    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(c, hipEventCreate(&ev.e0));
    HIP_TRY(c, hipEventCreate(&ev.e1));

    double table[CE_SHAPES * CE_N_MAX * 3];
    ce_shape_table(table);

    // what the csm kernel reads of every site, in site order (pool buffer: it outlives the rounds' scratch)
    Scoped keep(c);
    const size_t site_bytes = (size_t)K * sizeof(CeSite), cq_bytes = (size_t)K * CE_N_MAX * 3 * 8, table_bytes = sizeof(table);
    const size_t csm_bytes = (size_t)K * CE_SHAPES_PER_N * 8;
    HIP_TRY(c, sit_dmalloc(c, &keep.p, site_bytes + cq_bytes + table_bytes + csm_bytes));
    CeSite *d_all = (CeSite *)keep.p;
    double *d_allq = (double *)((char *)keep.p + site_bytes), *d_table = (double *)((char *)keep.p + site_bytes + cq_bytes);
    double *d_csm = (double *)((char *)keep.p + site_bytes + cq_bytes + table_bytes);

    std::vector<CeSite> sites((size_t)K);
    std::vector<double> allq((size_t)K * CE_N_MAX * 3, 0.0);
    std::vector<std::vector<i32>> sidx((size_t)K);
    for (CeSite &s : sites) { memset(&s, 0, sizeof(s)); s.status = VS_GROW; }
    std::vector<i32> active((size_t)K);
    for (i64 k = 0; k < K; k++) active[(size_t)k] = (i32)k;
    int rounds = 0;
    double R = 0.0, cell_ms = 0.0, csm_ms = 0.0;
    out.info[6] = vp_radius(vol, S, 0);
    while (!active.empty()) {
        BarrierPlan pl;
        const double Rk = vp_radius(vol, S, rounds);
        if (rounds >= VP_MAX_ROUNDS || !bp_plan(c->pbc, Rk, pl)) {   // nowhere to grow to
            for (i32 s : active) sites[(size_t)s].status = VS_CAPACITY;
            break;
        }
        R = Rk;
        rounds++;
        const i64 nA = (i64)active.size();
        double *d_pos, *d_cen, *d_cq;
        i32 *d_active, *d_csid;
        CeSite *d_sites;
        int rc = carve_scratch(c, [&](Carve &cv) {
            d_pos = cv.take<double>(3 * S, 64); d_cen = cv.take<double>(3 * K, 64); d_active = cv.take<i32>(nA, 64);
            d_sites = cv.take<CeSite>(nA, 64); d_csid = cv.take<i32>(nA * CE_COORD_CAP, 64); d_cq = cv.take<double>(nA * CE_N_MAX * 3, 64);
        });
        if (rc) return rc;
        if ((rc = copy_to_device(c, d_pos, static_pos, (size_t)S * 24))) return rc;
        if ((rc = copy_to_device(c, d_cen, centers, (size_t)K * 24))) return rc;
        if ((rc = copy_to_device(c, d_active, active.data(), (size_t)nA * 4))) return rc;
        HIP_TRY(c, hipMemsetAsync(d_cq, 0, (size_t)nA * CE_N_MAX * 24, c->stream));
        HIP_TRY(c, hipMemsetAsync(d_csid, 0, (size_t)nA * CE_COORD_CAP * 4, c->stream));
        HIP_TRY(c, hipEventRecord(ev.e0, c->stream));
        k_coordenv_cell<<<dim3((unsigned)nA), dim3(CE_BLOCK), 0, c->stream>>>(c->pbc, pl, d_pos, S, d_cen, d_active, R, tau, dcut, acut, d_sites, d_csid,
                                                                             d_cq);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev.e1, c->stream));
        std::vector<CeSite> got((size_t)nA);
        std::vector<i32> csid((size_t)nA * CE_COORD_CAP);
        std::vector<double> cq((size_t)nA * CE_N_MAX * 3);
        if ((rc = copy_to_host(c, got.data(), d_sites, (size_t)nA * sizeof(CeSite)))) return rc;
        if ((rc = copy_to_host(c, csid.data(), d_csid, csid.size() * 4))) return rc;
        if ((rc = copy_to_host(c, cq.data(), d_cq, cq.size() * 8))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        cell_ms += ms;
        std::vector<i32> next;
        for (i64 k = 0; k < nA; k++) {
            const i32 s = active[(size_t)k];
            const CeSite &g = got[(size_t)k];
            SIT_REQUIRE(c, g.status >= VS_OK && g.status <= VS_CAPACITY && g.n >= 0 && g.n <= CE_COORD_CAP,
                        "sit_coordination_environments: the cell kernel returned a count or a status outside its range");
            sites[(size_t)s] = g;
            if ((double)g.nbr > out.info[2]) out.info[2] = (double)g.nbr;
            if (g.status == VS_GROW) { next.push_back(s); continue; }
            if (g.status != VS_OK) continue;
            sidx[(size_t)s].assign(csid.begin() + k * CE_COORD_CAP, csid.begin() + k * CE_COORD_CAP + g.n);
            std::copy(cq.begin() + k * CE_N_MAX * 3, cq.begin() + (k + 1) * CE_N_MAX * 3, allq.begin() + (i64)s * CE_N_MAX * 3);
        }
        active.swap(next);
    }
    out.info[0] = (double)rounds; out.info[1] = R; out.info[4] = cell_ms;

    int rc;
    if ((rc = copy_to_device(c, d_all, sites.data(), site_bytes))) return rc;
    if ((rc = copy_to_device(c, d_allq, allq.data(), cq_bytes))) return rc;
    if ((rc = copy_to_device(c, d_table, table, table_bytes))) return rc;
    HIP_TRY(c, hipEventRecord(ev.e0, c->stream));
    k_coordenv_csm<<<dim3((unsigned)(K * CE_SHAPES_PER_N)), dim3(CE_BLOCK), 0, c->stream>>>(d_all, d_allq, d_table, 1, d_csm);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e1, c->stream));
    if ((rc = copy_to_host(c, out.csm_all.data(), d_csm, csm_bytes))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        csm_ms = ms;
    }
    out.info[5] = csm_ms;

    for (i64 k = 0; k < K; k++) {
        const CeSite &s = sites[(size_t)k];
        out.status[(size_t)k] = s.status;
        out.flags[(size_t)k] = s.flags;
        out.n[(size_t)k] = s.status == VS_OK ? s.n : 0;
        if (s.status == VS_OK) {
            for (int j = 0; j < s.n; j++) {
                const i32 m = sidx[(size_t)k][(size_t)j];
                SIT_REQUIRE(c, m >= 0 && (i64)m < S, "sit_coordination_environments: the cell kernel names an atom outside the lattice");
                out.indices.push_back(m); out.nd.push_back(s.nd[j]); out.na.push_back(s.na[j]);
            }
            if ((double)s.n > out.info[3]) out.info[3] = (double)s.n;
            int shapes[CE_SHAPES_PER_N];
            const int ns = s.n <= CE_N_MAX ? ce_shapes_of(s.n, shapes) : 0;
            const int best = ce_decide(&out.csm_all[(size_t)k * CE_SHAPES_PER_N], ns, max_csm, &out.confidence[(size_t)k], &out.csm_best[(size_t)k]);
            out.shape[(size_t)k] = best >= 0 ? shapes[best] : -1;
        } else {
            for (int j = 0; j < CE_SHAPES_PER_N; j++) out.csm_all[(size_t)k * CE_SHAPES_PER_N + j] = NAN;
        }
        out.offsets[(size_t)k + 1] = (i64)out.indices.size();
    }
    return SIT_OK;
}

extern "C" int sit_coordination_environments(sit_ctx *c, const double *static_pos, int64_t S, const double *centers, int64_t K, double tau,
                                             double distance_cutoff, double angle_cutoff, double max_csm, int64_t index_cap, int64_t *n_indices,
                                             int32_t *status, int32_t *flags, int32_t *n, int64_t *offsets, int32_t *indices, double *norm_distance,
                                             double *norm_angle, int32_t *shape, double *csm_best, double *csm_all, double *confidence, double *info8)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, static_pos && centers && n_indices, "sit_coordination_environments: missing array");
    SIT_REQUIRE(c, S >= 1 && K >= 1, "sit_coordination_environments: no atom or no site");
    SIT_REQUIRE(c, tau > 0.0 && tau < INFINITY, "sit_coordination_environments: the tolerance is not positive");
    SIT_REQUIRE(c, distance_cutoff >= 1.0 && distance_cutoff < INFINITY, "sit_coordination_environments: the distance cutoff is below 1 or not finite");
    SIT_REQUIRE(c, angle_cutoff > 0.0 && angle_cutoff <= 1.0, "sit_coordination_environments: the angle cutoff is outside (0, 1]");
    SIT_REQUIRE(c, max_csm > 0.0 && max_csm < INFINITY, "sit_coordination_environments: max_csm is not positive");
    SIT_REQUIRE(c, index_cap >= 0, "sit_coordination_environments: negative capacity");
    if (S >= ((i64)1 << 24) || K >= ((i64)1 << 24)) {
        c->msg = "sit_coordination_environments: more than 2^24 atoms or sites";
        return SIT_ERR_CAPACITY;
    }
    const double par[4] = {tau, distance_cutoff, angle_cutoff, max_csm};
    CoordEnvResult *res = (CoordEnvResult *)c->coordenv;
    const bool cached = res && memcmp(res->par, par, sizeof(par)) == 0 && (i64)res->pos.size() == 3 * S && (i64)res->centers.size() == 3 * K
                        && memcmp(res->pos.data(), static_pos, (size_t)S * 24) == 0 && memcmp(res->centers.data(), centers, (size_t)K * 24) == 0;
    if (!cached) {
        coordenv_free(c);
        res = new CoordEnvResult;
        const int rc = coordenv_compute(c, static_pos, S, centers, K, par, *res);
        if (rc != SIT_OK) { delete res; return rc; }
        c->coordenv = res;
    }
    const i64 ni = (i64)res->indices.size();
    *n_indices = ni;
    if (status) memcpy(status, res->status.data(), (size_t)K * 4);
    if (flags) memcpy(flags, res->flags.data(), (size_t)K * 4);
    if (n) memcpy(n, res->n.data(), (size_t)K * 4);
    if (shape) memcpy(shape, res->shape.data(), (size_t)K * 4);
    if (csm_best) memcpy(csm_best, res->csm_best.data(), (size_t)K * 8);
    if (csm_all) memcpy(csm_all, res->csm_all.data(), (size_t)K * CE_SHAPES_PER_N * 8);
    if (confidence) memcpy(confidence, res->confidence.data(), (size_t)K * 8);
    if (info8) { memcpy(info8, res->info, sizeof(res->info)); info8[7] = cached ? 0.0 : 1.0; }
    if (ni <= index_cap) {                                           // the fill call
        if (offsets) memcpy(offsets, res->offsets.data(), (size_t)(K + 1) * 8);
        if (indices && ni) memcpy(indices, res->indices.data(), (size_t)ni * 4);
        if (norm_distance && ni) memcpy(norm_distance, res->nd.data(), (size_t)ni * 8);
        if (norm_angle && ni) memcpy(norm_angle, res->na.data(), (size_t)ni * 8);
    }
    return SIT_OK;
}
