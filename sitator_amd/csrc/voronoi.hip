// VoronoiSiteGenerator on the device: the periodic Voronoi nodes of the static lattice, which the reference asks the external
// Zeo++ `network` binary for (sitator/voronoi.py, sitator/util/zeo.py).  voronoi_plan.h has every decision - the sphere of a
// quadruple with its error bound, the certified membership test, the completeness of an atom's cell at a search radius, the
// record rules, the merge; this file has the launches.
//
// k_voronoi_neighbours: one workgroup per atom.  The threads take the static atoms in turn, each all translations of its atom
// that can lie within R (the ranges of barrier_plan.h, valid for any cell shape); what lies within R is appended to LDS and
// then sorted by (squared distance, static index, image) in a bitonic network - the keys are distinct, so the list does not
// depend on the order of arrival.
// k_voronoi_spheres: one workgroup per atom, its neighbours in LDS.  The pairs (a, b) of the list are dealt to the threads in
// chunks of VP_BLOCK in lexicographic order, a thread walks c > b; every candidate sphere is tested against the neighbours
// nearest first and left at the first one certified inside.  The records of a chunk are placed by a prefix sum over the
// threads: they land in enumeration order.  Counters and flags meet in integer atomics on LDS.  Float64 throughout.
// The driver runs all atoms at the first R, then those with VS_GROW at the next R of the plan, until none is left or a cap is
// hit; the records come back in atom order and are merged on the host (vp_merge).
#include <string.h>
#include <algorithm>

#include "sit_internal.h"
#include "voronoi_plan.h"

static_assert(VP_NBR_CAP == VP_BLOCK, "the sort holds one key per thread");
static_assert(sizeof(VpRecord) % 8 == 0, "records are copied by words");

__global__ __launch_bounds__(VP_BLOCK) void k_voronoi_neighbours(Pbc pbc, BarrierPlan pl, const double *pos, i64 S, const i32 *active, double R2,
                                                                 double *nq, i32 *nsid, i32 *ncount)
{
    __shared__ VpKey key[VP_NBR_CAP];
    __shared__ int cnt;
    const int t = threadIdx.x;
    const i64 slot = blockIdx.x;
    const i32 i = active[slot];
    if (t == 0) cnt = 0;
    key[t].d2 = INFINITY; key[t].s = 0x7fffffff; key[t].m[0] = key[t].m[1] = key[t].m[2] = 0;
    __syncthreads();
    const double pi[3] = {pos[3 * (i64)i], pos[3 * (i64)i + 1], pos[3 * (i64)i + 2]};
    double fi[3];
    cp_to_cell(pbc, pi, fi);
    for (i64 s = t; s < S; s += VP_BLOCK) {
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
                    if (s == (i64)i && m0 == 0 && m1 == 0 && m2 == 0) continue;
                    double q[3];
                    const double d2 = vp_relative(pbc, pi, ps, m0, m1, m2, q);
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
    const int n = cnt < VP_NBR_CAP ? cnt : VP_NBR_CAP;
    if (t < n) {
        const VpKey k = key[t];
        const double ps[3] = {pos[3 * (i64)k.s], pos[3 * (i64)k.s + 1], pos[3 * (i64)k.s + 2]};
        double q[3];
        vp_relative(pbc, pi, ps, k.m[0], k.m[1], k.m[2], q);
        double *out = nq + (slot * VP_NBR_CAP + t) * 3;
        out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
        nsid[slot * VP_NBR_CAP + t] = k.s;
    }
    if (t == 0) ncount[slot] = cnt;                                  // the true count, also beyond the cap
}

// pair index p of the pairs a < b of n items in lexicographic order -> (a, b)
__device__ __forceinline__ void pair_of(int p, int n, int &a, int &b)
{
    const double w = (double)(2 * n - 1);
    int r = (int)((w - sqrt(w * w - 8.0 * (double)p)) * 0.5);
    if (r < 0) r = 0;
    if (r > n - 2) r = n - 2;
    while (r + 1 <= n - 2 && (r + 1) * (2 * n - (r + 1) - 1) / 2 <= p) r++;
    while (r > 0 && r * (2 * n - r - 1) / 2 > p) r--;
    a = r;
    b = r + 1 + (p - r * (2 * n - r - 1) / 2);
}

__global__ __launch_bounds__(VP_BLOCK) void k_voronoi_spheres(const double *pos, const i32 *active, const double *nq, const i32 *nsid, const i32 *ncount,
                                                              double R, double tau, VpRecord *slab, i32 *nrec, i32 *status, i32 *nfar)
{
    __shared__ double q[VP_NBR_CAP * 3];
    __shared__ i32 sid[VP_NBR_CAP];
    __shared__ int scan[VP_BLOCK];
    __shared__ int s_far, s_flags, s_oct;
    const int t = threadIdx.x;
    const i64 slot = blockIdx.x;
    const i32 self = active[slot];
    const int n = ncount[slot];
    if (n > VP_NBR_CAP) {                                            // the whole workgroup leaves
        if (t == 0) { nrec[slot] = 0; nfar[slot] = 0; status[slot] = VS_CAPACITY; }
        return;
    }
    if (t == 0) { s_far = 0; s_flags = 0; s_oct = 0; }
    for (int k = t; k < 3 * n; k += VP_BLOCK) q[k] = nq[slot * VP_NBR_CAP * 3 + k];
    if (t < n) sid[t] = nsid[slot * VP_NBR_CAP + t];
    __syncthreads();
    if (t < n) {
        const int o = vp_octant(q + 3 * t);
        if (o >= 0) atomicOr(&s_oct, 1 << o);
    }
    const double p[3] = {pos[3 * (i64)self], pos[3 * (i64)self + 1], pos[3 * (i64)self + 2]};
    const int npairs = n * (n - 1) / 2;
    int base = 0;
    VpRecord *mine = slab + slot * VP_REC_CAP;
    for (int p0 = 0; p0 < npairs; p0 += VP_BLOCK) {
        const int pr = p0 + t;
        int a = 0, b = 0, nf = 0, found[VP_PAIR_FOUND], far = 0, flags = 0;
        if (pr < npairs) {
            pair_of(pr, n, a, b);
            for (int c = b + 1; c < n; c++) {
                const int kind = vp_candidate(q, sid, n, self, p, a, b, c, R, tau, nullptr);
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
        if (!__syncthreads_or(nf)) continue;                         // no record in this chunk (the same answer in every thread)
        scan[t] = nf;
        __syncthreads();
        for (int off = 1; off < VP_BLOCK; off <<= 1) {               // inclusive prefix sum
            const int v = t >= off ? scan[t - off] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const int at = base + scan[t] - nf;
        for (int j = 0; j < nf; j++) {
            if (at + j < VP_REC_CAP) {
                VpRecord rec;
                vp_candidate(q, sid, n, self, p, a, b, found[j], R, tau, &rec);
                mine[at + j] = rec;
            } else atomicOr(&s_flags, 2);
        }
        base += scan[VP_BLOCK - 1];
        __syncthreads();                                             // scan is read before the next chunk writes it
    }
    __syncthreads();
    if (t == 0) {
        nrec[slot] = base < VP_REC_CAP ? base : VP_REC_CAP;
        nfar[slot] = s_far;
        status[slot] = vp_status(0, s_flags & 2, s_oct, s_far, s_flags & 1);
    }
}

// the records of the atoms that are done, one after the other: dense[offsets[slot] ...] = slab[slot][0 .. offsets[slot + 1] - offsets[slot])
__global__ __launch_bounds__(VP_BLOCK) void k_voronoi_gather(const VpRecord *slab, const i64 *offsets, VpRecord *dense)
{
    const i64 slot = blockIdx.x;
    const i64 first = offsets[slot], count = offsets[slot + 1] - first;
    const int words = (int)(sizeof(VpRecord) / 4);
    const i32 *src = (const i32 *)(slab + slot * VP_REC_CAP);
    i32 *dst = (i32 *)(dense + first);
    for (i64 k = threadIdx.x; k < count * words; k += VP_BLOCK) dst[k] = src[k];
}

// the result of the last sit_voronoi_nodes of a context, kept for the fill call that follows the size call
struct VoronoiResult {
    std::vector<double> pos;                                         // the input it belongs to
    double tau = 0;
    std::vector<double> centers, radii;
    std::vector<i64> offsets;
    std::vector<i32> indices, status, nbr;
    double info[8] = {0};
};

void voronoi_free(sit_ctx *c)
{
    delete (VoronoiResult *)c->voronoi;
    c->voronoi = nullptr;
}

extern "C" int sit_voronoi_plan(const double *cell, int64_t S, int64_t *out8, double *radius2)
{
    if (!cell || !out8 || S < 1) return SIT_ERR_INVALID;
    struct { double cm[9]; } c;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) c.cm[3 * k + j] = cell[3 * j + k];
    const double vol = vp_volume(c);
    if (!(vol > 0.0) || !(vol < INFINITY)) return SIT_ERR_INVALID;
    out8[0] = VP_NBR_CAP; out8[1] = VP_REC_CAP; out8[2] = VP_MEMBER_CAP; out8[3] = VP_BLOCK; out8[4] = VP_LDS_BYTES;
    out8[5] = VP_MAX_ROUNDS; out8[6] = (int64_t)sizeof(VpRecord); out8[7] = (int64_t)(1.0 / VP_SHAPE_MIN);
    if (radius2) { radius2[0] = vp_radius(vol, S, 0); radius2[1] = VP_GROWTH; }
    return SIT_OK;
}

static int voronoi_compute(sit_ctx *c, const double *static_pos, i64 S, double tau, VoronoiResult &out)
{
    const double vol = vp_volume(c->pbc);
    SIT_REQUIRE(c, vol > 0.0 && vol < INFINITY, "sit_voronoi_nodes: degenerate cell");
    for (i64 s = 0; s < S; s++) {
        double f[3];
        cp_to_cell(c->pbc, static_pos + 3 * s, f);
        SIT_REQUIRE(c, fabs(f[0]) <= BP_MAX_FRAC && fabs(f[1]) <= BP_MAX_FRAC && fabs(f[2]) <= BP_MAX_FRAC,
                    "sit_voronoi_nodes: an atom that is not finite or more than 2^20 cells from the origin");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    out.pos.assign(static_pos, static_pos + 3 * S);
    out.tau = tau;
    out.status.assign((size_t)S, VS_GROW);
    out.nbr.assign((size_t)S, 0);
    out.centers.clear(); out.radii.clear(); out.indices.clear();
    out.offsets.assign(1, 0);
    for (double &v : out.info) v = 0.0;

    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(c, hipEventCreate(&ev.e0));
    HIP_TRY(c, hipEventCreate(&ev.e1));

    std::vector<std::vector<VpRecord>> records((size_t)S);
    std::vector<i32> active((size_t)S);
    for (i64 s = 0; s < S; s++) active[(size_t)s] = (i32)s;
    int rounds = 0;
    double R = 0.0, kernel_ms = 0.0;
    out.info[5] = vp_radius(vol, S, 0);
    while (!active.empty()) {
        BarrierPlan pl;
        const double Rk = vp_radius(vol, S, rounds);
        if (rounds >= VP_MAX_ROUNDS || !bp_plan(c->pbc, Rk, pl)) {   // nowhere to grow to
            for (i32 s : active) out.status[(size_t)s] = VS_CAPACITY;
            break;
        }
        R = Rk;
        rounds++;
        const i64 nA = (i64)active.size();
        double *d_pos, *d_nq;
        i32 *d_active, *d_nsid, *d_ncount, *d_nrec, *d_status, *d_nfar;
        i64 *d_off;
        VpRecord *d_slab;
        int rc = carve_scratch(c, [&](Carve &cv) {
            d_pos = cv.take<double>(3 * S, 64); d_active = cv.take<i32>(nA, 64); d_nq = cv.take<double>(nA * VP_NBR_CAP * 3, 64);
            d_nsid = cv.take<i32>(nA * VP_NBR_CAP, 64); d_ncount = cv.take<i32>(nA, 64); d_nrec = cv.take<i32>(nA, 64);
            d_status = cv.take<i32>(nA, 64); d_nfar = cv.take<i32>(nA, 64); d_off = cv.take<i64>(nA + 1, 64);
            d_slab = cv.take<VpRecord>(nA * VP_REC_CAP, 64);
        });
        if (rc) return rc;
        if ((rc = copy_to_device(c, d_pos, static_pos, (size_t)S * 24))) return rc;
        if ((rc = copy_to_device(c, d_active, active.data(), (size_t)nA * 4))) return rc;
        HIP_TRY(c, hipEventRecord(ev.e0, c->stream));
        k_voronoi_neighbours<<<dim3((unsigned)nA), dim3(VP_BLOCK), 0, c->stream>>>(c->pbc, pl, d_pos, S, d_active, R * R, d_nq, d_nsid, d_ncount);
        k_voronoi_spheres<<<dim3((unsigned)nA), dim3(VP_BLOCK), 0, c->stream>>>(d_pos, d_active, d_nq, d_nsid, d_ncount, R, tau, d_slab, d_nrec,
                                                                               d_status, d_nfar);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev.e1, c->stream));
        std::vector<i32> ncount((size_t)nA), nrec((size_t)nA), status((size_t)nA);
        if ((rc = copy_to_host(c, ncount.data(), d_ncount, (size_t)nA * 4))) return rc;
        if ((rc = copy_to_host(c, nrec.data(), d_nrec, (size_t)nA * 4))) return rc;
        if ((rc = copy_to_host(c, status.data(), d_status, (size_t)nA * 4))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        kernel_ms += ms;

        std::vector<i64> off((size_t)nA + 1, 0);
        std::vector<i32> next;
        for (i64 k = 0; k < nA; k++) {
            const i32 s = active[(size_t)k];
            SIT_REQUIRE(c, nrec[(size_t)k] >= 0 && nrec[(size_t)k] <= VP_REC_CAP && status[(size_t)k] >= VS_OK && status[(size_t)k] <= VS_CAPACITY,
                        "sit_voronoi_nodes: the sphere kernel returned a count or a status outside its range");
            out.status[(size_t)s] = status[(size_t)k];
            out.nbr[(size_t)s] = ncount[(size_t)k];
            if ((double)ncount[(size_t)k] > out.info[2]) out.info[2] = (double)ncount[(size_t)k];
            if (status[(size_t)k] == VS_GROW) next.push_back(s);
            off[(size_t)k + 1] = off[(size_t)k] + (status[(size_t)k] == VS_OK ? nrec[(size_t)k] : 0);
        }
        const i64 total = off[(size_t)nA];
        if (total > 0) {
            Scoped dense(c);
            HIP_TRY(c, sit_dmalloc(c, &dense.p, (size_t)total * sizeof(VpRecord)));
            if ((rc = copy_to_device(c, d_off, off.data(), (size_t)(nA + 1) * 8))) return rc;
            k_voronoi_gather<<<dim3((unsigned)nA), dim3(VP_BLOCK), 0, c->stream>>>(d_slab, d_off, (VpRecord *)dense.p);
            HIP_TRY(c, hipGetLastError());
            std::vector<VpRecord> got((size_t)total);
            if ((rc = copy_to_host(c, got.data(), dense.p, (size_t)total * sizeof(VpRecord)))) return rc;
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (i64 k = 0; k < nA; k++)
                records[(size_t)active[(size_t)k]].assign(got.begin() + off[(size_t)k], got.begin() + off[(size_t)k + 1]);
        }
        active.swap(next);
    }
    out.info[0] = (double)rounds; out.info[1] = R; out.info[4] = kernel_ms;

    bool all_ok = true;
    for (i64 s = 0; s < S; s++) all_ok = all_ok && out.status[(size_t)s] == VS_OK;
    if (!all_ok) return SIT_OK;                                      // never a partial network

    std::vector<VpRecord> flat;
    for (i64 s = 0; s < S; s++) flat.insert(flat.end(), records[(size_t)s].begin(), records[(size_t)s].end());
    const i64 n = (i64)flat.size();
    out.info[3] = (double)n;
    std::vector<double> w((size_t)(3 * n));
    for (i64 k = 0; k < n; k++) {
        double fl[3];
        SIT_REQUIRE(c, flat[(size_t)k].n >= 1 && flat[(size_t)k].n <= VP_MEMBER_CAP, "sit_voronoi_nodes: a record with a member count outside its range");
        cp_wrap(c->pbc, flat[(size_t)k].c, &w[(size_t)(3 * k)], fl);
    }
    std::vector<i64> node, first;
    const int merged = vp_merge(c->pbc, w.data(), n, VP_MU_FACTOR * tau, node, first);
    out.info[6] = (double)merged;
    if (merged != VS_OK) return SIT_OK;
    const i64 n_nodes = (i64)first.size();
    std::vector<std::vector<i32>> verts((size_t)n_nodes);
    for (i64 k = 0; k < n; k++) {
        std::vector<i32> &v = verts[(size_t)node[(size_t)k]];
        for (int j = 0; j < flat[(size_t)k].n; j++) {
            const i32 m = flat[(size_t)k].m[j];
            SIT_REQUIRE(c, m >= 0 && (i64)m < S, "sit_voronoi_nodes: a record names an atom outside the lattice");
            v.push_back(m);
        }
    }
    out.centers.resize((size_t)(3 * n_nodes));
    out.radii.resize((size_t)n_nodes);
    for (i64 j = 0; j < n_nodes; j++) {
        std::vector<i32> &v = verts[(size_t)j];
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        out.indices.insert(out.indices.end(), v.begin(), v.end());
        out.offsets.push_back((i64)out.indices.size());
        for (int k = 0; k < 3; k++) out.centers[(size_t)(3 * j + k)] = w[(size_t)(3 * first[(size_t)j] + k)];
        out.radii[(size_t)j] = flat[(size_t)first[(size_t)j]].r;
    }
    return SIT_OK;
}

extern "C" int sit_voronoi_nodes(sit_ctx *c, const double *static_pos, int64_t S, double tau, int64_t node_cap, int64_t index_cap,
                                 int64_t *n_nodes, int64_t *n_indices, double *centers, double *radii, int64_t *offsets, int32_t *indices,
                                 int32_t *status, int32_t *nbr_count, double *info8)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, static_pos && n_nodes && n_indices, "sit_voronoi_nodes: missing array");
    SIT_REQUIRE(c, S >= 1 && S < ((i64)1 << 24), "sit_voronoi_nodes: no atom, or more than 2^24 atoms");
    SIT_REQUIRE(c, tau > 0.0 && tau < INFINITY, "sit_voronoi_nodes: the tolerance is not positive");
    SIT_REQUIRE(c, node_cap >= 0 && index_cap >= 0, "sit_voronoi_nodes: negative capacity");
    VoronoiResult *res = (VoronoiResult *)c->voronoi;
    const bool cached = res && res->tau == tau && (i64)res->pos.size() == 3 * S && memcmp(res->pos.data(), static_pos, (size_t)S * 24) == 0;
    if (!cached) {
        voronoi_free(c);
        res = new VoronoiResult;
        const int rc = voronoi_compute(c, static_pos, S, tau, *res);
        if (rc != SIT_OK) { delete res; return rc; }
        c->voronoi = res;
    }
    const i64 nn = (i64)res->radii.size(), ni = (i64)res->indices.size();
    *n_nodes = nn; *n_indices = ni;
    if (status) memcpy(status, res->status.data(), (size_t)S * 4);
    if (nbr_count) memcpy(nbr_count, res->nbr.data(), (size_t)S * 4);
    if (info8) memcpy(info8, res->info, sizeof(res->info));
    if (nn <= node_cap && ni <= index_cap) {                         // the fill call
        if (centers && nn) memcpy(centers, res->centers.data(), (size_t)nn * 24);
        if (radii && nn) memcpy(radii, res->radii.data(), (size_t)nn * 8);
        if (offsets) memcpy(offsets, res->offsets.data(), (size_t)(nn + 1) * 8);
        if (indices && ni) memcpy(indices, res->indices.data(), (size_t)ni * 4);
    }
    return SIT_OK;
}
