// Convex hulls of all sites' point clouds at once (SiteVolumes.compute_accessable_volumes, site_descriptors/SiteVolumes.py:
// 63-69, where the reference calls qhull per site): one workgroup per site wraps the recentred working copy that
// sit_grouped_recenter_step leaves in the context (group.hip) and only reads it.
//
// Gift wrapping.  The first facet comes from the first-facet rule of hull_predicates.h; from then on a step takes a wanted
// directed edge (u, v) off the list (hull_plan.h), every thread scans its share of the site's points with hp_pick, the 256
// candidates are joined by a shuffle tree in each wave and a tree over the waves in LDS - with the same hp_pick as
// comparator - and the winner w closes the facet (u, v, w).  Thread 0 keeps the list, the counts and the volume: the signed
// tetrahedron volumes against the first vertex, summed in the order the facets are found.  That order follows from the
// list discipline and the winners alone, and a winner reached through certified signs does not depend on the order of the
// merges: the bytes of a result are the same in every run.
//
// Nothing here depends on geometry to end: a pivot is a loop over the site's length, the wrap a loop of at most
// HP_FACET_CAP steps, the search of the list a loop over at most HP_OPEN_CAP entries.  A site whose signs were not all
// certified, or whose counts are not a closed surface's, ends with a status and no volume (NaN); the caller decides what
// to do with it (site_descriptors.py: qhull on the host, as before).
#include <cmath>
#include <climits>

#include "sit_internal.h"
#include "hull_predicates.h"
#include "hull_plan.h"

namespace {

__device__ __forceinline__ HpCand shuffle_down(const HpCand &c, int d)
{
    HpCand o;
    o.i = __shfl_down(c.i, d);
    o.uncertain = __shfl_down(c.uncertain, d);
    o.p[0] = __shfl_down(c.p[0], d);
    o.p[1] = __shfl_down(c.p[1], d);
    o.p[2] = __shfl_down(c.p[2], d);
    return o;
}

// Joins the candidates of the 256 threads; every thread gets the result.  After the step of distance d lane l holds the
// join of the lanes [l, l + 2 d) of its wave, lane 0 in the end that of all 64.
template <class Merge> __device__ HpCand hull_reduce(HpCand c, HpCand *s_wave, HpCand *s_win, Merge merge)
{
    const int t = threadIdx.x, lane = t & (HP_WAVE - 1), wave = t / HP_WAVE;
    for (int d = 1; d < HP_WAVE; d <<= 1) {
        const HpCand o = shuffle_down(c, d);
        if (lane + d < HP_WAVE) c = merge(c, o);
    }
    if (lane == 0) s_wave[wave] = c;
    __syncthreads();
    if (t == 0) {
        static_assert(HP_WAVES == 4, "the tree over the waves is written for four");
        *s_win = merge(merge(s_wave[0], s_wave[1]), merge(s_wave[2], s_wave[3]));
    }
    __syncthreads();
    return *s_win;
}

// the pivot about (a, b) over the site; b_real: b is a point of the site (the virtual second point of the first facet is not)
__device__ HpCand hull_pivot(const double *pts, i64 len, const double a[3], const double b[3], bool b_real, HpCand *s_wave, HpCand *s_win)
{
    HpCand c = hp_none();
    for (i64 j = threadIdx.x; j < len; j += HP_BLOCK) {
        const double q[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
        if (hp_same(q, a) || (b_real && hp_same(q, b))) continue;
        c = hp_pick(a, b, c, hp_point((uint32_t)j, q));
    }
    return hull_reduce(c, s_wave, s_win, [&](const HpCand &x, const HpCand &y) { return hp_pick(a, b, x, y); });
}

}

// work [N, 3], offsets [K + 1]; mask [N] zeroed by the host.  volumes [K] (NaN unless status 0), status [K], n_facets [K].
__global__ __launch_bounds__(HP_BLOCK) void k_group_hull(const double *work, const i64 *offsets, double *volumes, i32 *status, i32 *n_facets,
                                                         unsigned char *mask)
{
    __shared__ HullEdge s_open[HP_OPEN_CAP];
    __shared__ HpCand s_wave[HP_WAVES];
    __shared__ HpCand s_win;
    __shared__ HullEdge s_edge;
    __shared__ int s_pos[2], s_state, s_n;
    const int t = threadIdx.x;
    const i64 site = blockIdx.x;
    const i64 o = offsets[site], len = offsets[site + 1] - o;
    const double *pts = work + 3 * o;
    unsigned char *m = mask + o;

    int state = -1;                                              // the same in every thread at every barrier
    HullWrap w;                                                  // thread 0's
    hw_init(w, s_open);
    double vol = 0.0, p0[3] = {0.0, 0.0, 0.0};
    if (len < 4) state = HS_FEW;
    else if (len > HP_MAX_POINTS) state = HS_CAPACITY;
    if (state < 0) {
        HpCand c = hp_none();
        for (i64 j = t; j < len; j += HP_BLOCK) {
            const double q[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
            c = hp_pick_least(c, hp_point((uint32_t)j, q));
        }
        const HpCand a = hull_reduce(c, s_wave, &s_win, [](const HpCand &x, const HpCand &y) { return hp_pick_least(x, y); });
        double v[3];
        hp_virtual_second(a.p, v);
        const HpCand b = hull_pivot(pts, len, a.p, v, false, s_wave, &s_win);
        if (b.i == HP_NONE || b.uncertain) state = HS_UNCERTAIN;
        else {
            const HpCand cc = hull_pivot(pts, len, a.p, b.p, true, s_wave, &s_win);
            if (cc.i == HP_NONE || cc.uncertain) state = HS_UNCERTAIN;
            else if (t == 0) {
                hw_first(w, a.i, b.i, cc.i);
                m[a.i] = 1; m[b.i] = 1; m[cc.i] = 1;
                w.n_vertices = 3;
                p0[0] = a.p[0]; p0[1] = a.p[1]; p0[2] = a.p[2];
                double permanent;
                vol = hp_det(a.p, b.p, cc.p, p0, &permanent);    // an exact 0: p0 is a
            }
        }
    }
    if (state < 0) {
        for (int step = 0; step < HP_FACET_CAP; step++) {
            if (t == 0) {
                s_state = -1;
                if (w.overflow) s_state = HS_CAPACITY;
                else if (w.n_open == 0) s_state = hw_closed_status(w);
                else if (w.n_facets >= HP_FACET_CAP) s_state = HS_CAPACITY;
                else { s_edge = hw_take(w); s_n = w.n_open; s_pos[0] = INT_MAX; s_pos[1] = INT_MAX; }
            }
            __syncthreads();
            state = s_state;
            if (state >= 0) break;
            const HullEdge e = s_edge;
            const int n_open = s_n;
            const double pu[3] = {pts[3 * (i64)e.from], pts[3 * (i64)e.from + 1], pts[3 * (i64)e.from + 2]};
            const double pv[3] = {pts[3 * (i64)e.to], pts[3 * (i64)e.to + 1], pts[3 * (i64)e.to + 2]};
            const HpCand win = hull_pivot(pts, len, pu, pv, true, s_wave, &s_win);
            if (win.i == HP_NONE || win.uncertain) { state = HS_UNCERTAIN; break; }
            // is e.to->win or win->e.from wanted already?  the first position of each
            for (int k = t; k < n_open; k += HP_BLOCK) {
                const HullEdge x = s_open[k];
                if (x.from == e.to && x.to == win.i) atomicMin(&s_pos[0], k);
                if (x.from == win.i && x.to == e.from) atomicMin(&s_pos[1], k);
            }
            __syncthreads();
            if (t == 0) {
                hw_join(w, e, win.i, s_pos[0] == INT_MAX ? -1 : s_pos[0], s_pos[1] == INT_MAX ? -1 : s_pos[1]);
                if (!m[win.i]) { m[win.i] = 1; w.n_vertices++; }
                double permanent;
                vol += hp_det(pu, pv, win.p, p0, &permanent);
            }
        }
        if (state < 0) state = HS_CAPACITY;                      // (not reached: the last step's first branch always ends the loop)
    }
    if (t == 0) {
        status[site] = state;
        n_facets[site] = w.n_facets;
        volumes[site] = state == HS_CLOSED ? vol / 6.0 : NAN;
    }
}

extern "C" int sit_hull_plan(i64 *out4)
{
    if (!out4) return SIT_ERR_INVALID;
    out4[0] = HP_FACET_CAP; out4[1] = HP_OPEN_CAP; out4[2] = HP_BLOCK; out4[3] = HP_LDS_BYTES;
    return SIT_OK;
}

extern "C" int sit_grouped_hull_volumes(sit_ctx *c, double *volumes, int32_t *status, int32_t *n_facets, uint8_t *vertex_mask)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    GroupWork g;
    int rc = group_working_copy(c, "sit_grouped_hull_volumes", &g);
    if (rc) return rc;
    SIT_REQUIRE(c, volumes && status && n_facets, "sit_grouped_hull_volumes: missing array");
    if (g.K == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 K = g.K, N = g.N;
    double *d_vol;
    i32 *d_status, *d_facets;
    unsigned char *d_mask;
    rc = carve_scratch(c, [&](Carve &cv) {
        d_vol = cv.take<double>(K); d_status = cv.take<i32>(K); d_facets = cv.take<i32>(K); d_mask = cv.take<unsigned char>(N > 0 ? N : 1);
    });
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(d_mask, 0, (size_t)(N > 0 ? N : 1), c->stream));
    HIP_TRY(c, hipEventRecord(g.ev0, c->stream));
    k_group_hull<<<dim3((unsigned)K), dim3(HP_BLOCK), 0, c->stream>>>(g.work, g.d_offsets, d_vol, d_status, d_facets, d_mask);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(g.ev1, c->stream));
    HIP_TRY(c, hipMemcpyAsync(volumes, d_vol, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, d_status, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(n_facets, d_facets, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    if (vertex_mask && N > 0 && (rc = copy_to_host(c, vertex_mask, d_mask, (size_t)N))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, g.ev0, g.ev1);
    *g.ms_hull = ms;
    return SIT_OK;
}

extern "C" int sit_grouped_work_fetch(sit_ctx *c, i64 first, i64 n, double *pts)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    GroupWork g;
    int rc = group_working_copy(c, "sit_grouped_work_fetch", &g);
    if (rc) return rc;
    SIT_REQUIRE(c, first >= 0 && n >= 0 && first <= g.N && n <= g.N - first, "sit_grouped_work_fetch: a range outside the grouping");
    SIT_REQUIRE(c, pts || n == 0, "sit_grouped_work_fetch: missing array");
    if (n == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = copy_to_host(c, pts, g.work + 3 * first, (size_t)n * 24))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}
