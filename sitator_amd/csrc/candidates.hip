// Construction of the result-preserving landmark pruning tables, on the device.
//
// A landmark component is non-zero only if EVERY vertex h of landmark k satisfies
// dist/vcd[k,h] <= cutoff_round_to_zero (landmark/helpers.pyx:196-203).  The distance is a
// shift-and-wrap distance (helpers.pyx:99-103,176), which is the norm of ONE periodic image
// of the displacement and therefore >= the true periodic distance d_P.  Every static atom
// that passed the static-lattice check is within static_threshold of its reference position
// (helpers.pyx:76), again in a metric >= d_P.  Hence for an ion anywhere inside a bin with
// centre c_b and covering radius r_b:
//     component k non-zero  =>  for all h:  d_P(c_b, ref[v_kh]) <= rz*vcd[k,h] + thr + r_b
// The tables list, per fractional-coordinate bin, every landmark that satisfies the right-hand
// side (computed with an exhaustive image search, so it holds for any cell shape or size).
// Landmarks not listed are exactly 0.0 for that ion, as in the reference; listed ones are
// evaluated with the reference's arithmetic.  Lists are ascending in k, so the sparse row is
// ordered like the dense one.
//
// One workgroup per landmark walks the bins of the box around the landmark's tightest vertex:
// pass 1 counts the landmarks per bin, a scan turns the counts into offsets, pass 2 repeats the
// tests and scatters (with each entry's critical vertex), pass 3 sorts every bin's (short) list.
#include "sit_internal.h"
#include "candidates_plan.h"

namespace {

// The decisions - bound, box, pair test, critical vertex - are candidates_plan.h's (host-tested); the kernels keep the
// parallel structure.  FILL = false: count; true: scatter
template <bool FILL>
__global__ __launch_bounds__(256) void k_cand_pass(CandArgs a)
{
    const i64 k = blockIdx.x;
    const CandBox box = cand_box(a, k);
    const i64 total = cand_box_bins(box);
    for (i64 q = threadIdx.x; q < total; q += 256) {
        double cb[3];
        const i64 b = cand_box_bin(a, box, q, cb);
        if (!cand_pair_listed(a, k, box.nv, cb)) continue;
        if (!FILL) atomicAdd(&a.cnt[b + 1], 1);
        else a.list[a.cnt[b] + atomicAdd(&a.cursor[b], 1)] = cand_pack(k, cand_critical_vertex(a, k, box.nv, cb));
    }
}

// exclusive scan of cnt[1..nb] in place (cnt[0] = 0), one workgroup; also the widest bin
__global__ __launch_bounds__(1024) void k_cand_scan(i32 *cnt, i64 nb, i32 *stats)
{
    __shared__ long long part[1024];
    __shared__ int wmax[1024];
    const int t = threadIdx.x;
    const i64 per = (nb + 1023) / 1024;
    const i64 lo = 1 + t * per, hi = (lo + per) < (nb + 1) ? (lo + per) : (nb + 1);
    long long s = 0;
    int w = 0;
    for (i64 i = lo; i < hi; i++) { s += cnt[i]; w = cnt[i] > w ? cnt[i] : w; }
    part[t] = s; wmax[t] = w;
    __syncthreads();
    if (t == 0) {
        long long acc = 0;
        int m = 0;
        for (int i = 0; i < 1024; i++) { const long long v = part[i]; part[i] = acc; acc += v; m = wmax[i] > m ? wmax[i] : m; }
        stats[0] = m;
        stats[1] = (i32)(acc & 0x7fffffff); stats[2] = (i32)(acc >> 31);
    }
    __syncthreads();
    long long acc = part[t];
    for (i64 i = lo; i < hi; i++) { acc += cnt[i]; cnt[i] = (i32)acc; }
}

// ascending k inside every bin (the scatter order is arbitrary); the critical vertex moves to its own array
__global__ __launch_bounds__(256) void k_cand_sort(const i32 *off, i32 *list, unsigned char *crit, i64 nb, int packed)
{
    const i64 b = (i64)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    cand_sort_bin(list + off[b], crit + off[b], off[b + 1] - off[b], packed);
}

}  // namespace

// Builds the table for static displacements up to `displacement` with bins of about `bin_target` Angstrom; the
// table stays on the device (*d_off [nb+1], *d_list).  W = widest bin, mean = landmarks per bin; *meta: what
// sit_candidate_table reports about it.
int sit_build_candidates(sit_ctx *c, double displacement, double bin_target, i32 **d_off, i32 **d_list,
                         unsigned char **d_crit, int G_out[3], i64 *W, double *mean, CandMeta *meta)
{
    CandArgs a;
    meta->valid = false;               // G_out and *d_off change below: a build that fails leaves nothing to read back
    cand_setup(a, c->pbc.cm, c->pbc.ci, displacement, bin_target);     // grid, perpendicular heights, covering radius
    const i64 nb = a.nb;
    for (int i = 0; i < 3; i++) G_out[i] = a.G[i];
    a.ref_static = c->d_ref_static; a.verts = c->d_verts; a.vcd = c->d_vcd;
    a.D = c->D; a.Vp = c->Vp; a.rz = c->rz;
    int rc;
    if ((rc = dev_alloc(c, d_off, nb + 1))) return rc;
    i32 *cursor = nullptr, *stats = nullptr;
    if ((rc = dev_alloc(c, &cursor, nb + 4))) return rc;
    stats = cursor + nb;
    HIP_TRY(c, hipMemsetAsync(*d_off, 0, (size_t)(nb + 1) * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(cursor, 0, (size_t)(nb + 4) * 4, c->stream));
    a.cnt = *d_off; a.cursor = cursor; a.list = nullptr;
    k_cand_pass<false><<<dim3((unsigned)c->D), dim3(256), 0, c->stream>>>(a);
    k_cand_scan<<<dim3(1), dim3(1024), 0, c->stream>>>(*d_off, nb, stats);
    HIP_TRY(c, hipGetLastError());
    i32 hs[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(hs, stats, 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const i64 total = (i64)hs[1] + ((i64)hs[2] << 31);
    if (total > 2000000000LL) { sit_dfree(c, cursor); c->msg = "candidate table too large"; return SIT_ERR_CAPACITY; }
    if ((rc = dev_alloc(c, d_list, total > 0 ? total : 1))) { sit_dfree(c, cursor); return rc; }
    if ((rc = dev_alloc(c, d_crit, total > 0 ? total : 1))) { sit_dfree(c, cursor); return rc; }
    a.list = *d_list;
    k_cand_pass<true><<<dim3((unsigned)c->D), dim3(256), 0, c->stream>>>(a);
    k_cand_sort<<<dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream>>>(*d_off, *d_list, *d_crit, nb, c->D < (1LL << 24) ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sit_dfree(c, cursor);
    *W = hs[0] > 0 ? hs[0] : 1;
    *mean = (double)total / (double)nb;
    meta->displacement = displacement; meta->rb = a.rb; meta->total = total; meta->valid = true;
    c->table_gen++;
    return SIT_OK;
}

// Diagnostic read-back of a built table (include/sitator_hip.h); nowhere near the hot path.
extern "C" int sit_candidate_table(sit_ctx *c, int which, int32_t *G3, double *displacement, double *rb, int64_t *total,
                                   int64_t off_cap, int32_t *off, int64_t list_cap, int32_t *list, uint8_t *crit)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, which == 0 || which == 1, "sit_candidate_table: which must be 0 (loose) or 1 (tight)");
    SIT_REQUIRE(c, c->d_bin_off && c->S > 0, "sit_candidate_table: no basis set");
    if (which == 1) SIT_REQUIRE(c, c->tight_valid && c->d_tbin_off, "sit_candidate_table: no tight table (it is built by the first sit_fill over the frames of a basis)");
    HIP_TRY(c, hipSetDevice(c->device));
    const int *G = which ? c->tG : c->G;
    const CandMeta &m = c->cand_meta[which];
    SIT_REQUIRE(c, m.valid, "sit_candidate_table: the last build of that table failed");
    const i64 nb = (i64)G[0] * G[1] * G[2];
    if (G3) for (int i = 0; i < 3; i++) G3[i] = G[i];
    if (displacement) *displacement = m.displacement;
    if (rb) *rb = m.rb;
    if (total) *total = m.total;
    SIT_REQUIRE(c, !off || off_cap >= nb + 1, "sit_candidate_table: off_cap below bins + 1");
    SIT_REQUIRE(c, (!list && !crit) || list_cap >= m.total, "sit_candidate_table: list_cap below the entry count");
    if (off) HIP_TRY(c, hipMemcpyAsync(off, which ? c->d_tbin_off : c->d_bin_off, (size_t)(nb + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (list && m.total > 0) HIP_TRY(c, hipMemcpyAsync(list, which ? c->d_tbin_list : c->d_bin_list, (size_t)m.total * 4, hipMemcpyDeviceToHost, c->stream));
    if (crit && m.total > 0) HIP_TRY(c, hipMemcpyAsync(crit, which ? c->d_tbin_crit : c->d_bin_crit, (size_t)m.total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}
