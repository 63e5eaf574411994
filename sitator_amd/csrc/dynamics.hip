// The steps either side of the landmark path, on the device-resident label array:
//   jump detection                           SiteTrajectory.py:307-373
//   JumpAnalysis.run                         dynamics/JumpAnalysis.py:27-135
//   SiteTrajectory.assign_to_last_known_site SiteTrajectory.py:235-304
//   ReplaceUnassignedPositions.run           dynamics/ReplaceUnassignedPositions.py:90-117
//   SmoothSiteTrajectory.running_windowed_mode   dynamics/SmoothSiteTrajectory.pyx:79-111
//   RecenterTrajectory.run                   util/RecenterTrajectory.pyx:14-100
// The first four are per-ion scans along the frames in chunks (the scheme, the summary and the state transitions:
// label_scan.h): k_label_chunk_summary for all of them, then per scan a carry kernel and a replay kernel.
#include <cmath>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "sit_internal.h"
#include "label_scan.h"

// Step (1) of every scan.  Grid (chunks, ceil(M / 64)).
__global__ __launch_bounds__(64) void k_label_chunk_summary(const i64 *labels, i64 F, i64 M, int all_known, ChunkSummary *out)
{
    const i64 c = blockIdx.x, j = (i64)blockIdx.y * 64 + threadIdx.x;
    if (j >= M) return;
    out[c * M + j] = ls_summarise(labels + c * LS_CHUNK * M + j, M, ls_chunk_len(c, F), all_known != 0);
}

// ---- jump detection (SiteTrajectory.py:307-329) ----------------------------------------------------------
// A forward fill of the last known site per ion; the replay reports the jumps as an [F, M] source array and/or as records.
#define JUMP_NONE ((i64)0x8000000000000000ull)                   // sit_jump_sources: "no jump at this frame"

__global__ void k_jump_chunk_carry(const i64 *labels, i64 F, i64 M, i64 nch, const i64 *last_in, const ChunkSummary *sum,
                                   i64 *carry, i64 *last_out)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    i64 last = last_in ? last_in[j] : (F > 0 ? labels[j] : -1);       // last_known = traj[0] (:312)
    for (i64 c = 0; c < nch; c++) {
        carry[c * M + j] = last;
        jump_advance(last, sum[c * M + j]);
    }
    last_out[j] = last;
}

// (Frame 0 of a context without carried-in state only defines the state: the carry starts from its label, no jump.)
__global__ __launch_bounds__(64) void k_jump_emit(const i64 *labels, i64 F, i64 M, int unknown_as_jump, const i64 *carry,
                                                  i64 *from, i64 *rec, u64 *counter, i64 max_rec)
{
    const i64 c = blockIdx.x, j = (i64)blockIdx.y * 64 + threadIdx.x;
    if (j >= M) return;
    const i64 f0 = c * LS_CHUNK, f1 = f0 + ls_chunk_len(c, F);
    i64 last = carry[c * M + j];
    for (i64 f = f0; f < f1; f++) {
        const i64 cur = labels[f * M + j];
        const i64 was = last;
        const bool jumped = jump_step(last, cur, unknown_as_jump != 0);
        if (from) from[f * M + j] = jumped ? was : JUMP_NONE;
        if (rec && jumped) {
            const u64 slot = atomicAdd(counter, 1ull);
            if ((i64)slot < max_rec) { rec[4 * slot] = f; rec[4 * slot + 1] = j; rec[4 * slot + 2] = was; rec[4 * slot + 3] = cur; }
        }
    }
}

static int jump_scan(sit_ctx *c, int unknown_as_jump, const i64 *last_known_in, const ScanScratch<i64> &s, i64 *dfrom, i64 *drec,
                     i64 max_rec, u64 *dcounter)
{
    const i64 M = c->M, F = c->F, nch = ls_chunks(F);
    if (last_known_in) HIP_TRY(c, hipMemcpyAsync(s.in0, last_known_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    if (dcounter) HIP_TRY(c, hipMemsetAsync(dcounter, 0, 8, c->stream));
    const unsigned gy = (unsigned)((M + 63) / 64);
    if (nch > 0) k_label_chunk_summary<<<dim3((unsigned)nch, gy), dim3(64), 0, c->stream>>>(c->d_labels, F, M, unknown_as_jump, s.sum);
    k_jump_chunk_carry<<<dim3(gy), dim3(64), 0, c->stream>>>(c->d_labels, F, M, nch, last_known_in ? s.in0 : nullptr, s.sum,
                                                            s.carry, s.out0);
    if (nch > 0) k_jump_emit<<<dim3((unsigned)nch, gy), dim3(64), 0, c->stream>>>(c->d_labels, F, M, unknown_as_jump, s.carry,
                                                                               dfrom, drec, dcounter, max_rec);
    HIP_TRY(c, hipGetLastError());
    return SIT_OK;
}

extern "C" int sit_jump_sources(sit_ctx *c, int unknown_as_jump, const i64 *last_known_in, i64 *from, i64 *last_known_out)
{
    if (!c || !from) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_jump_sources: assignments needed");
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 N = c->N, M = c->M, nch = ls_chunks(c->F);
    ScanScratch<i64> s;
    i64 *dfrom;
    int rc = carve_scratch(c, [&](Carve &cv) { s.lay(cv, M, nch); dfrom = cv.take<i64>(N); });
    if (rc) return rc;
    if ((rc = jump_scan(c, unknown_as_jump, last_known_in, s, dfrom, nullptr, 0, nullptr))) return rc;
    if (N > 0) HIP_TRY(c, hipMemcpyAsync(from, dfrom, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    if (last_known_out) HIP_TRY(c, hipMemcpyAsync(last_known_out, s.out0, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

extern "C" int sit_jump_list(sit_ctx *c, int unknown_as_jump, const i64 *last_known_in, i64 max_records, i64 *records,
                             i64 *n_records, i64 *last_known_out)
{
    if (!c || !n_records || (max_records > 0 && !records)) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid && max_records >= 0, "sit_jump_list: assignments needed");
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 M = c->M, nch = ls_chunks(c->F);
    ScanScratch<i64> s;
    i64 *drec;
    u64 *dcount;
    int rc = carve_scratch(c, [&](Carve &cv) { s.lay(cv, M, nch); drec = cv.take<i64>(4 * max_records); dcount = cv.take<u64>(1); });
    if (rc) return rc;
    if ((rc = jump_scan(c, unknown_as_jump, last_known_in, s, nullptr, drec, max_records, dcount))) return rc;
    u64 n = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, dcount, 8, hipMemcpyDeviceToHost, c->stream));
    if (last_known_out) HIP_TRY(c, hipMemcpyAsync(last_known_out, s.out0, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_records = (i64)n;
    const i64 got = (i64)n < max_records ? (i64)n : max_records;
    if (got > 0) {
        HIP_TRY(c, hipMemcpyAsync(records, drec, (size_t)got * 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return SIT_OK;
}

// ---- JumpAnalysis --------------------------------------------------------------------------------------
// Pass 1: the forward-filled state machine of JumpAnalysis.py:46-92 per ion, frames in order:
//   jfrom = last_known, jto = frame value after re-assigning unassigned to last_known (or -1 when either is
//   unknown), jtime = time_at_current if the ion jumped this frame else 0.
// The state (last known site, time at it) at every chunk's start; the final state goes to last_out / tac_out.
__global__ void k_ja_chunk_carry(const i64 *labels, i64 F, i64 M, i64 nch, const i64 *last_in, const i64 *tac_in,
                                 const ChunkSummary *sum, JaState *carry, i64 *last_out, i64 *tac_out)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    JaState s = last_in ? JaState{last_in[j], tac_in[j]} : JaState{F > 0 ? labels[j] : -1, 1};   // :46-49
    for (i64 c = 0; c < nch; c++) {
        carry[c * M + j] = s;
        ja_advance(s, sum[c * M + j], ls_chunk_len(c, F));
    }
    last_out[j] = s.last; tac_out[j] = s.tac;
}

__global__ __launch_bounds__(64) void k_ja_chunk_replay(const i64 *labels, i64 F, i64 M, const JaState *carry,
                                                        i32 *jfrom, i32 *jto, i32 *jtime, u64 *n_problems)
{
    const i64 c = blockIdx.x, j = (i64)blockIdx.y * 64 + threadIdx.x;
    u64 problems = 0;
    if (j < M) {
        const i64 f0 = c * LS_CHUNK, f1 = f0 + ls_chunk_len(c, F);
        JaState s = carry[c * M + j];
        for (i64 f = f0; f < f1; f++) {
            const JaStep o = ja_step(s, labels[f * M + j]);
            jfrom[f * M + j] = o.from; jto[f * M + j] = o.to; jtime[f * M + j] = o.time;
            problems += o.problem;
        }
    }
    for (int off = 32; off > 0; off >>= 1) problems += __shfl_down(problems, off);
    if (threadIdx.x == 0 && problems) atomicAdd(n_problems, problems);
}

// Pass 2 (frames in parallel): numpy's fancy-index "+=" semantics of :72-86 -- within ONE frame duplicate
// indices count once, and for the summed jump times the LAST duplicate's value is the one added.
// A site index beyond the K x K tables (labels a caller built or edited: the reference's fancy indexing raises there,
// dynamics/JumpAnalysis.py:75-88) is not applied; the largest such index + 1 goes to *oob and the call fails with it.
__global__ __launch_bounds__(256) void k_ja_accumulate(const i32 *jfrom, const i32 *jto, const i32 *jtime, i64 F, i64 M, i64 K,
                                                       double *n_ij, double *tsum, u64 *tn, u64 *total_time, u64 *oob)
{
    const i64 f = blockIdx.x;
    const i32 *pf = jfrom + f * M, *pt = jto + f * M, *pm = jtime + f * M;
    for (i64 j = threadIdx.x; j < M; j += blockDim.x) {
        const i32 to = pt[j], from = pf[j];
        if (to < 0) continue;
        if (to >= K || from >= K) { atomicMax(oob, (u64)(to > from ? to : from) + 1ull); continue; }
        bool first_to = true, first_pair = true, last_jump_pair = pm[j] > 0;
        for (i64 q = 0; q < j; q++) {
            if (pt[q] == to) { first_to = false; if (pf[q] == from) { first_pair = false; break; } }
        }
        if (first_pair && !first_to) { /* same `to`, different `from`: fine */ }
        if (first_to) atomicAdd(&total_time[to], 1ull);                         // :71
        if (first_pair) unsafeAtomicAdd(&n_ij[(i64)from * K + to], 1.0);        // :76
        if (last_jump_pair) {
            for (i64 q = j + 1; q < M; q++)
                if (pm[q] > 0 && pt[q] == to && pf[q] == from) { last_jump_pair = false; break; }
            if (last_jump_pair) {                                               // :84-85
                unsafeAtomicAdd(&tsum[(i64)from * K + to], (double)pm[j]);
                atomicAdd(&tn[(i64)from * K + to], 1ull);
            }
        }
    }
}

extern "C" int sit_jump_analysis(sit_ctx *c, i64 K, const i64 *last_known_in, const i64 *time_at_current_in,
                                 double *n_ij, double *time_sum, i64 *time_n, i64 *total_time,
                                 i64 *n_problems, i64 *last_known_out, i64 *time_at_current_out)
{
    if (!c || !n_ij || !time_sum || !time_n || !total_time || !n_problems) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid && K > 0, "sit_jump_analysis: assignments needed");
    SIT_REQUIRE(c, (last_known_in == nullptr) == (time_at_current_in == nullptr), "sit_jump_analysis: halo arrays come in pairs");
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 N = c->N, M = c->M, F = c->F, nch = ls_chunks(F);
    const i64 nacc = 3 * K * K + K + 2;      // n_ij, time sum, time n [K, K]; total time [K]; problems, largest out-of-range site index + 1
    ScanScratch<JaState> s;
    u64 *d_acc;
    i32 *d_from, *d_to, *d_time;
    int rc = carve_scratch(c, [&](Carve &cv) {
        s.lay(cv, M, nch); d_acc = cv.take<u64>(nacc); d_from = cv.take<i32>(N); d_to = cv.take<i32>(N); d_time = cv.take<i32>(N);
    });
    if (rc) return rc;
    double *d_nij = (double *)d_acc, *d_ts = d_nij + K * K;
    u64 *d_tn = d_acc + 2 * K * K, *d_tt = d_tn + K * K, *d_np = d_tt + K;
    HIP_TRY(c, hipMemsetAsync(d_acc, 0, (size_t)nacc * 8, c->stream));
    if (last_known_in) {
        HIP_TRY(c, hipMemcpyAsync(s.in0, last_known_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(s.in1, time_at_current_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    }
    const dim3 cgrid((unsigned)(nch > 0 ? nch : 1), (unsigned)((M + 63) / 64));
    if (nch > 0) k_label_chunk_summary<<<cgrid, dim3(64), 0, c->stream>>>(c->d_labels, F, M, 0, s.sum);
    k_ja_chunk_carry<<<dim3((unsigned)((M + 63) / 64)), dim3(64), 0, c->stream>>>(
        c->d_labels, F, M, nch, last_known_in ? s.in0 : nullptr, last_known_in ? s.in1 : nullptr, s.sum, s.carry, s.out0, s.out1);
    if (nch > 0) k_ja_chunk_replay<<<cgrid, dim3(64), 0, c->stream>>>(c->d_labels, F, M, s.carry, d_from, d_to, d_time, d_np);
    if (F > 0) k_ja_accumulate<<<dim3((unsigned)F), dim3(256), 0, c->stream>>>(d_from, d_to, d_time, F, M, K, d_nij, d_ts, d_tn, d_tt, d_np + 1);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(n_ij, d_nij, (size_t)(K * K) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(time_sum, d_ts, (size_t)(K * K) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(time_n, d_tn, (size_t)(K * K) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(total_time, d_tt, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    u64 *h_np = (u64 *)c->h_pinned;                             // [0] problems, [1] largest out-of-range site index + 1
    HIP_TRY(c, hipMemcpyAsync(h_np, d_np, 16, hipMemcpyDeviceToHost, c->stream));
    if (last_known_out) HIP_TRY(c, hipMemcpyAsync(last_known_out, s.out0, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    if (time_at_current_out) HIP_TRY(c, hipMemcpyAsync(time_at_current_out, s.out1, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_problems = (i64)h_np[0];
    return label_status(c, "sit_jump_analysis", h_np[1], 0, K);
}

// ---- assign_to_last_known_site (SiteTrajectory.py:235-304) -----------------------------------------------
// Rewrites the device labels in place.  frame_max[f] = max over ions of the time an ion had been unknown when it
// became known again at frame f (for the reference's max statistic).
__global__ void k_alk_chunk_carry(i64 F, i64 M, i64 nch, const i64 *last_in, const i64 *tu_in, const ChunkSummary *sum,
                                  AlkState *carry, i64 *last_out, i64 *tu_out)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    AlkState s = {last_in ? last_in[j] : -1, tu_in ? tu_in[j] : 0};
    for (i64 c = 0; c < nch; c++) {
        carry[c * M + j] = s;
        alk_advance(s, sum[c * M + j], ls_chunk_len(c, F));
    }
    last_out[j] = s.last; tu_out[j] = s.tu;
}

__global__ __launch_bounds__(64) void k_alk_chunk_replay(i64 *labels, i64 F, i64 M, i64 threshold, const AlkState *carry,
                                                         i32 *frame_max, u64 *stats)
{
    const i64 c = blockIdx.x, j = (i64)blockIdx.y * 64 + threadIdx.x;
    u64 sum_t = 0, n_t = 0, reassigned = 0;
    if (j < M) {
        const i64 f0 = c * LS_CHUNK, f1 = f0 + ls_chunk_len(c, F);
        AlkState s = carry[c * M + j];
        for (i64 f = f0; f < f1; f++) {
            const AlkStep o = alk_step(s, labels[f * M + j], threshold);
            if (o.ended) { sum_t += (u64)o.ended; n_t++; atomicMax(&frame_max[f], (i32)o.ended); }   // :263-271
            if (o.reassign) { labels[f * M + j] = s.last; reassigned++; }                            // :275-278
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum_t += __shfl_down(sum_t, off); n_t += __shfl_down(n_t, off); reassigned += __shfl_down(reassigned, off);
    }
    if (threadIdx.x == 0) {
        if (sum_t) atomicAdd(&stats[0], sum_t);
        if (n_t) atomicAdd(&stats[1], n_t);
        if (reassigned) atomicAdd(&stats[2], reassigned);
    }
}

extern "C" int sit_assign_last_known(sit_ctx *c, i64 frame_threshold, const i64 *last_known_in, const i64 *time_unknown_in,
                                     i64 *labels_out, i32 *frame_max, i64 *stats3, i64 *last_known_out, i64 *time_unknown_out)
{
    if (!c || !stats3 || !frame_max) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_assign_last_known: assignments needed");
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 M = c->M, F = c->F, N = c->N, nch = ls_chunks(F);
    const i64 nfm = F > 0 ? F : 1;
    ScanScratch<AlkState> s;
    u64 *d_st;
    i32 *d_fm;
    int rc = carve_scratch(c, [&](Carve &cv) { s.lay(cv, M, nch); d_st = cv.take<u64>(3); d_fm = cv.take<i32>(nfm); });
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(d_st, 0, 24, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_fm, 0, (size_t)nfm * 4, c->stream));
    if (last_known_in) HIP_TRY(c, hipMemcpyAsync(s.in0, last_known_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    if (time_unknown_in) HIP_TRY(c, hipMemcpyAsync(s.in1, time_unknown_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    const dim3 cgrid((unsigned)(nch > 0 ? nch : 1), (unsigned)((M + 63) / 64));
    if (nch > 0) k_label_chunk_summary<<<cgrid, dim3(64), 0, c->stream>>>(c->d_labels, F, M, 0, s.sum);
    k_alk_chunk_carry<<<dim3((unsigned)((M + 63) / 64)), dim3(64), 0, c->stream>>>(
        F, M, nch, last_known_in ? s.in0 : nullptr, time_unknown_in ? s.in1 : nullptr, s.sum, s.carry, s.out0, s.out1);
    c->labels_gen++;                                         // the replay rewrites the resident labels in place
    if (nch > 0) k_alk_chunk_replay<<<cgrid, dim3(64), 0, c->stream>>>(c->d_labels, F, M, frame_threshold, s.carry, d_fm, d_st);
    HIP_TRY(c, hipGetLastError());
    u64 st[3];
    HIP_TRY(c, hipMemcpyAsync(st, d_st, 24, hipMemcpyDeviceToHost, c->stream));
    if (F > 0) HIP_TRY(c, hipMemcpyAsync(frame_max, d_fm, (size_t)F * 4, hipMemcpyDeviceToHost, c->stream));
    if (labels_out && N > 0) HIP_TRY(c, hipMemcpyAsync(labels_out, c->d_labels, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    if (last_known_out) HIP_TRY(c, hipMemcpyAsync(last_known_out, s.out0, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    if (time_unknown_out) HIP_TRY(c, hipMemcpyAsync(time_unknown_out, s.out1, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stats3[0] = (i64)st[0]; stats3[1] = (i64)st[1]; stats3[2] = (i64)st[2];
    return SIT_OK;
}

// ---- ReplaceUnassignedPositions (dynamics/ReplaceUnassignedPositions.py:90-117) ---------------------------
// Every unknown frame of an ion needs the nearest known label BEFORE it and the nearest AFTER it: the carry chains the
// summaries forwards and backwards.  The resident labels are only read.
// carry_before[c]: the label a run that starts chunk c has before it; carry_after[c] / carry_end[c]: the label after a
// run that reaches the end of chunk c and the (local) frame that label stands at (F: none).  ends[0..M) / ends[M..2M):
// first and last known label of the ion in these frames (INT64_MIN: none) - without the values carried in.
__global__ void k_rup_chunk_carry(i64 F, i64 M, i64 nch, const i64 *before_in, const i64 *after_in, const ChunkSummary *sum,
                                  i64 *carry_before, i64 *carry_after, i64 *carry_end, i64 *ends)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    i64 before = before_in ? before_in[j] : -1, after = after_in ? after_in[j] : -1, end = F;
    i64 first = INT64_MIN, last = INT64_MIN;
    for (i64 c = 0; c < nch; c++) {
        carry_before[c * M + j] = before;
        jump_advance(before, sum[c * M + j]);
        if (sum[c * M + j].first_pos >= 0) last = sum[c * M + j].last;
    }
    for (i64 c = nch - 1; c >= 0; c--) {
        carry_after[c * M + j] = after; carry_end[c * M + j] = end;
        rup_back_advance(after, end, sum[c * M + j], c * LS_CHUNK);
        if (sum[c * M + j].first_pos >= 0) first = sum[c * M + j].first;
    }
    ends[j] = first; ends[M + j] = last;
}

// mode 0: forwards, every unknown frame takes `before`; mode 1: backwards, it takes `after`
__global__ __launch_bounds__(64) void k_rup_chunk_replay(const i64 *labels, i64 F, i64 M, int mode, const i64 *carry_before,
                                                         const i64 *carry_after, i64 *out)
{
    const i64 c = blockIdx.x, j = (i64)blockIdx.y * 64 + threadIdx.x;
    if (j >= M) return;
    const i64 f0 = c * LS_CHUNK, f1 = f0 + ls_chunk_len(c, F);
    i64 fill = (mode == 0 ? carry_before : carry_after)[c * M + j];
    for (i64 i = 0; i < f1 - f0; i++) {
        const i64 f = mode == 0 ? f0 + i : f1 - 1 - i;
        jump_step(fill, labels[f * M + j], false);
        out[f * M + j] = fill;
    }
}

// The maximal runs of unknown frames that START in chunk c of ion j.  EMIT = false counts them and the positions they
// ask for (runs whose two sides are known and differ); EMIT = true writes them from the offsets the scan made of the
// counts.  A run that reaches the chunk's end takes its end and `after` from the backward carry.
template <bool EMIT>
__global__ __launch_bounds__(64) void k_rup_runs(const i64 *labels, i64 F, i64 M, i64 frame0, const i64 *carry_before,
                                                 const i64 *carry_after, const i64 *carry_end, i64 *n_runs, i64 *n_pos,
                                                 i64 *rec)
{
    const i64 c = blockIdx.x, j = (i64)blockIdx.y * 64 + threadIdx.x;
    if (j >= M) return;
    const i64 f0 = c * LS_CHUNK, f1 = f0 + LS_CHUNK < F ? f0 + LS_CHUNK : F;
    i64 before = carry_before[c * M + j];
    i64 runs = EMIT ? n_runs[c * M + j] : 0, pos = EMIT ? n_pos[c * M + j] : 0;
    bool open = f0 > 0 && labels[(f0 - 1) * M + j] == -1;        // a run of an earlier chunk is still going
    i64 start = -1;
    for (i64 f = f0; f <= f1; f++) {
        const i64 cur = f < f1 ? labels[f * M + j] : 0;
        if (f < f1 && cur == -1) {
            if (!open && start < 0) start = f;
            continue;
        }
        if (start >= 0) {
            const i64 end = f < f1 ? f : carry_end[c * M + j];
            const i64 after = f < f1 ? cur : carry_after[c * M + j];
            const bool decide = before >= 0 && after >= 0 && before != after;
            if (EMIT) {
                i64 *r = rec + 6 * runs;
                r[0] = j; r[1] = frame0 + start; r[2] = frame0 + end; r[3] = before; r[4] = after; r[5] = decide ? pos : -1;
            }
            runs++;
            if (decide) pos += end - start;
            start = -1;
        }
        open = false;
        before = cur;
    }
    if (!EMIT) { n_runs[c * M + j] = runs; n_pos[c * M + j] = pos; }
}

// Exclusive prefix sums of the two count tables in ION-MAJOR order (item i = j * nch + c lives at [c * M + j]): the
// reference walks the ions, and the runs of an ion in frame order (:99-112).  One workgroup: the tables have F * M / LS_CHUNK
// entries.  totals[0], totals[1]: the sums.
__global__ __launch_bounds__(1024) void k_rup_scan(i64 *n_runs, i64 *n_pos, i64 M, i64 nch, i64 *totals)
{
    __shared__ i64 sr[1024], sp[1024];
    const i64 T = M * nch, per = (T + 1023) / 1024;
    const i64 i0 = (i64)threadIdx.x * per, i1 = i0 + per < T ? i0 + per : T;
    i64 r = 0, p = 0;
    for (i64 i = i0; i < i1; i++) { const i64 o = (i % nch) * M + i / nch; r += n_runs[o]; p += n_pos[o]; }
    sr[threadIdx.x] = r; sp[threadIdx.x] = p;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {                           // inclusive scan of the threads' sums
        const i64 ar = (int)threadIdx.x >= s ? sr[threadIdx.x - s] : 0, ap = (int)threadIdx.x >= s ? sp[threadIdx.x - s] : 0;
        __syncthreads();
        sr[threadIdx.x] += ar; sp[threadIdx.x] += ap;
        __syncthreads();
    }
    i64 br = sr[threadIdx.x] - r, bp = sp[threadIdx.x] - p;
    for (i64 i = i0; i < i1; i++) {
        const i64 o = (i % nch) * M + i / nch;
        const i64 nr = n_runs[o], np = n_pos[o];
        n_runs[o] = br; n_pos[o] = bp;
        br += nr; bp += np;
    }
    if (threadIdx.x == 1023) { totals[0] = sr[1023]; totals[1] = sp[1023]; }
}

// the two launches every entry point below starts with
static int rup_scan(sit_ctx *c, const i64 *before_in, const i64 *after_in, const RupScratch &s)
{
    const i64 M = c->M, F = c->F, nch = ls_chunks(F);
    if (before_in) {
        HIP_TRY(c, hipMemcpyAsync(s.before_in, before_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(s.after_in, after_in, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    }
    const unsigned gy = (unsigned)((M + 63) / 64);
    if (nch > 0) k_label_chunk_summary<<<dim3((unsigned)nch, gy), dim3(64), 0, c->stream>>>(c->d_labels, F, M, 0, s.sum);
    k_rup_chunk_carry<<<dim3(gy), dim3(64), 0, c->stream>>>(F, M, nch, before_in ? s.before_in : nullptr,
                                                          before_in ? s.after_in : nullptr, s.sum, s.cb, s.ca, s.ce, s.ends);
    HIP_TRY(c, hipGetLastError());
    return SIT_OK;
}

extern "C" int sit_label_ends(sit_ctx *c, i64 *first_known, i64 *last_known)
{
    if (!c || !first_known || !last_known) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_label_ends: assignments needed");
    const i64 M = c->M, nch = ls_chunks(c->F);
    if (M == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    RupScratch s;
    int rc = carve_scratch(c, [&](Carve &cv) { s.lay(cv, M, nch); });
    if (rc) return rc;
    if ((rc = rup_scan(c, nullptr, nullptr, s))) return rc;
    HIP_TRY(c, hipMemcpyAsync(first_known, s.ends, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(last_known, s.ends + M, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

extern "C" int sit_replace_unassigned(sit_ctx *c, int mode, const i64 *before_in, const i64 *after_in, i64 *labels_out)
{
    if (!c || !labels_out) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_replace_unassigned: assignments needed");
    SIT_REQUIRE(c, mode == 0 || mode == 1, "sit_replace_unassigned: mode is 0 (last known) or 1 (next known)");
    SIT_REQUIRE(c, (before_in == nullptr) == (after_in == nullptr), "sit_replace_unassigned: the carried-in arrays come in pairs");
    const i64 M = c->M, F = c->F, N = c->N, nch = ls_chunks(F);
    if (N == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    RupScratch s;
    i64 *d_out;
    int rc = carve_scratch(c, [&](Carve &cv) { s.lay(cv, M, nch); d_out = cv.take<i64>(N); });
    if (rc) return rc;
    if ((rc = rup_scan(c, before_in, after_in, s))) return rc;
    k_rup_chunk_replay<<<dim3((unsigned)nch, (unsigned)((M + 63) / 64)), dim3(64), 0, c->stream>>>(c->d_labels, F, M, mode, s.cb,
                                                                                                 s.ca, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(labels_out, d_out, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

extern "C" int sit_unknown_runs(sit_ctx *c, const i64 *before_in, const i64 *after_in, i64 max_records, i64 *records,
                                i64 *n_records, i64 *n_positions)
{
    if (!c || !n_records || !n_positions || (max_records > 0 && !records)) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid && max_records >= 0, "sit_unknown_runs: assignments needed");
    SIT_REQUIRE(c, (before_in == nullptr) == (after_in == nullptr), "sit_unknown_runs: the carried-in arrays come in pairs");
    const i64 M = c->M, F = c->F, nch = ls_chunks(F);
    *n_records = 0; *n_positions = 0;
    if (c->N == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    RupScratch s;
    i64 *d_nr, *d_np, *d_tot, *d_rec;
    int rc = carve_scratch(c, [&](Carve &cv) {
        s.lay(cv, M, nch);
        d_nr = cv.take<i64>(nch * M); d_np = cv.take<i64>(nch * M); d_tot = cv.take<i64>(2); d_rec = cv.take<i64>(6 * max_records);
    });
    if (rc) return rc;
    if ((rc = rup_scan(c, before_in, after_in, s))) return rc;
    const dim3 cgrid((unsigned)nch, (unsigned)((M + 63) / 64));
    k_rup_runs<false><<<cgrid, dim3(64), 0, c->stream>>>(c->d_labels, F, M, c->frame0, s.cb, s.ca, s.ce, d_nr, d_np, nullptr);
    k_rup_scan<<<dim3(1), dim3(1024), 0, c->stream>>>(d_nr, d_np, M, nch, d_tot);
    HIP_TRY(c, hipGetLastError());
    i64 *h_tot = (i64 *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_tot, d_tot, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_records = h_tot[0]; *n_positions = h_tot[1];
    if (h_tot[0] == 0 || h_tot[0] > max_records) return SIT_OK;
    k_rup_runs<true><<<cgrid, dim3(64), 0, c->stream>>>(c->d_labels, F, M, c->frame0, s.cb, s.ca, s.ce, d_nr, d_np, d_rec);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(records, d_rec, (size_t)h_tot[0] * 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

// The closer-site strategy (:56-87) on records the CALLER hands in.  k_rc_check looks at every record before anything is
// indexed with it: flags[0] = records that break a bound, flags[1] = largest label >= K, + 1.
__global__ __launch_bounds__(256) void k_rc_check(const i64 *rec, i64 n, i64 F, i64 M, i64 frame0, i64 K, i64 n_positions, u64 *flags)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const i64 ion = rec[6 * r], start = rec[6 * r + 1], end = rec[6 * r + 2], before = rec[6 * r + 3], after = rec[6 * r + 4],
              off = rec[6 * r + 5];
    bool bad = ion < 0 || ion >= M || start < frame0 || start >= end || end > frame0 + F || before < -1 || after < -1;
    if (before >= K || after >= K) atomicMax(&flags[1], (u64)(before > after ? before : after) + 1ull);
    else if (!bad && before >= 0 && after >= 0 && before != after)
        bad = off < 0 || off > n_positions - (end - start);
    if (bad) atomicAdd(&flags[0], 1ull);
}

// Lane per (checked) record: a run whose two sides are the same site takes it; a run to decide marks its positions with
// its own number for k_rc_decide.  Only frames that ARE unknown in the resident labels are written.
__global__ __launch_bounds__(256) void k_rc_expand(const i64 *rec, i64 n, const i64 *labels, i64 M, i64 frame0, i64 *owner, i64 *out)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const i64 ion = rec[6 * r], start = rec[6 * r + 1] - frame0, end = rec[6 * r + 2] - frame0, before = rec[6 * r + 3],
              after = rec[6 * r + 4], off = rec[6 * r + 5];
    if (before < 0 || after < 0) return;
    if (before == after) {
        for (i64 f = start; f < end; f++)
            if (labels[f * M + ion] == -1) out[f * M + ion] = before;
    } else {
        for (i64 i = 0; i < end - start; i++) owner[off + i] = r;
    }
}

// Lane per (run, frame of the run) to decide: `before` if the position is strictly nearer to its centre, else `after`
__global__ __launch_bounds__(256) void k_rc_decide(Pbc P, const i64 *rec, const i64 *owner, i64 n_positions, const double *pos,
                                                   const double *centers, const i64 *labels, i64 M, i64 frame0, i64 *out)
{
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_positions) return;
    const i64 r = owner[p];
    if (r < 0) return;
    const i64 ion = rec[6 * r], before = rec[6 * r + 3], after = rec[6 * r + 4];
    const i64 f = rec[6 * r + 1] - frame0 + (p - rec[6 * r + 5]);
    if (labels[f * M + ion] != -1) return;
    const double x = pos[3 * p], y = pos[3 * p + 1], z = pos[3 * p + 2];
    const double db = dist_sw(P, x, y, z, centers[3 * before], centers[3 * before + 1], centers[3 * before + 2]);
    const double da = dist_sw(P, x, y, z, centers[3 * after], centers[3 * after + 1], centers[3 * after + 2]);
    out[f * M + ion] = db < da ? before : after;                  // :83-86
}

extern "C" int sit_replace_closer(sit_ctx *c, const i64 *records, i64 n, const double *centers, i64 K, const double *positions,
                                  i64 n_positions, i64 *labels_out)
{
    if (!c || !labels_out) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_replace_closer: assignments needed");
    SIT_REQUIRE(c, n >= 0 && K >= 0 && n_positions >= 0, "sit_replace_closer: negative count");
    SIT_REQUIRE(c, (n == 0 || records) && (K == 0 || centers) && (n_positions == 0 || positions), "sit_replace_closer: missing array");
    const i64 M = c->M, F = c->F, N = c->N;
    if (N == 0) {
        SIT_REQUIRE(c, n == 0, "sit_replace_closer: records for a context without frames");
        return SIT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    u64 *d_flags;
    i64 *d_out, *d_rec, *d_owner;
    double *d_cen, *d_pos;
    int rc = carve_scratch(c, [&](Carve &cv) {
        d_flags = cv.take<u64>(2); d_out = cv.take<i64>(N); d_rec = cv.take<i64>(6 * n); d_owner = cv.take<i64>(n_positions);
        d_cen = cv.take<double>(3 * K); d_pos = cv.take<double>(3 * n_positions);
    });
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_out, c->d_labels, (size_t)N * 8, hipMemcpyDeviceToDevice, c->stream));
    if (n > 0) {
        HIP_TRY(c, hipMemsetAsync(d_flags, 0, 16, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_rec, records, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
        k_rc_check<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(d_rec, n, F, M, c->frame0, K, n_positions, d_flags);
        HIP_TRY(c, hipGetLastError());
        u64 *h_flags = (u64 *)c->h_pinned;
        HIP_TRY(c, hipMemcpyAsync(h_flags, d_flags, 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if ((rc = label_status(c, "sit_replace_closer", h_flags[1], 0, K))) return rc;
        if (h_flags[0]) {
            char text[160];
            snprintf(text, sizeof(text), "sit_replace_closer: %llu records outside the context (ion, frames, sites or position offset)",
                     (unsigned long long)h_flags[0]);
            c->msg = text;
            return SIT_ERR_INVALID;
        }
        if (K > 0) HIP_TRY(c, hipMemcpyAsync(d_cen, centers, (size_t)K * 24, hipMemcpyHostToDevice, c->stream));
        if (n_positions > 0) {
            HIP_TRY(c, hipMemcpyAsync(d_pos, positions, (size_t)n_positions * 24, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemsetAsync(d_owner, 0xFF, (size_t)n_positions * 8, c->stream));
        }
        k_rc_expand<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(d_rec, n, c->d_labels, M, c->frame0, d_owner, d_out);
        if (n_positions > 0)
            k_rc_decide<<<dim3((unsigned)((n_positions + 255) / 256)), dim3(256), 0, c->stream>>>(
                c->pbc, d_rec, d_owner, n_positions, d_pos, d_cen, c->d_labels, M, c->frame0, d_out);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(labels_out, d_out, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

// ---- running windowed mode (dynamics/SmoothSiteTrajectory.pyx:79-111) -------------------------------------
// Lane per (frame, ion): mode of the window [frame - wleft, frame + wright) with the reference's tie rule
// (lowest site index wins, "unknown" = index 0 first); threshold on the multiplicity.
__global__ void k_running_mode(const i64 *traj, i64 *out, i64 F, i64 M, i64 wleft, i64 wright, i64 threshold, int replace_unknown)
{
    const i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= F * M) return;
    const i64 f = o / M, j = o - f * M;
    const i64 lo = f - wleft > 0 ? f - wleft : 0, hi = f + wright < F ? f + wright : F;
    i64 winner = -1, best = 0;
    for (i64 a = lo; a < hi; a++) {
        const i64 s = traj[a * M + j];
        bool seen = false;
        for (i64 b = lo; b < a; b++) if (traj[b * M + j] == s) { seen = true; break; }
        if (seen) continue;
        i64 cnt = 0;
        for (i64 b = a; b < hi; b++) cnt += traj[b * M + j] == s;
        if (cnt > best || (cnt == best && s < winner)) { best = cnt; winner = s; }
    }
    if (best == 0) winner = -1;
    out[o] = best >= threshold ? winner : (replace_unknown ? -1 : traj[o]);
}

// labels_hist: np.bincount(labels[labels >= 0], minlength = K) of a device label array (fill.hip)
int label_counts_of(sit_ctx *c, const i64 *d_labels, i64 N, i64 K, i64 *counts_host);

extern "C" int sit_running_mode(sit_ctx *c, i64 wleft, i64 wright, i64 threshold, int replace_unknown, i64 *out, i64 K,
                                i64 *counts)
{
    if (!c || !out) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid && wleft >= 0 && wright >= 0, "sit_running_mode: assignments needed");
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 N = c->N;
    if (N == 0) return SIT_OK;
    i64 *d_out;
    int rc = carve_scratch(c, [&](Carve &cv) { d_out = cv.take<i64>(N); });
    if (rc) return rc;
    k_running_mode<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream>>>(
        c->d_labels, d_out, c->F, c->M, wleft, wright, threshold, replace_unknown);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    if (counts && K > 0) return label_counts_of(c, d_out, N, K, counts);   // (synchronises)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

// ---- RecenterTrajectory (util/RecenterTrajectory.pyx:66-100) ------------------------------------------------
// Block per frame: com = sum_j (tmi * factor_j * mass_j) * x_ij, then x -= com (+ optional constant, the cell
// centroid of :57-58).  Fixed-shape tree reduction (deterministic; the reference sums left to right, the
// difference is O(1e-16) relative to the coordinates' magnitude).
__global__ __launch_bounds__(256) void k_recenter(double *arr, i64 A, const double *coef, double ax, double ay, double az)
{
    __shared__ double red[3][256];
    double *fr = arr + (i64)blockIdx.x * A * 3;
    double s0 = 0, s1 = 0, s2 = 0;
    for (i64 j = threadIdx.x; j < A; j += 256) {
        const double w = coef[j];
        s0 += w * fr[3 * j]; s1 += w * fr[3 * j + 1]; s2 += w * fr[3 * j + 2];
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int q = 0; q < 3; q++) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    const double c0 = red[0][0], c1 = red[1][0], c2 = red[2][0];
    for (i64 j = threadIdx.x; j < A; j += 256) {
        double x = fr[3 * j] - c0, y = fr[3 * j + 1] - c1, z = fr[3 * j + 2] - c2;
        fr[3 * j] = x + ax; fr[3 * j + 1] = y + ay; fr[3 * j + 2] = z + az;
    }
}

// total_mass_inverse and the per-atom coefficient exactly as :83-92 (left to right)
static std::vector<double> recenter_coef(i64 A, const double *masses, const double *factors)
{
    double tot = 0.0;
    for (i64 j = 0; j < A; j++) tot += factors[j] * masses[j];
    const double tmi = 1.0 / tot;
    std::vector<double> coef((size_t)A);
    for (i64 j = 0; j < A; j++) coef[(size_t)j] = tmi * factors[j] * masses[j];
    return coef;
}

extern "C" int sit_recenter(sit_ctx *c, double *arr, i64 F, i64 A, const double *masses, const double *factors, const double *add3)
{
    if (!c || !arr || !masses || !factors) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, F >= 0 && A > 0, "sit_recenter: bad shape");
    if (F == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const std::vector<double> coef = recenter_coef(A, masses, factors);
    double *d, *dc;
    int rc = carve_scratch(c, [&](Carve &cv) { d = cv.take<double>(F * A * 3); dc = cv.take<double>(A); });
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(d, arr, (size_t)(F * A) * 24, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dc, coef.data(), (size_t)A * 8, hipMemcpyHostToDevice, c->stream));
    k_recenter<<<dim3((unsigned)F), dim3(256), 0, c->stream>>>(d, A, dc, add3 ? add3[0] : 0.0, add3 ? add3[1] : 0.0, add3 ? add3[2] : 0.0);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(arr, d, (size_t)(F * A) * 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

// The same subtraction on the frames ALREADY RESIDENT for the landmark analysis (sit_set_frames), in place on the
// device: the pre-processing step of util/RecenterTrajectory.pyx:66-100 without the round trip of the trajectory over
// PCIe.  The caller's host array is not touched.
extern "C" int sit_recenter_resident(sit_ctx *c, const double *masses, const double *factors, const double *add3)
{
    if (!c || !masses || !factors) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, c->d_frames && c->frames_owned && c->A > 0, "sit_recenter_resident: no resident frames (sit_set_frames first)");
    if (c->F == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 A = c->A;
    const std::vector<double> coef = recenter_coef(A, masses, factors);
    double *dc;
    int rc = carve_scratch(c, [&](Carve &cv) { dc = cv.take<double>(A); });
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(dc, coef.data(), (size_t)A * 8, hipMemcpyHostToDevice, c->stream));
    k_recenter<<<dim3((unsigned)c->F), dim3(256), 0, c->stream>>>(c->d_frames, A, dc, add3 ? add3[0] : 0.0, add3 ? add3[1] : 0.0, add3 ? add3[2] : 0.0);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));         // coef lives on this stack frame
    c->rows_valid = false; c->assign_valid = false; c->labels_gen++; c->map_valid = false; c->tight_valid = false;
    return SIT_OK;
}
