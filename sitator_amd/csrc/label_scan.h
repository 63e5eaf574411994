// The per-ion scans along the frames of the label array (dynamics.hip), in a form the host compiler takes too
// (tests/test_label_scan.py runs them with g++ under ASan / UBSan, at any chunk length).
// Frames are cut into chunks of LS_CHUNK: (1) every (chunk, ion) summarises its chunk (ls_summarise), (2) one lane per
// ion chains the summaries into the state at every chunk's start (*_advance), (3) every (chunk, ion) replays its chunk
// from that state (*_step).  A label is KNOWN when it is not -1 (the jump scan with unknown_as_jump: always); a known
// label below -1 is known but not a site.
#pragma once

#include <stdint.h>

#include "scratch_carve.h"

#ifdef __HIPCC__
#define LS_HD __host__ __device__
#else
#define LS_HD
#endif

typedef int64_t i64;
typedef int32_t i32;

#define LS_CHUNK 256

LS_HD inline i64 ls_chunks(i64 F, i64 chunk = LS_CHUNK) { return (F + chunk - 1) / chunk; }
LS_HD inline i64 ls_chunk_len(i64 c, i64 F, i64 chunk = LS_CHUNK) { return c * chunk + chunk < F ? chunk : F - c * chunk; }

// One per (chunk, ion): the first and last known label and where they stand (first_pos < 0: the chunk has none), and the
// last position where two consecutive known labels INSIDE the chunk differ and both are sites (-1: none).
struct ChunkSummary {
    i64 first, last;
    i32 first_pos, last_pos, last_jump_pos, pad;
};

LS_HD inline ChunkSummary ls_summarise(const i64 *col, i64 stride, i64 len, bool all_known)
{
    ChunkSummary s = {0, 0, -1, -1, -1, 0};
    for (i64 p = 0; p < len; p++) {
        const i64 cur = col[p * stride];
        if (!all_known && cur == -1) continue;
        if (s.first_pos < 0) { s.first = cur; s.first_pos = (i32)p; }
        else if (cur != s.last && cur >= 0 && s.last >= 0) s.last_jump_pos = (i32)p;   // JumpAnalysis.py:68,:74: both known
        s.last = cur; s.last_pos = (i32)p;
    }
    return s;
}

// ---- jump detection (SiteTrajectory.py:307-329): the last known label.  Also `before` and both fills of ReplaceUnassignedPositions.
LS_HD inline void jump_advance(i64 &last, const ChunkSummary &s) { if (s.first_pos >= 0) last = s.last; }

// true: the ion jumped at this frame (from the `last` of before the call)
LS_HD inline bool jump_step(i64 &last, i64 cur, bool all_known)
{
    const bool known = all_known || cur != -1;
    const bool jumped = known && cur != last;
    if (known) last = cur;
    return jumped;
}

// ---- ReplaceUnassignedPositions backwards: the label after a run that reaches a chunk's end and its frame (f0: the chunk's first)
LS_HD inline void rup_back_advance(i64 &after, i64 &end, const ChunkSummary &s, i64 f0)
{
    if (s.first_pos >= 0) { after = s.first; end = f0 + s.first_pos; }
}

// ---- JumpAnalysis (dynamics/JumpAnalysis.py:46-92): (last known site, time at the current site)
struct JaState { i64 last, tac; };
struct JaStep { i32 from, to, time; bool problem; };

// whether the chunk's first known label is a jump depends on the carried-in site
LS_HD inline void ja_advance(JaState &s, const ChunkSummary &c, i64 len)
{
    i64 jp = c.last_jump_pos;
    if (c.first_pos >= 0) {
        if (s.last >= 0 && c.first >= 0 && c.first != s.last && jp < c.first_pos) jp = c.first_pos;
        s.last = c.last;
    }
    s.tac = jp >= 0 ? len - jp : s.tac + len;                    // :88-91: 1 after the jump frame, + 1 per frame
}

LS_HD inline JaStep ja_step(JaState &s, i64 cur)
{
    const bool unassigned = cur == -1;
    const i64 fr = unassigned ? s.last : cur;                    // :65-67
    const bool fknown = fr >= 0 && s.last >= 0;                  // :68
    const bool jumped = fknown && fr != s.last;                  // :74
    const JaStep o = {fknown ? (i32)s.last : -1, fknown ? (i32)fr : -1, jumped ? (i32)s.tac : 0, !fknown};
    s.tac = jumped ? 1 : s.tac + 1;                              // :88-91
    if (!unassigned) s.last = cur;                               // :94
    return o;
}

// ---- assign_to_last_known_site (SiteTrajectory.py:235-304): (last known site, frames unknown so far)
struct AlkState { i64 last, tu; };
struct AlkStep { i64 ended; bool reassign; };   // ended: the time unknown that ends at this frame (0: none); reassign: the frame takes s.last

LS_HD inline void alk_advance(AlkState &s, const ChunkSummary &c, i64 len)
{
    if (c.first_pos >= 0) { s.last = c.last; s.tu = len - 1 - c.last_pos; }
    else s.tu += len;
}

LS_HD inline AlkStep alk_step(AlkState &s, i64 cur, i64 threshold)
{
    AlkStep o = {0, false};
    if (cur != -1) { s.last = cur; o.ended = s.tu; s.tu = 0; }   // :261-273
    else { o.reassign = s.tu < threshold; s.tu++; }              // :275-279
    return o;
}

// ---- the scratch layouts of the scans (the carver: scratch_carve.h)
// What the three launches of a forward scan share: the state carried in and out per ion (the jump scan uses the first
// array of each), the summaries, and the state at every chunk's start (S: i64, JaState, AlkState).
template <class S>
struct ScanScratch {
    i64 *in0, *in1, *out0, *out1;
    ChunkSummary *sum;
    S *carry;
    void lay(Carve &cv, i64 M, i64 nch)
    {
        in0 = cv.take<i64>(M); in1 = cv.take<i64>(M); out0 = cv.take<i64>(M); out1 = cv.take<i64>(M);
        sum = cv.take<ChunkSummary>(nch * M); carry = cv.take<S>(nch * M);
    }
};

// The two-directional scan of ReplaceUnassignedPositions: carried-in before / after, the ion's first and last known label
// (ends[0..M) / ends[M..2M)), the summaries, `before` at every chunk's start, `after` / `end` at every chunk's end.
struct RupScratch {
    i64 *before_in, *after_in, *ends, *cb, *ca, *ce;
    ChunkSummary *sum;
    void lay(Carve &cv, i64 M, i64 nch)
    {
        before_in = cv.take<i64>(M); after_in = cv.take<i64>(M); ends = cv.take<i64>(2 * M); sum = cv.take<ChunkSummary>(nch * M);
        cb = cv.take<i64>(nch * M); ca = cv.take<i64>(nch * M); ce = cv.take<i64>(nch * M);
    }
};
