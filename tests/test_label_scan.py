"""CPU-only: the chunk algebra of the label scans (sitator_amd/csrc/label_scan.h: jump detection, JumpAnalysis,
assign_to_last_known_site, ReplaceUnassignedPositions) and their scratch layouts, compiled with the host compiler under
ASan / UBSan the way test_fill3_plan.py compiles the launch planner (the carver itself: test_scratch_carve.py).  The probe runs what the kernels of dynamics.hip
run - ls_summarise per (chunk, ion), the *_advance chain per ion, the *_step replay per (chunk, ion) - at ANY chunk
length, through pointers a Carve handed out over a heap buffer of exactly the size the same layout asked for, and next
to it a serial fold of the *_step functions from frame 0 (for the backward chain: from the last frame)."""
import os
import subprocess

import numpy as np
import pytest

from tests import replace_ref as R
from tests.test_gpu_label_kernels import make_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -(1 << 63)
SHAPES = [(1, 65), (2, 1), (255, 64), (256, 63), (257, 300)]
THRESHOLD = 3

# stdin, int64: F M chunk halo threshold, labels[F, M], with halo: jump last, ja last, ja tac, alk last, alk tu, rup before,
# rup after (M each).  stdout, int64: the arrays of `parse` below, in its order.
PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "label_scan.h"

static char *g_base;
static i64 g_used;

template <class Lay> static void carve(Lay lay)
{
    Carve size = {nullptr, 0};
    lay(size);
    g_used = size.used;
    g_base = (char *)malloc((size_t)g_used);            // exactly `used` bytes: ASan sees a write one byte beyond
    Carve cv = {g_base, 0};
    lay(cv);
    if (cv.used != size.used) { fprintf(stderr, "sizing and carving pass disagree\n"); exit(3); }
}
template <class T> static void inside(const T *p, i64 n)
{
    const char *q = (const char *)p;
    if (((size_t)q & 15) || q < g_base || q + n * (i64)sizeof(T) > g_base + g_used) { fprintf(stderr, "pointer outside its buffer\n"); exit(3); }
}
template <class S> static void inside(const ScanScratch<S> &s, i64 M, i64 nch)
{
    inside(s.in0, M); inside(s.in1, M); inside(s.out0, M); inside(s.out1, M); inside(s.sum, nch * M); inside(s.carry, nch * M);
}
static void put(const void *p, i64 n) { fwrite(p, 8, (size_t)n, stdout); }

int main()
{
    i64 h[5];
    if (fread(h, 8, 5, stdin) != 5) return 2;
    const i64 F = h[0], M = h[1], chunk = h[2], halo = h[3], threshold = h[4], nch = ls_chunks(F, chunk);
    std::vector<i64> lab((size_t)(F * M)), in((size_t)(7 * M));
    if (fread(lab.data(), 8, (size_t)(F * M), stdin) != (size_t)(F * M)) return 2;
    if (halo && fread(in.data(), 8, (size_t)(7 * M), stdin) != (size_t)(7 * M)) return 2;
    const i64 *hin[7];
    for (int q = 0; q < 7; q++) hin[q] = halo ? in.data() + q * M : nullptr;
    std::vector<i64> serial((size_t)(3 * nch * M + 2 * M));

    // ---- jump detection, both values of unknown_as_jump: carry, serial carry, last out, serial last out, from[F, M]
    for (int uaj = 0; uaj < 2; uaj++) {
        ScanScratch<i64> s;
        i64 *from;
        carve([&](Carve &cv) { s.lay(cv, M, nch); from = cv.take<i64>(F * M); });
        inside(s, M, nch); inside(from, F * M);
        for (i64 j = 0; j < M; j++) {
            for (i64 c = 0; c < nch; c++) s.sum[c * M + j] = ls_summarise(&lab[c * chunk * M + j], M, ls_chunk_len(c, F, chunk), uaj);
            i64 last = halo ? hin[0][j] : lab[j];
            for (i64 c = 0; c < nch; c++) { s.carry[c * M + j] = last; jump_advance(last, s.sum[c * M + j]); }
            s.out0[j] = last;
            for (i64 c = 0; c < nch; c++) {
                last = s.carry[c * M + j];
                for (i64 f = c * chunk; f < c * chunk + ls_chunk_len(c, F, chunk); f++) {
                    const i64 was = last;
                    from[f * M + j] = jump_step(last, lab[f * M + j], uaj) ? was : INT64_MIN;
                }
            }
            last = halo ? hin[0][j] : lab[j];
            for (i64 f = 0; f < F; f++) {
                if (f % chunk == 0) serial[f / chunk * M + j] = last;
                jump_step(last, lab[f * M + j], uaj);
            }
            serial[nch * M + j] = last;
        }
        put(s.carry, nch * M); put(serial.data(), nch * M); put(s.out0, M); put(&serial[nch * M], M); put(from, F * M);
        free(g_base);
    }

    // ---- JumpAnalysis: carry {last, tac}, serial carry, final (last[M], tac[M]), serial final, jfrom, jto, jtime, problems
    {
        ScanScratch<JaState> s;
        i64 *jf, *jt, *jm;
        carve([&](Carve &cv) { s.lay(cv, M, nch); jf = cv.take<i64>(F * M); jt = cv.take<i64>(F * M); jm = cv.take<i64>(F * M); });
        inside(s, M, nch); inside(jf, F * M); inside(jt, F * M); inside(jm, F * M);
        i64 problems = 0;
        for (i64 j = 0; j < M; j++) {
            for (i64 c = 0; c < nch; c++) s.sum[c * M + j] = ls_summarise(&lab[c * chunk * M + j], M, ls_chunk_len(c, F, chunk), false);
            const JaState start = halo ? JaState{hin[1][j], hin[2][j]} : JaState{lab[j], 1};
            JaState st = start;
            for (i64 c = 0; c < nch; c++) { s.carry[c * M + j] = st; ja_advance(st, s.sum[c * M + j], ls_chunk_len(c, F, chunk)); }
            s.out0[j] = st.last; s.out1[j] = st.tac;
            for (i64 c = 0; c < nch; c++) {
                st = s.carry[c * M + j];
                for (i64 f = c * chunk; f < c * chunk + ls_chunk_len(c, F, chunk); f++) {
                    const JaStep o = ja_step(st, lab[f * M + j]);
                    jf[f * M + j] = o.from; jt[f * M + j] = o.to; jm[f * M + j] = o.time; problems += o.problem;
                }
            }
            st = start;
            for (i64 f = 0; f < F; f++) {
                if (f % chunk == 0) { serial[2 * (f / chunk * M + j)] = st.last; serial[2 * (f / chunk * M + j) + 1] = st.tac; }
                ja_step(st, lab[f * M + j]);
            }
            serial[2 * nch * M + j] = st.last; serial[2 * nch * M + M + j] = st.tac;
        }
        put(s.carry, 2 * nch * M); put(serial.data(), 2 * nch * M); put(s.out0, M); put(s.out1, M); put(&serial[2 * nch * M], 2 * M);
        put(jf, F * M); put(jt, F * M); put(jm, F * M); put(&problems, 1);
        free(g_base);
    }

    // ---- assign_to_last_known_site: carry {last, tu}, serial carry, final, serial final, labels, frame_max, stats[3]
    {
        ScanScratch<AlkState> s;
        i64 *out, *fmax, *stats;
        carve([&](Carve &cv) { s.lay(cv, M, nch); out = cv.take<i64>(F * M); fmax = cv.take<i64>(F); stats = cv.take<i64>(3); });
        inside(s, M, nch); inside(out, F * M); inside(fmax, F); inside(stats, 3);
        for (i64 f = 0; f < F; f++) fmax[f] = 0;
        stats[0] = stats[1] = stats[2] = 0;
        for (i64 j = 0; j < M; j++) {
            for (i64 c = 0; c < nch; c++) s.sum[c * M + j] = ls_summarise(&lab[c * chunk * M + j], M, ls_chunk_len(c, F, chunk), false);
            const AlkState start = {halo ? hin[3][j] : -1, halo ? hin[4][j] : 0};
            AlkState st = start;
            for (i64 c = 0; c < nch; c++) { s.carry[c * M + j] = st; alk_advance(st, s.sum[c * M + j], ls_chunk_len(c, F, chunk)); }
            s.out0[j] = st.last; s.out1[j] = st.tu;
            for (i64 c = 0; c < nch; c++) {
                st = s.carry[c * M + j];
                for (i64 f = c * chunk; f < c * chunk + ls_chunk_len(c, F, chunk); f++) {
                    const AlkStep o = alk_step(st, lab[f * M + j], threshold);
                    if (o.ended) { stats[0] += o.ended; stats[1]++; if (o.ended > fmax[f]) fmax[f] = o.ended; }
                    if (o.reassign) stats[2]++;
                    out[f * M + j] = o.reassign ? st.last : lab[f * M + j];
                }
            }
            st = start;
            for (i64 f = 0; f < F; f++) {
                if (f % chunk == 0) { serial[2 * (f / chunk * M + j)] = st.last; serial[2 * (f / chunk * M + j) + 1] = st.tu; }
                alk_step(st, lab[f * M + j], threshold);
            }
            serial[2 * nch * M + j] = st.last; serial[2 * nch * M + M + j] = st.tu;
        }
        put(s.carry, 2 * nch * M); put(serial.data(), 2 * nch * M); put(s.out0, M); put(s.out1, M); put(&serial[2 * nch * M], 2 * M);
        put(out, F * M); put(fmax, F); put(stats, 3);
        free(g_base);
    }

    // ---- ReplaceUnassignedPositions: before / after / end per chunk, the same three by serial folds, ends[2 M], both replays
    {
        RupScratch s;
        i64 *out0, *out1;
        carve([&](Carve &cv) { s.lay(cv, M, nch); out0 = cv.take<i64>(F * M); out1 = cv.take<i64>(F * M); });
        inside(s.before_in, M); inside(s.after_in, M); inside(s.ends, 2 * M); inside(s.sum, nch * M);
        inside(s.cb, nch * M); inside(s.ca, nch * M); inside(s.ce, nch * M); inside(out0, F * M); inside(out1, F * M);
        for (i64 j = 0; j < M; j++) {
            for (i64 c = 0; c < nch; c++) s.sum[c * M + j] = ls_summarise(&lab[c * chunk * M + j], M, ls_chunk_len(c, F, chunk), false);
            i64 before = halo ? hin[5][j] : -1, after = halo ? hin[6][j] : -1, end = F, first = INT64_MIN, last = INT64_MIN;
            for (i64 c = 0; c < nch; c++) {
                s.cb[c * M + j] = before;
                jump_advance(before, s.sum[c * M + j]);
                if (s.sum[c * M + j].first_pos >= 0) last = s.sum[c * M + j].last;
            }
            for (i64 c = nch - 1; c >= 0; c--) {
                s.ca[c * M + j] = after; s.ce[c * M + j] = end;
                rup_back_advance(after, end, s.sum[c * M + j], c * chunk);
                if (s.sum[c * M + j].first_pos >= 0) first = s.sum[c * M + j].first;
            }
            s.ends[j] = first; s.ends[M + j] = last;
            for (i64 c = 0; c < nch; c++) {
                const i64 f0 = c * chunk, f1 = f0 + ls_chunk_len(c, F, chunk);
                i64 fill = s.cb[c * M + j];
                for (i64 f = f0; f < f1; f++) { jump_step(fill, lab[f * M + j], false); out0[f * M + j] = fill; }
                fill = s.ca[c * M + j];
                for (i64 f = f1 - 1; f >= f0; f--) { jump_step(fill, lab[f * M + j], false); out1[f * M + j] = fill; }
            }
            before = halo ? hin[5][j] : -1;
            for (i64 f = 0; f < F; f++) {
                if (f % chunk == 0) serial[f / chunk * M + j] = before;
                jump_step(before, lab[f * M + j], false);
            }
            after = halo ? hin[6][j] : -1; end = F;
            for (i64 f = F - 1; f >= 0; f--) {
                if (f == F - 1 || (f + 1) % chunk == 0) { serial[(nch + f / chunk) * M + j] = after; serial[(2 * nch + f / chunk) * M + j] = end; }
                if (lab[f * M + j] != -1) { after = lab[f * M + j]; end = f; }
            }
        }
        put(s.cb, nch * M); put(s.ca, nch * M); put(s.ce, nch * M); put(serial.data(), 3 * nch * M); put(s.ends, 2 * M);
        put(out0, F * M); put(out1, F * M);
        free(g_base);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("label_scan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(lab, chunk, halos=None):
        F, M = lab.shape
        head = np.array([F, M, chunk, halos is not None, THRESHOLD], dtype=np.int64)
        data = head.tobytes() + np.ascontiguousarray(lab).tobytes() + (b"" if halos is None else np.ascontiguousarray(halos).tobytes())
        out = np.frombuffer(subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout, dtype=np.int64)
        return parse(out, F, M, -(-F // chunk))
    return run


def parse(out, F, M, nch):
    fields = [("jump%d_%s" % (u, n), s) for u in (0, 1)
              for n, s in (("carry", (nch, M)), ("serial", (nch, M)), ("out", (M,)), ("serial_out", (M,)), ("from", (F, M)))]
    for scan in ("ja", "alk"):
        fields += [(scan + "_carry", (nch, M, 2)), (scan + "_serial", (nch, M, 2)), (scan + "_out", (2, M)), (scan + "_serial_out", (2, M))]
        fields += [("ja_from", (F, M)), ("ja_to", (F, M)), ("ja_time", (F, M)), ("ja_problems", ())] if scan == "ja" else \
                  [("alk_labels", (F, M)), ("alk_frame_max", (F,)), ("alk_stats", (3,))]
    fields += [("rup_carry", (3, nch, M)), ("rup_serial", (3, nch, M)), ("rup_ends", (2, M)), ("rup_last", (F, M)), ("rup_next", (F, M))]
    d, at = {}, 0
    for name, shape in fields:
        n = int(np.prod(shape, dtype=np.int64))
        d[name] = out[at:at + n].reshape(shape)
        at += n
    assert at == len(out)
    return d


def labels_of(F, M):
    return make_labels(F, M, seed=F * 1000 + M)


def seeded_halos(M, K, seed):
    """[7, M]: jump last, ja last, ja tac, alk last, alk tu, rup before, rup after; the site rows hold -1 too"""
    rng = np.random.default_rng(seed)
    h = rng.integers(-1, K, size=(7, M))
    h[2] = rng.integers(1, 700, size=M)
    h[4] = np.where(h[3] == -1, rng.integers(0, 700, size=M), rng.integers(0, 5, size=M))
    assert (h[[0, 1, 3, 5, 6]] == -1).any() or M < 8
    return h.astype(np.int64)


def chunk_lengths(F):
    return (1, 2, 7, 256, F + 1)


@pytest.mark.parametrize("F,M", SHAPES)
@pytest.mark.parametrize("with_halos", [False, True])
def test_chunked_equals_serial(probe, F, M, with_halos):
    """For every scan, both values of unknown_as_jump and chunk lengths 1, 2, 7, 256 and F + 1: the state the advance
    chain gives at every chunk's start (the backward chain: at every chunk's end) and at the end is the state of a serial
    fold of the step function; the results do not depend on the chunk length."""
    lab, K = labels_of(F, M)
    halos = seeded_halos(M, K, seed=F + M) if with_halos else None
    first = None
    for chunk in chunk_lengths(F):
        d = probe(lab, chunk, halos)
        for scan in ("jump0", "jump1", "ja", "alk"):
            assert np.array_equal(d[scan + "_carry"], d[scan + "_serial"]), (scan, chunk)
            assert np.array_equal(d[scan + "_out"], d[scan + "_serial_out"]), (scan, chunk)
        assert np.array_equal(d["rup_carry"], d["rup_serial"]), chunk
        results = {k: v for k, v in d.items() if "carry" not in k and "serial" not in k}
        if first is None:
            first = results
        for k, v in results.items():
            assert np.array_equal(v, first[k]), (k, chunk)
    before_in, after_in = (halos[5], halos[6]) if with_halos else (None, None)
    assert np.array_equal(first["rup_last"], R.replace(lab, 0, before_in, after_in))
    assert np.array_equal(first["rup_next"], R.replace(lab, 1, before_in, after_in))


def fold_jump_analysis(jfrom, jto, jtime, K):
    """dynamics/JumpAnalysis.py:70-86 on the per-frame arrays of pass 1 (numpy's fancy-index +=)."""
    total = np.zeros(K, dtype=np.int64)
    n_ij, tsum, tn = np.zeros((K, K)), np.zeros((K, K)), np.zeros((K, K), dtype=np.int64)
    for fr, to, tm in zip(jfrom, jto, jtime):
        known, jumped = to >= 0, tm > 0
        total[to[known]] += 1
        n_ij[fr[known], to[known]] += 1
        tsum[fr[jumped], to[jumped]] += tm[jumped]
        tn[fr[jumped], to[jumped]] += 1
    return n_ij, tsum, tn, total


@pytest.mark.parametrize("F,M", SHAPES)
@pytest.mark.parametrize("chunk", [7, 256])
def test_chunked_results_equal_the_cpu_references(probe, F, M, chunk):
    """Bit for bit: oracle.jumps, oracle.jump_analysis, oracle.assign_to_last_known_site, replace_ref.replace / ends."""
    from oracle import oracle
    lab, K = labels_of(F, M)
    d = probe(lab, chunk)
    for u in (0, 1):
        src = np.full((F, M), NONE, dtype=np.int64)
        for f, a, fr, to in oracle.jumps(lab, unknown_as_jump=bool(u)):
            assert to == lab[f, a]
            src[f, a] = fr
        assert np.array_equal(d["jump%d_from" % u], src), u
    exp = oracle.jump_analysis(lab, K)
    n_ij, tsum, tn, total = fold_jump_analysis(d["ja_from"], d["ja_to"], d["ja_time"], K)
    assert np.array_equal(n_ij, exp["n_ij"]) and np.array_equal(tsum, exp["time_sum"]) and np.array_equal(tn, exp["time_n"])
    assert np.array_equal(total, exp["total_corrected_residences"]) and int(d["ja_problems"]) == exp["n_problems"]
    t, (mx, avg, re) = oracle.assign_to_last_known_site(lab, THRESHOLD)
    assert np.array_equal(d["alk_labels"], t)
    s, n, reassigned = (int(x) for x in d["alk_stats"])
    above = np.nonzero(d["alk_frame_max"] > THRESHOLD)[0]          # the reference keeps the LAST frame's maximum above the threshold
    assert (int(d["alk_frame_max"][above[-1]]) if len(above) else 0) == mx
    assert (float(s) / n if n else 0) == avg and (reassigned if n else 0) == re
    assert np.array_equal(d["rup_last"], R.replace(lab, 0)) and np.array_equal(d["rup_next"], R.replace(lab, 1))
    first, last = R.ends(lab)
    assert np.array_equal(d["rup_ends"][0], first) and np.array_equal(d["rup_ends"][1], last)
