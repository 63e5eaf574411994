"""CPU-only: every decision of the device coordination environments (sitator_amd/csrc/coordenv_plan.h) compiled with the host
compiler into a stand-alone probe under ASan / UBSan, the way test_voronoi_plan.py builds its probe.  The probe answers the
unranking, the Horn eigenvalue, the shape measure (enumerated in the kernel's chunks), the solid angle, the cutoffs and the
confidence, and runs the whole driver serially - the kernels' order, one candidate after the other - over the fixtures
tests/test_gpu_coordenv.py runs on the device; the answers are compared with numpy, with closed forms and with the restatement
(tests/coordenv_ref.py).  Both compilers are told -ffp-contract=off."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import coordenv_ref as CR
from tests import voronoi_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode.
#   mode 0: -> int64 plan[8]; int32 shape_n[12]; float64 table[12, 8, 3]
#   mode 1: int64 n, first, count -> int32 perm[count, 8] (the first unranked, the others stepped); int32 again[count, 8] (each unranked)
#   mode 2: int64 n; float64 M[n, 9] -> float64 t[n]
#   mode 3: int64 n, shape, use_bound, chunks; float64 q[n, 3] -> float64 S
#   mode 4: int64 nv; float64 qj[3]; float64 verts[nv, 3] -> float64 solid angle; int32 {touched, overflow}
#   mode 5: int64 n; float64 rows[n, 6] = {d, d_min, w, w_max, dcut, acut} -> int32 {in, near}[n]; float64 {nd, na}[n]
#   mode 6: int64 ns; float64 max_csm; float64 csm[ns] -> int32 best; float64 {confidence, best_csm}
#   mode 7: float64 cm[9], ci[9]; int64 S, K; float64 {tau, dcut, acut, max_csm}; float64 pos[S, 3]; float64 sites[K, 3]
#           -> per site: int32 {rounds, status, flags, n, nbr, shape}; int32 sid[n]; float64 nd[n], na[n]; float64 csm_all[3];
#              float64 {confidence, csm_best}
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "coordenv_plan.h"

struct Cell { double cm[9], ci[9]; };

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

// k_coordenv_csm: the assignments in `chunks` chunks, the maximum of the chunks' maxima
static double measure(const double *q, int n, int s, int use_bound, int64_t chunks, const double *table)
{
    if (n == 1) return 0.0;
    const double *p = table + s * CE_N_MAX * 3;
    const int64_t total = ce_factorial(n), chunk = (total + chunks - 1) / chunks;
    double best = -INFINITY;
    for (int64_t t = 0; t < chunks; t++) {
        const int64_t first = t * chunk;
        const int64_t count = first < total ? (first + chunk <= total ? chunk : total - first) : 0;
        const double b = ce_best_t(q, p, n, first, count, use_bound);
        if (b > best) best = b;
    }
    return ce_measure(best, ce_norm2(q, n), ce_norm2(p, n));
}

int main()
{
    int64_t mode;
    if (fread(&mode, 8, 1, stdin) != 1) return 2;
    std::vector<double> table(CE_SHAPES * CE_N_MAX * 3);
    ce_shape_table(table.data());
    if (mode == 0) {
        const int64_t plan[8] = {VP_NBR_CAP, CE_REC_CAP, CE_FACE_CAP, CE_COORD_CAP, CE_N_MAX, CE_BLOCK, CE_LDS_BYTES, CE_SHAPES};
        int32_t sn[CE_SHAPES];
        for (int s = 0; s < CE_SHAPES; s++) sn[s] = ce_shape_n(s);
        wr(plan, 8, 8); wr(sn, 4, CE_SHAPES); wr(table.data(), 8, table.size());
        return 0;
    }
    if (mode == 1) {
        int64_t h[3];
        if (fread(h, 8, 3, stdin) != 3 || h[0] < 1 || h[0] > CE_N_MAX || h[1] < 0 || h[2] < 0 || h[1] + h[2] > ce_factorial((int)h[0])) return 2;
        const int n = (int)h[0];
        std::vector<int32_t> a((size_t)(8 * h[2]), -1), b((size_t)(8 * h[2]), -1);
        int perm[CE_N_MAX];
        ce_unrank(h[1], n, perm);
        for (int64_t k = 0; k < h[2]; k++) {
            int again[CE_N_MAX];
            ce_unrank(h[1] + k, n, again);
            for (int j = 0; j < n; j++) { a[(size_t)(8 * k + j)] = perm[j]; b[(size_t)(8 * k + j)] = again[j]; }
            const bool more = ce_next(perm, n);
            if (!more && h[1] + k + 1 != ce_factorial(n)) return 3;
        }
        wr(a.data(), 4, a.size()); wr(b.data(), 4, b.size());
        return 0;
    }
    if (mode == 2) {
        int64_t n;
        if (fread(&n, 8, 1, stdin) != 1 || n < 0) return 2;
        std::vector<double> M((size_t)(9 * n)), t((size_t)n);
        if (!rd(M.data(), 8, M.size())) return 2;
        for (int64_t k = 0; k < n; k++) t[(size_t)k] = ce_horn(&M[(size_t)(9 * k)]);
        wr(t.data(), 8, t.size());
        return 0;
    }
    if (mode == 3) {
        int64_t h[4];
        if (fread(h, 8, 4, stdin) != 4 || h[0] < 1 || h[0] > CE_N_MAX || h[1] < 0 || h[1] >= CE_SHAPES || ce_shape_n((int)h[1]) != h[0] || h[3] < 1) return 2;
        std::vector<double> q((size_t)(3 * h[0]));
        if (!rd(q.data(), 8, q.size())) return 2;
        const double S = measure(q.data(), (int)h[0], (int)h[1], (int)h[2], h[3], table.data());
        wr(&S, 8, 1);
        return 0;
    }
    if (mode == 4) {
        int64_t nv; double qj[3];
        if (fread(&nv, 8, 1, stdin) != 1 || nv < 0 || nv > 200 || fread(qj, 8, 3, stdin) != 3) return 2;
        std::vector<double> v((size_t)(3 * nv));
        if (!rd(v.data(), 8, v.size())) return 2;
        std::vector<CeVertex> rec((size_t)nv + 1);
        for (int64_t k = 0; k < nv; k++) {
            for (int a = 0; a < 3; a++) rec[(size_t)k].u[a] = v[(size_t)(3 * k + a)];
            rec[(size_t)k].nm = 3; rec[(size_t)k].pad = 0;
            for (int j = 0; j < VP_MEMBER_CAP; j++) rec[(size_t)k].m[j] = (uint8_t)(j < 3 ? 5 + j : 0);   // the face of neighbour 5
        }
        int32_t f[2] = {0, 0};
        const double w = ce_face_angle(qj, rec.data(), (int)nv, 5, &f[0], &f[1]);
        wr(&w, 8, 1); wr(f, 4, 2);
        return 0;
    }
    if (mode == 5) {
        int64_t n;
        if (fread(&n, 8, 1, stdin) != 1 || n < 0) return 2;
        std::vector<double> rows((size_t)(6 * n)), out((size_t)(2 * n));
        std::vector<int32_t> ans((size_t)(2 * n));
        if (!rd(rows.data(), 8, rows.size())) return 2;
        for (int64_t k = 0; k < n; k++) {
            const double *r = &rows[(size_t)(6 * k)];
            int near = 0;
            ans[(size_t)(2 * k)] = ce_select(r[0], r[1], r[2], r[3], r[4], r[5], &out[(size_t)(2 * k)], &out[(size_t)(2 * k + 1)], &near) ? 1 : 0;
            ans[(size_t)(2 * k + 1)] = near;
        }
        wr(ans.data(), 4, ans.size()); wr(out.data(), 8, out.size());
        return 0;
    }
    if (mode == 6) {
        int64_t ns; double max_csm, csm[CE_SHAPES_PER_N];
        if (fread(&ns, 8, 1, stdin) != 1 || ns < 0 || ns > CE_SHAPES_PER_N || fread(&max_csm, 8, 1, stdin) != 1 || !rd(csm, 8, (size_t)ns)) return 2;
        double out[2];
        const int32_t best = ce_decide(csm, (int)ns, max_csm, &out[0], &out[1]);
        wr(&best, 4, 1); wr(out, 8, 2);
        return 0;
    }
    if (mode == 7) {
        Cell c; int64_t h[2]; double f[4];
        if (fread(&c, 8, 18, stdin) != 18 || fread(h, 8, 2, stdin) != 2 || fread(f, 8, 4, stdin) != 4 || h[0] < 1 || h[1] < 1) return 2;
        const int64_t S = h[0], K = h[1];
        std::vector<double> pos((size_t)(3 * S)), sites((size_t)(3 * K));
        if (!rd(pos.data(), 8, pos.size()) || !rd(sites.data(), 8, sites.size())) return 2;
        const double vol = vp_volume(c);
        for (int64_t k = 0; k < K; k++) {
            const double *pi = &sites[(size_t)(3 * k)];
            double fi[3];
            cp_to_cell(c, pi, fi);
            CeSite out;
            out.status = VS_GROW; out.flags = 0; out.n = 0; out.nbr = 0;
            int rounds = 0;
            std::vector<double> q;
            std::vector<int32_t> sid;
            while (out.status == VS_GROW) {
                BarrierPlan pl;
                const double R = vp_radius(vol, S, rounds);
                if (rounds >= VP_MAX_ROUNDS || !bp_plan(c, R, pl)) { out.status = VS_CAPACITY; break; }
                rounds++;
                std::vector<VpKey> keys;
                for (int64_t s = 0; s < S; s++) {
                    const double *ps = &pos[(size_t)(3 * s)];
                    double fs[3];
                    cp_to_cell(c, ps, fs);
                    int lo[3], hi[3];
                    for (int a = 0; a < 3; a++) bp_axis_range(fi[a] - fs[a], pl.q[a], pl.n[a], &lo[a], &hi[a]);
                    for (int m0 = lo[0]; m0 <= hi[0]; m0++)
                        for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                            for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                                double x[3];
                                VpKey key;
                                key.d2 = vp_relative(c, pi, ps, m0, m1, m2, x);
                                key.s = (int32_t)s; key.m[0] = m0; key.m[1] = m1; key.m[2] = m2;
                                if (key.d2 <= R * R) keys.push_back(key);
                            }
                }
                std::sort(keys.begin(), keys.end(), vp_key_less);
                const int count = (int)keys.size();
                out.nbr = count;
                if (count > VP_NBR_CAP) { out.status = VS_CAPACITY; break; }
                q.assign((size_t)(3 * count) + 3, 0.0);
                sid.assign((size_t)count + 1, 0);
                for (int j = 0; j < count; j++) {
                    vp_relative(c, pi, &pos[(size_t)(3 * keys[(size_t)j].s)], keys[(size_t)j].m[0], keys[(size_t)j].m[1], keys[(size_t)j].m[2], &q[(size_t)(3 * j)]);
                    sid[(size_t)j] = keys[(size_t)j].s;
                }
                std::vector<CeVertex> rec(CE_REC_CAP);
                ce_site_serial(q.data(), count, R, f[0], f[1], f[2], rec.data(), out);
            }
            double csm[CE_SHAPES_PER_N] = {NAN, NAN, NAN}, tail[2] = {0.0, NAN};
            int32_t shape = -1;
            const int n = out.status == VS_OK ? out.n : 0;
            std::vector<int32_t> ids((size_t)n + 1);
            if (out.status == VS_OK) {
                double cq[CE_N_MAX * 3];
                for (int j = 0; j < n; j++) {
                    ids[(size_t)j] = sid[(size_t)out.pos[j]];
                    if (j < CE_N_MAX) for (int a = 0; a < 3; a++) cq[3 * j + a] = q[(size_t)(3 * out.pos[j] + a)];
                }
                int shapes[CE_SHAPES_PER_N];
                const int ns = n <= CE_N_MAX ? ce_shapes_of(n, shapes) : 0;
                for (int j = 0; j < ns; j++) csm[j] = measure(cq, n, shapes[j], 1, CE_BLOCK, table.data());
                const int best = ce_decide(csm, ns, f[3], &tail[0], &tail[1]);
                shape = best >= 0 ? shapes[best] : -1;
            }
            const int32_t head[6] = {rounds, out.status, out.status == VS_OK ? out.flags : 0, n, out.nbr, shape};
            wr(head, 4, 6); wr(ids.data(), 4, (size_t)n); wr(out.nd, 8, (size_t)n); wr(out.na, 8, (size_t)n); wr(csm, 8, 3); wr(tail, 8, 2);
        }
        return 0;
    }
    return 2;
}
"""


class Probe(object):
    def __init__(self, exe):
        self.exe = exe

    def _run(self, mode, *parts):
        data = np.array([mode], dtype=np.int64).tobytes() + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
        return subprocess.run([self.exe], input=data, stdout=subprocess.PIPE, check=True).stdout

    def plan(self):
        raw = self._run(0)
        return ([int(v) for v in np.frombuffer(raw[:64], dtype=np.int64)], np.frombuffer(raw[64:112], dtype=np.int32),
                np.frombuffer(raw[112:], dtype=np.float64).reshape(12, 8, 3))

    def perms(self, n, first, count):
        raw = self._run(1, np.array([n, first, count], dtype=np.int64))
        both = np.frombuffer(raw, dtype=np.int32).reshape(2, count, 8)
        return both[0, :, :n], both[1, :, :n]

    def horn(self, M):
        M = np.asarray(M, dtype=np.float64).reshape(-1, 9)
        return np.frombuffer(self._run(2, np.array([len(M)], dtype=np.int64), M), dtype=np.float64)

    def csm(self, q, symbol, use_bound=1, chunks=256):
        q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
        raw = self._run(3, np.array([len(q), CR.SYMBOLS.index(symbol), use_bound, chunks], dtype=np.int64), q)
        return float(np.frombuffer(raw, dtype=np.float64)[0])

    def face(self, qj, verts):
        verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
        raw = self._run(4, np.array([len(verts)], dtype=np.int64), np.asarray(qj, dtype=np.float64), verts)
        return float(np.frombuffer(raw[:8], dtype=np.float64)[0]), [int(v) for v in np.frombuffer(raw[8:], dtype=np.int32)]

    def select(self, rows):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        raw = self._run(5, np.array([len(rows)], dtype=np.int64), rows)
        n = len(rows)
        return np.frombuffer(raw[:8 * n], dtype=np.int32).reshape(n, 2), np.frombuffer(raw[8 * n:], dtype=np.float64).reshape(n, 2)

    def decide(self, csm, max_csm):
        raw = self._run(6, np.array([len(csm)], dtype=np.int64), np.array([max_csm]), np.asarray(csm, dtype=np.float64))
        return int(np.frombuffer(raw[:4], dtype=np.int32)[0]), [float(v) for v in np.frombuffer(raw[4:], dtype=np.float64)]

    def sites(self, cell, pos, sites, tau=CR.TAU, dcut=CR.DISTANCE_CUTOFF, acut=CR.ANGLE_CUTOFF, max_csm=CR.MAX_CSM):
        cell = np.asarray(cell, dtype=np.float64)
        raw = self._run(7, np.ascontiguousarray(cell.T), VR.cell_inverse(cell), np.array([len(pos), len(sites)], dtype=np.int64),
                        np.array([tau, dcut, acut, max_csm]), np.asarray(pos, dtype=np.float64), np.asarray(sites, dtype=np.float64))
        out, at = [], 0
        for _ in range(len(sites)):
            rounds, status, flags, n, nbr, shape = (int(v) for v in np.frombuffer(raw[at:at + 24], dtype=np.int32))
            at += 24
            sid = np.frombuffer(raw[at:at + 4 * n], dtype=np.int32); at += 4 * n
            nd = np.frombuffer(raw[at:at + 8 * n], dtype=np.float64); at += 8 * n
            na = np.frombuffer(raw[at:at + 8 * n], dtype=np.float64); at += 8 * n
            csm = np.frombuffer(raw[at:at + 24], dtype=np.float64); at += 24
            conf, best = (float(v) for v in np.frombuffer(raw[at:at + 16], dtype=np.float64)); at += 16
            out.append({"rounds": rounds, "status": status, "flags": flags, "n": n, "nbr_count": nbr, "shape": shape, "vertices": sid.tolist(),
                        "norm_distance": nd, "norm_angle": na, "csm_all": csm, "confidence": conf, "csm_best": best})
        assert at == len(raw)
        return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("coordenv_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])
    return Probe(exe)


def test_plan_and_shape_table(probe):
    plan, shape_n, table = probe.plan()
    assert plan[0] == VR.NBR_CAP and plan[4] == 8 and plan[5] == 256 and plan[6] <= 64 * 1024 and plan[7] == len(CR.SYMBOLS)
    for s, sym in enumerate(CR.SYMBOLS):
        ref = CR.shapes()[sym]
        assert shape_n[s] == len(ref) == int(sym.split(":")[1])
        got = table[s, :len(ref)]
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=4e-16)
        assert np.all(table[s, len(ref):] == 0.0)
        # the same shape as the restatement's own table, whatever the order and the orientation of the vertices
        assert CR.csm(got, ref) <= 1e-12


@pytest.mark.parametrize("n", range(1, 9))
def test_unranking_is_itertools(probe, n):
    ref = np.array(list(itertools.permutations(range(n))), dtype=np.int32)
    total = math.factorial(n)
    chunk = -(-total // 256)
    if total <= 5040:
        spans = [(0, total)]
    else:                                                             # first and last ranks, and the chunk boundaries of the kernel
        spans = [(0, 2 * chunk + 1), (total - chunk - 1, chunk + 1)] + [(k * chunk - 1, 3) for k in (1, 2, 100, 255)]
    for first, count in spans:
        stepped, unranked = probe.perms(n, first, count)
        assert np.array_equal(stepped, ref[first:first + count]) and np.array_equal(unranked, ref[first:first + count])


def horn_reference(M):
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    sv = np.linalg.svd(M, compute_uv=False)
    return sv[0] + sv[1] + (sv[2] if np.linalg.det(M) >= 0 else -sv[2])


def test_horn_eigenvalue_is_the_signed_sum_of_singular_values(probe):
    rng = np.random.default_rng(5)
    Ms = [rng.normal(size=(3, 3)) for _ in range(200)]
    Ms += [np.outer(rng.normal(size=3), rng.normal(size=3)) for _ in range(50)]                     # rank 1
    Ms += [rng.normal(size=(3, 2)) @ rng.normal(size=(2, 3)) for _ in range(50)]                    # rank 2
    sh = CR.shapes()
    for sym in ("L:2", "TL:3", "S:4"):                                                              # planar and linear shapes
        p = sh[sym]
        for _ in range(20):
            q = p[rng.permutation(len(p))] + rng.normal(0, 0.05, p.shape)
            Ms.append(q.T @ p)
    Ms += [np.zeros((3, 3)), np.eye(3), -np.eye(3), np.diag([1.0, 1.0, -1.0]), np.diag([3.0, 2.0, 0.0])]
    got = probe.horn(np.array(Ms))
    ref = np.array([horn_reference(M) for M in Ms])
    scale = np.array([max(1.0, np.linalg.norm(M)) for M in Ms])
    err = np.abs(got - ref) / scale
    print("largest |t - svd| / |M| = %.3g" % err.max())
    assert err.max() <= 32 * 2.0 ** -53                               # a 4 x 4 Jacobi is backward stable to a few eps |N|


def test_closed_form_shape_measures(probe):
    sh = CR.shapes()
    _, _, table = probe.plan()
    assert abs(probe.csm(sh["S:4"], "T:4") - 100.0 / 3.0) <= 1e-11
    assert abs(probe.csm(sh["O:6"], "T:6") - 16.7367553608) <= 1e-9
    assert abs(probe.csm(sh["T:5"], "S:5") - 10.4307806183) <= 1e-9
    assert abs(probe.csm(sh["S:4"] * 1.5, "S:4")) <= 1e-12 and abs(probe.csm(sh["S:4"], "S:4", use_bound=0, chunks=1)) <= 1e-12
    rng = np.random.default_rng(9)
    for s, sym in enumerate(CR.SYMBOLS):
        p = sh[sym]
        rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        rot *= np.sign(np.linalg.det(rot))
        q = 2.5 * p[rng.permutation(len(p))] @ rot.T                  # scaled, rotated, relabelled: still the shape
        assert probe.csm(q, sym) <= 1e-12, sym
        assert probe.csm(table[s, :len(p)], sym) == 0.0 or probe.csm(table[s, :len(p)], sym) <= 1e-13
        # the bound never changes the answer, nor does the chunking
        noisy = q + rng.normal(0, 0.1, q.shape)
        a = probe.csm(noisy, sym, use_bound=1, chunks=256)
        assert a == probe.csm(noisy, sym, use_bound=0, chunks=256) == probe.csm(noisy, sym, use_bound=1, chunks=7)
        assert abs(a - CR.csm(noisy, p)) <= 1e-11
    mirror = sh["T:5"] + np.array([[0.1, 0.2, 0.0], [0, 0, 0], [0, 0, 0.1], [0, 0.1, 0], [0, 0, 0]])
    assert abs(probe.csm(mirror * [1, 1, -1.0], "T:5") - CR.csm(mirror * [1, 1, -1.0], sh["T:5"])) <= 1e-11   # proper rotations only


def test_solid_angles(probe):
    square = [[1, 1, 1.0], [-1, 1, 1], [-1, -1, 1], [1, -1, 1]]
    w, (touched, over) = probe.face([0, 0, 2.0], square)
    assert abs(w - 4 * np.pi / 6) <= 1e-15 and touched == 1 and over == 0
    w, _ = probe.face([0, 0, 2.0], [square[k] for k in (2, 0, 3, 1)])           # any order of arrival
    assert abs(w - 4 * np.pi / 6) <= 1e-15
    tilted = np.array(square) @ np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0].T
    normal = 2.0 * tilted.mean(axis=0)
    assert abs(probe.face(normal, tilted)[0] - 4 * np.pi / 6) <= 1e-14
    assert probe.face([0, 0, 2.0], square[:1]) == (0.0, [1, 0])                  # a vertex-only face
    assert probe.face([0, 0, 2.0], square[:2]) == (0.0, [1, 0])
    assert probe.face([0, 0, 2.0], [[-1, 0, 1.0], [0, 0, 1], [2, 0, 1]])[0] == 0.0    # collinear
    assert probe.face([0, 0, 2.0], [])[1] == [0, 0]
    ring = [[np.cos(a), np.sin(a), 1.0] for a in np.linspace(0, 2 * np.pi, 40, endpoint=False)]
    assert probe.face([0, 0, 2.0], ring)[1] == [1, 1]                            # more vertices than the cap: reported
    w, f = probe.face([0, 0, 2.0], ring[:32])
    assert f == [1, 0] and abs(w - CR.polygon_angle(ring[:32], np.array([0, 0, 2.0]))) <= 1e-14


def test_cutoffs_at_inside_and_outside(probe):
    d, a = CR.DISTANCE_CUTOFF, CR.ANGLE_CUTOFF
    rows = [[d, 1.0, 1.0, 1.0, d, a], [d * (1 - 1e-6), 1.0, 1.0, 1.0, d, a], [d * (1 + 1e-6), 1.0, 1.0, 1.0, d, a],
            [d * (1 + 5e-10), 1.0, 1.0, 1.0, d, a], [d * (1 - 5e-10), 1.0, 1.0, 1.0, d, a],
            [1.0, 1.0, a, 1.0, d, a], [1.0, 1.0, a * (1 + 1e-6), 1.0, d, a], [1.0, 1.0, a * (1 - 1e-6), 1.0, d, a],
            [1.0, 1.0, a * (1 - 5e-10), 1.0, d, a], [1.0, 1.0, a * (1 + 5e-10), 1.0, d, a],
            [2.0, 2.0, 0.0, 0.0, d, a], [3.0, 2.0, 0.5, 1.0, d, a]]
    ans, ratios = probe.select(rows)
    assert ans.tolist() == [[1, 1], [1, 0], [0, 0], [0, 1], [1, 1], [1, 1], [1, 0], [0, 0], [0, 1], [1, 1], [0, 0], [0, 0]]
    assert ratios[-1].tolist() == [1.5, 0.5] and ratios[-2].tolist() == [1.0, 0.0]


def test_confidence(probe):
    best, (conf, s) = probe.decide([2.0, 6.0], 8.0)
    assert best == 0 and s == 2.0 and abs(conf - 0.5625 / (0.5625 + 0.0625)) <= 1e-15
    assert probe.decide([2.2876383367, 20.0], 8.0)[0] == 0 and probe.decide([2.2876383367, 20.0], 8.0)[1][0] == 1.0
    best, (conf, s) = probe.decide([9.0, 8.0], 8.0)                   # nothing under max_csm: no shape, confidence 0
    assert best == -1 and conf == 0.0 and s == 8.0
    best, (conf, s) = probe.decide([], 8.0)
    assert best == -1 and conf == 0.0 and np.isnan(s)
    assert probe.decide([3.0, 3.0], 8.0)[0] == 0                      # library order breaks the tie
    assert probe.decide([3.0, 3.0], 8.0)[1][0] == 0.5


@pytest.mark.parametrize("name", sorted(CR.FIXTURES))
def test_serial_driver_is_the_restatement(probe, name):
    cell, pos, sites = CR.fixture(name)
    ref = CR.answer(name)
    got = probe.sites(cell, pos, sites)
    worst = 0.0
    for g, r in zip(got, ref):
        assert g["status"] == CR.OK and g["flags"] == 0
        assert g["rounds"] == r["rounds"] and g["nbr_count"] == r["nbr_count"]
        assert g["n"] == r["n"] and g["vertices"] == r["vertices"]
        symbol = CR.SYMBOLS[g["shape"]] if g["shape"] >= 0 else "UN:%d" % g["n"]
        assert symbol == r["symbol"]
        assert np.array_equal(np.isnan(g["csm_all"]), np.isnan(r["csm_all"]))
        for key in ("norm_distance", "norm_angle", "csm_all", "confidence"):
            a, b = np.atleast_1d(g[key]), np.atleast_1d(r[key])
            if np.any(~np.isnan(b)):
                worst = max(worst, float(np.nanmax(np.abs(a - b))))
    print("%s: largest deviation from the restatement %.3g" % (name, worst))
    assert worst <= 1e-9 / 64
