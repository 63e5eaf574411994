"""CPU-only: every decision of the device Voronoi nodes (sitator_amd/csrc/voronoi_plan.h) compiled with the host compiler into a
stand-alone probe under ASan / UBSan, the way test_hull_predicates.py builds its probe.  The probe answers sphere and
membership questions, and drives the neighbour search, the enumeration, the completeness test and the merge serially - the
kernels' order, one candidate after the other - over the fixtures tests/test_gpu_voronoi.py runs on the device; the answers are
compared with the restatement (tests/voronoi_ref.py) and with the exact rational evaluation.  Both compilers are told
-ffp-contract=off, so what is certified here is what the kernel certifies.

Designed inputs: a coplanar quadruple (skipped), a quadruple at the shape floor on both sides, a neighbour exactly on, just inside
and just outside each threshold (certified or uncertain, never wrong), an atom whose neighbours leave an octant empty (VS_GROW),
two record centres 2 mu apart (ambiguous)."""
import os
import subprocess

import numpy as np
import pytest

from tests import voronoi_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode.
#   mode 0: -> int64 plan[8]; float64 {VP_R0_FACTOR, VP_GROWTH, VP_MU_FACTOR, VP_SHAPE_MIN}
#   mode 1: int64 n; float64 quad[n, 3, 3] -> int32 valid[n]; float64 out[n, 6] = {u0, u1, u2, r, ec, rho}
#   mode 2: int64 n; float64 tau; float64 rows[n, 12] = {qa, qb, qc, q} -> int32 answer[n] (-1: skipped); float64 out[n, 3] = {d, r, slack}
#   mode 3: float64 cm[9], ci[9]; int64 S, nA; float64 R, tau; float64 pos[S, 3]; int32 active[nA]
#           -> per active atom: int32 {count, status, n_far, n_rec}; int32 sid[min(count, cap)]; float64 q[min(count, cap), 3];
#              VpRecord rec[n_rec]
#   mode 4: float64 cm[9], ci[9]; int64 n; float64 mu; float64 c[n, 3] -> int32 status; float64 w[n, 3]; int64 node[n]; int64 n_first;
#              int64 first[n_first]
#   mode 5: int64 n; int32 self; float64 R, tau; float64 q[n, 3]; int32 sid[n] -> int32 {status, n_far, n_rec}; VpRecord rec[n_rec]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "voronoi_plan.h"

struct Cell { double cm[9], ci[9]; };

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

// k_voronoi_spheres, one candidate after the other
static int run_atom(const double *q, const int32_t *sid, int n, int32_t self, const double p[3], double R, double tau,
                    std::vector<VpRecord> &rec, int *n_far)
{
    int octants = 0, uncertain = 0, capacity = 0;
    *n_far = 0;
    for (int k = 0; k < n; k++) {
        const int o = vp_octant(q + 3 * k);
        if (o >= 0) octants |= 1 << o;
    }
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) {
            int found = 0;
            for (int c = b + 1; c < n; c++) {
                VpRecord r;
                const int kind = vp_candidate(q, sid, n, self, p, a, b, c, R, tau, &r);
                if (kind == VC_FAR) (*n_far)++;
                else if (kind == VC_UNCERTAIN) uncertain = 1;
                else if (kind == VC_CAPACITY) capacity = 1;
                else if (kind == VC_RECORD) {
                    if (found < VP_PAIR_FOUND && (int)rec.size() < VP_REC_CAP) { rec.push_back(r); found++; }
                    else capacity = 1;
                }
            }
        }
    return vp_status(0, capacity, octants, *n_far, uncertain);
}

int main()
{
    int64_t mode;
    if (fread(&mode, 8, 1, stdin) != 1) return 2;
    if (mode == 0) {
        const int64_t plan[8] = {VP_NBR_CAP, VP_REC_CAP, VP_MEMBER_CAP, VP_BLOCK, VP_LDS_BYTES, VP_MAX_ROUNDS, (int64_t)sizeof(VpRecord),
                                 (int64_t)(1.0 / VP_SHAPE_MIN)};
        const double f[4] = {VP_R0_FACTOR, VP_GROWTH, VP_MU_FACTOR, VP_SHAPE_MIN};
        wr(plan, 8, 8); wr(f, 8, 4);
        return 0;
    }
    if (mode == 1) {
        int64_t n;
        if (fread(&n, 8, 1, stdin) != 1 || n < 0) return 2;
        std::vector<double> quad((size_t)(9 * n)), out((size_t)(6 * n), 0.0);
        std::vector<int32_t> valid((size_t)n);
        if (!rd(quad.data(), 8, (size_t)(9 * n))) return 2;
        for (int64_t k = 0; k < n; k++) {
            const double *p = &quad[(size_t)(9 * k)];
            VpSphere s;
            valid[(size_t)k] = vp_sphere(p, p + 3, p + 6, s) ? 1 : 0;
            if (valid[(size_t)k]) {
                double *o = &out[(size_t)(6 * k)];
                o[0] = s.u[0]; o[1] = s.u[1]; o[2] = s.u[2]; o[3] = s.r; o[4] = s.ec; o[5] = s.rho;
            }
        }
        wr(valid.data(), 4, (size_t)n); wr(out.data(), 8, (size_t)(6 * n));
        return 0;
    }
    if (mode == 2) {
        int64_t n; double tau;
        if (fread(&n, 8, 1, stdin) != 1 || n < 0 || fread(&tau, 8, 1, stdin) != 1) return 2;
        std::vector<double> rows((size_t)(12 * n)), out((size_t)(3 * n), 0.0);
        std::vector<int32_t> answer((size_t)n);
        if (!rd(rows.data(), 8, (size_t)(12 * n))) return 2;
        for (int64_t k = 0; k < n; k++) {
            const double *p = &rows[(size_t)(12 * k)];
            VpSphere s;
            answer[(size_t)k] = -1;
            if (!vp_sphere(p, p + 3, p + 6, s)) continue;
            const double d = vp_distance(p + 9, s), slack = vp_slack(d, s, tau);
            answer[(size_t)k] = vp_classify(d, s.r, tau, slack);
            out[(size_t)(3 * k)] = d; out[(size_t)(3 * k + 1)] = s.r; out[(size_t)(3 * k + 2)] = slack;
        }
        wr(answer.data(), 4, (size_t)n); wr(out.data(), 8, (size_t)(3 * n));
        return 0;
    }
    if (mode == 3) {
        Cell c; int64_t h[2]; double f[2];
        if (fread(&c, 8, 18, stdin) != 18 || fread(h, 8, 2, stdin) != 2 || fread(f, 8, 2, stdin) != 2 || h[0] < 1 || h[1] < 0) return 2;
        const int64_t S = h[0], nA = h[1];
        const double R = f[0], tau = f[1];
        std::vector<double> pos((size_t)(3 * S));
        std::vector<int32_t> active((size_t)nA);
        if (!rd(pos.data(), 8, (size_t)(3 * S)) || !rd(active.data(), 4, (size_t)nA)) return 2;
        BarrierPlan pl;
        if (!bp_plan(c, R, pl)) return 3;
        for (int64_t k = 0; k < nA; k++) {
            const int32_t i = active[(size_t)k];
            if (i < 0 || i >= S) return 3;
            const double *pi = &pos[(size_t)(3 * i)];
            double fi[3];
            cp_to_cell(c, pi, fi);
            std::vector<VpKey> keys;                                  // k_voronoi_neighbours
            for (int64_t s = 0; s < S; s++) {
                const double *ps = &pos[(size_t)(3 * s)];
                double fs[3];
                cp_to_cell(c, ps, fs);
                int lo[3], hi[3];
                for (int a = 0; a < 3; a++) bp_axis_range(fi[a] - fs[a], pl.q[a], pl.n[a], &lo[a], &hi[a]);
                for (int m0 = lo[0]; m0 <= hi[0]; m0++)
                    for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                        for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                            if (s == i && m0 == 0 && m1 == 0 && m2 == 0) continue;
                            double q[3];
                            VpKey key;
                            key.d2 = vp_relative(c, pi, ps, m0, m1, m2, q);
                            key.s = (int32_t)s; key.m[0] = m0; key.m[1] = m1; key.m[2] = m2;
                            if (key.d2 <= R * R) keys.push_back(key);
                        }
            }
            std::sort(keys.begin(), keys.end(), vp_key_less);
            const int count = (int)keys.size(), n = count < VP_NBR_CAP ? count : VP_NBR_CAP;
            std::vector<double> q((size_t)(3 * n) + 3);
            std::vector<int32_t> sid((size_t)n + 1);
            for (int j = 0; j < n; j++) {
                vp_relative(c, pi, &pos[(size_t)(3 * keys[(size_t)j].s)], keys[(size_t)j].m[0], keys[(size_t)j].m[1], keys[(size_t)j].m[2], &q[(size_t)(3 * j)]);
                sid[(size_t)j] = keys[(size_t)j].s;
            }
            std::vector<VpRecord> rec;
            int n_far = 0, status = VS_CAPACITY;
            if (count <= VP_NBR_CAP) status = run_atom(q.data(), sid.data(), n, i, pi, R, tau, rec, &n_far);
            if (status != VS_OK) rec.clear();
            const int32_t head[4] = {count, status, n_far, (int32_t)rec.size()};
            wr(head, 4, 4); wr(sid.data(), 4, (size_t)n); wr(q.data(), 8, (size_t)(3 * n)); wr(rec.data(), sizeof(VpRecord), rec.size());
        }
        return 0;
    }
    if (mode == 4) {
        Cell c; int64_t n; double mu;
        if (fread(&c, 8, 18, stdin) != 18 || fread(&n, 8, 1, stdin) != 1 || n < 0 || fread(&mu, 8, 1, stdin) != 1) return 2;
        std::vector<double> cen((size_t)(3 * n)), w((size_t)(3 * n));
        if (!rd(cen.data(), 8, (size_t)(3 * n))) return 2;
        for (int64_t k = 0; k < n; k++) { double fl[3]; cp_wrap(c, &cen[(size_t)(3 * k)], &w[(size_t)(3 * k)], fl); }
        std::vector<int64_t> node, first;
        const int32_t status = vp_merge(c, w.data(), n, mu, node, first);
        const int64_t nf = (int64_t)first.size();
        wr(&status, 4, 1); wr(w.data(), 8, (size_t)(3 * n)); wr(node.data(), 8, (size_t)n); wr(&nf, 8, 1); wr(first.data(), 8, first.size());
        return 0;
    }
    if (mode == 5) {
        int64_t n; int32_t self; double f[2];
        if (fread(&n, 8, 1, stdin) != 1 || n < 0 || n > VP_NBR_CAP || fread(&self, 4, 1, stdin) != 1 || fread(f, 8, 2, stdin) != 2) return 2;
        std::vector<double> q((size_t)(3 * n) + 3);
        std::vector<int32_t> sid((size_t)n + 1);
        if (!rd(q.data(), 8, (size_t)(3 * n)) || !rd(sid.data(), 4, (size_t)n)) return 2;
        const double p[3] = {0.0, 0.0, 0.0};
        std::vector<VpRecord> rec;
        int n_far = 0;
        const int status = run_atom(q.data(), sid.data(), (int)n, self, p, f[0], f[1], rec, &n_far);
        const int32_t head[3] = {status, n_far, (int32_t)rec.size()};
        wr(head, 4, 3); wr(rec.data(), sizeof(VpRecord), rec.size());
        return 0;
    }
    return 2;
}
"""

RECORD = np.dtype([("c", np.float64, 3), ("r", np.float64), ("n", np.int32), ("atom", np.int32), ("m", np.int32, VR.MEMBER_CAP)])


def cell_block(cell):
    cell = np.asarray(cell, dtype=np.float64)
    return np.ascontiguousarray(cell.T).tobytes() + VR.cell_inverse(cell).tobytes()


class Probe(object):
    def __init__(self, exe):
        self.exe = exe

    def _run(self, data):
        return subprocess.run([self.exe], input=data, stdout=subprocess.PIPE, check=True).stdout

    def plan(self):
        raw = self._run(np.array([0], dtype=np.int64).tobytes())
        return [int(v) for v in np.frombuffer(raw[:64], dtype=np.int64)], [float(v) for v in np.frombuffer(raw[64:], dtype=np.float64)]

    def spheres(self, quads):
        quads = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 3, 3)
        n = len(quads)
        raw = self._run(np.array([1, n], dtype=np.int64).tobytes() + quads.tobytes())
        return np.frombuffer(raw[:4 * n], dtype=np.int32), np.frombuffer(raw[4 * n:], dtype=np.float64).reshape(n, 6)

    def classify(self, rows, tau):
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 12)
        n = len(rows)
        raw = self._run(np.array([2, n], dtype=np.int64).tobytes() + np.array([tau]).tobytes() + rows.tobytes())
        return np.frombuffer(raw[:4 * n], dtype=np.int32), np.frombuffer(raw[4 * n:], dtype=np.float64).reshape(n, 3)

    def atoms(self, cell, pos, active, R, tau):
        """Per active atom a dict of ``count``, ``status``, ``n_far``, ``sid``, ``q``, ``rec`` (a RECORD array)."""
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        active = np.ascontiguousarray(active, dtype=np.int32)
        raw = self._run(np.array([3], dtype=np.int64).tobytes() + cell_block(cell) + np.array([len(pos), len(active)], dtype=np.int64).tobytes()
                        + np.array([R, tau]).tobytes() + pos.tobytes() + active.tobytes())
        out, at = [], 0
        for _ in active:
            count, status, n_far, n_rec = (int(v) for v in np.frombuffer(raw[at:at + 16], dtype=np.int32))
            at += 16
            n = min(count, VR.NBR_CAP)
            sid = np.frombuffer(raw[at:at + 4 * n], dtype=np.int32); at += 4 * n
            q = np.frombuffer(raw[at:at + 24 * n], dtype=np.float64).reshape(n, 3); at += 24 * n
            rec = np.frombuffer(raw[at:at + RECORD.itemsize * n_rec], dtype=RECORD); at += RECORD.itemsize * n_rec
            out.append({"count": count, "status": status, "n_far": n_far, "sid": sid, "q": q, "rec": rec})
        assert at == len(raw)
        return out

    def merge(self, cell, centers, mu):
        centers = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3)
        n = len(centers)
        raw = self._run(np.array([4], dtype=np.int64).tobytes() + cell_block(cell) + np.array([n], dtype=np.int64).tobytes()
                        + np.array([mu]).tobytes() + centers.tobytes())
        status = int(np.frombuffer(raw[:4], dtype=np.int32)[0])
        w = np.frombuffer(raw[4:4 + 24 * n], dtype=np.float64).reshape(n, 3)
        node = np.frombuffer(raw[4 + 24 * n:4 + 32 * n], dtype=np.int64)
        first = np.frombuffer(raw[12 + 32 * n:], dtype=np.int64)
        return status, w, node, first

    def atom_list(self, q, sid, self_sid, R, tau):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
        sid = np.ascontiguousarray(sid, dtype=np.int32)
        raw = self._run(np.array([5, len(q)], dtype=np.int64).tobytes() + np.array([self_sid], dtype=np.int32).tobytes()
                        + np.array([R, tau]).tobytes() + q.tobytes() + sid.tobytes())
        status, n_far, n_rec = (int(v) for v in np.frombuffer(raw[:12], dtype=np.int32))
        return status, n_far, np.frombuffer(raw[12:], dtype=RECORD)

    def nodes(self, cell, pos, tau):
        """The driver of voronoi.hip over the probe: rounds of the search radius, then the merge."""
        S = len(pos)
        status, nbr = np.full(S, VR.GROW, dtype=np.int32), np.zeros(S, dtype=np.int32)
        recs, active, rounds, R = [None] * S, list(range(S)), 0, 0.0
        while active and rounds < VR.MAX_ROUNDS:
            R = VR.radius(cell, S, rounds)
            rounds += 1
            nxt = []
            for i, a in zip(active, self.atoms(cell, pos, active, R, tau)):
                status[i], nbr[i], recs[i] = a["status"], a["count"], a["rec"]
                if a["status"] == VR.GROW:
                    nxt.append(i)
            active = nxt
        out = {"status": status, "nbr_count": nbr, "rounds": rounds, "final_radius": R, "vertices": [], "centers": np.zeros((0, 3)),
               "radii": np.zeros(0)}
        if np.all(status == VR.OK):
            flat = np.concatenate(recs)
            merged, w, node, first = self.merge(cell, flat["c"], VR.MU_FACTOR * tau)
            out["merge_status"], out["records"] = merged, len(flat)
            if merged == VR.OK:
                verts = [set() for _ in first]
                for k, r in enumerate(flat):
                    verts[node[k]].update(int(v) for v in r["m"][:r["n"]])
                out.update(vertices=[sorted(v) for v in verts], centers=w[first], radii=flat["r"][first])
        return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("voronoi_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])
    return Probe(exe)


def test_plan_constants(probe):
    plan, f = probe.plan()
    assert plan[:3] == [VR.NBR_CAP, VR.REC_CAP, VR.MEMBER_CAP] and plan[3] == 256 and plan[4] <= 64 * 1024
    assert plan[5] == VR.MAX_ROUNDS and plan[6] == RECORD.itemsize and plan[7] == int(1.0 / VR.SHAPE_MIN)
    assert f == [VR.R0_FACTOR, VR.GROWTH, VR.MU_FACTOR, VR.SHAPE_MIN]


# ---- the sphere ---------------------------------------------------------------------------------------------------------------

def fixture_quads(name):
    """The relative quadruples (q_a, q_b, q_c) of every record of a fixture."""
    return np.array([quad for _, quad, _, _ in VR.answer(name)["all_quads"]]).reshape(-1, 3, 3)


def test_the_sphere_is_within_its_bound_of_the_exact_one(probe):
    worst_c, worst_bound = 0.0, 0.0
    for name in ("bcc2_jitter", "fcc2_jitter", "sc3_jitter", "small_triclinic", "triclinic"):
        quads = fixture_quads(name)
        valid, out = probe.spheres(quads)
        assert valid.all(), name
        r_valid, r_u, r_r, _ = VR.spheres(quads[:, 0], quads[:, 1], quads[:, 2])
        assert r_valid.all() and np.array_equal(out[:, :3], r_u) and np.array_equal(out[:, 3], r_r), name   # the restatement's arithmetic is the header's
        for k, quad in enumerate(quads):
            u = VR.exact_center(*quad)
            err = float(VR._sqrt(sum((VR.Fraction(float(out[k, j])) - u[j]) ** 2 for j in range(3))))
            assert err <= out[k, 4], (name, k, err, out[k, 4])        # the forward bound holds
            assert abs(float(VR.exact_radius(u)) - out[k, 3]) <= out[k, 4] + 4 * VR.EPS * out[k, 3], (name, k)
            worst_c, worst_bound = max(worst_c, err), max(worst_bound, out[k, 4])
    print("largest error of a relative centre %.3g, largest bound %.3g" % (worst_c, worst_bound))
    assert worst_bound < VR.TAU / 16.0                                # what VP_SHAPE_MIN is derived for


def test_a_coplanar_quadruple_is_skipped_and_the_shape_floor_cuts_where_it_says(probe):
    a, b = np.array([1.5, 0.25, 1.0]), np.array([-0.5, 2.0, 1.25])
    normal = np.cross(a, b) / np.linalg.norm(np.cross(a, b))
    flat = 0.5 * a + 0.75 * b                                        # dyadic weights of dyadic points: exactly coplanar with 0, a, b
    quads = [[a, b, flat], [a, b, a]]                                 # coplanar; a repeated point
    base = VR.exact_ratio(a, b, flat + 1e-3 * normal) / 1e-3         # |det| / permanent per unit of height, to first order
    sides = []
    for factor in (0.9, 1.1):
        c = flat + factor * VR.SHAPE_MIN / base * normal
        sides.append(VR.exact_ratio(a, b, c))
        quads.append([a, b, c])
    assert sides[0] < 0.95 * VR.SHAPE_MIN and sides[1] > 1.05 * VR.SHAPE_MIN, sides
    valid, _ = probe.spheres(np.array(quads))
    assert valid.tolist() == [0, 0, 0, 1]
    assert VR.exact_center(a, b, flat) is None


# ---- membership ---------------------------------------------------------------------------------------------------------------

def test_membership_is_certified_or_uncertain_never_wrong(probe):
    tau = VR.TAU
    rng = np.random.default_rng(5)
    rows, expect = [], []
    for _ in range(40):
        quad = rng.uniform(-4.0, 4.0, (3, 3))
        if VR.exact_ratio(*quad) < 0.05:
            continue
        u = np.array([float(v) for v in VR.exact_center(*quad)])
        r = float(VR.exact_radius(VR.exact_center(*quad)))
        e = rng.normal(size=3)
        e /= np.linalg.norm(e)
        for threshold in (r - tau, r, r + tau):
            for delta in (0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-4, -1e-4):
                rows.append(np.concatenate([quad.ravel(), u + (threshold + delta) * e]))
                expect.append(abs(delta))
    rows = np.array(rows)
    answer, out = probe.classify(rows, tau)
    assert np.all(answer >= 0)
    certified = uncertain = 0
    for k, row in enumerate(rows):
        gap = VR.exact_gaps(VR.exact_center(row[0:3], row[3:6], row[6:9]), [row[9:12]])[0]      # d - r, exactly
        truth = 1 if gap < -VR.Decimal(tau) else (2 if abs(gap) <= VR.Decimal(tau) else 3)
        if answer[k] != 0:
            certified += 1
            assert answer[k] == truth, (k, answer[k], truth, gap)     # never wrong
        else:
            uncertain += 1
            nearest = min(abs(gap + VR.Decimal(tau)), abs(gap - VR.Decimal(tau)))
            assert nearest <= 2 * VR.Decimal(float(out[k, 2])), (k, nearest, out[k, 2])   # uncertain only within the slack
        # a clear case is certified.  Clear: 1e-9 from the threshold - these quadruples have rho <= 20 and coordinates below
        # L = 8, so ec <= eps * 20 * (12 * 8 L + 10 L) = 1.9e-12 and the slack stays below 1e-11
        assert out[k, 2] < 1e-11
        if expect[k] >= 1e-9:
            assert answer[k] == truth, (k, expect[k])
    print("%d certified, %d uncertain of %d" % (certified, uncertain, len(rows)))
    assert certified > 500 and uncertain > 100


# ---- completeness -------------------------------------------------------------------------------------------------------------

def test_an_empty_octant_asks_for_a_larger_radius(probe):
    cell, pos = VR.fixture("sc2")
    R = VR.radius(cell, len(pos), 0)
    q, sid, _ = VR.neighbours(cell, pos, 0, R)
    status, n_far, rec = probe.atom_list(q, sid, 0, R, VR.TAU)
    ref_status, ref_rec, _ = VR.atom_round(q, sid, 0, R, VR.TAU)
    assert status == VR.OK == ref_status and n_far == 0 and len(rec) == len(ref_rec) == 8
    keep = ~np.all(q > 0.0, axis=1)                                   # nobody in the all-positive octant
    status, n_far, rec = probe.atom_list(q[keep], sid[keep], 0, R, VR.TAU)
    assert status == VR.GROW == VR.atom_round(q[keep], sid[keep], 0, R, VR.TAU)[0]
    # a radius too small for the cell: the spheres are empty but not certified within R / 2
    q, sid, _ = VR.neighbours(cell, pos, 0, 0.8 * R)
    status, n_far, _ = probe.atom_list(q, sid, 0, 0.8 * R, VR.TAU)
    assert status == VR.GROW and n_far > 0


# ---- the merge ----------------------------------------------------------------------------------------------------------------

def test_merge_rules(probe):
    cell = np.diag([10.0, 11.0, 12.0])
    mu = VR.MU_FACTOR * VR.TAU
    base = np.array([3.0, 4.0, 5.0])
    e = np.array([1.0, 0.0, 0.0])
    status, _, node, first = probe.merge(cell, [base, base + 0.5 * mu * e, base + 10 * mu * e], mu)
    assert status == VR.OK and node.tolist() == [0, 0, 1] and first.tolist() == [0, 2]
    status, _, _, _ = probe.merge(cell, [base, base + 2.0 * mu * e], mu)
    assert status == VR.UNCERTAIN                                     # two record centres 2 mu apart: ambiguous
    # across the boundary of the cell, and a centre given outside it
    status, w, node, first = probe.merge(cell, [[0.25 * mu, 4.0, 5.0], [10.0 - 0.25 * mu, 4.0, 5.0], [20.0 + 0.3 * mu, 4.0, 5.0]], mu)
    assert status == VR.OK and node.tolist() == [0, 0, 0] and first.tolist() == [0]
    assert np.all((w >= 0.0) & (w < np.diag(cell)))
    ref_status, ref_node, ref_first = VR.merge(cell, w, mu)
    assert ref_status == VR.OK and ref_node.tolist() == [0, 0, 0] and ref_first.tolist() == [0]
    status, _, node, _ = probe.merge(cell, np.zeros((0, 3)), mu)
    assert status == VR.OK and len(node) == 0
    assert probe.merge(np.eye(3) * 7.0 * mu, [base], mu)[0] == VR.CAPACITY    # 8 mu is not below the cell's height


# ---- the whole operator, serially ------------------------------------------------------------------------------------------------

def test_neighbour_lists_are_the_restatements(probe):
    for name in ("small_triclinic", "triclinic", "sc1"):
        cell, pos = VR.fixture(name)
        R = VR.radius(cell, len(pos), 0)
        for i, a in enumerate(probe.atoms(cell, pos, np.arange(len(pos)), R, VR.TAU)):
            q, sid, _ = VR.neighbours(cell, pos, i, R)
            assert a["count"] == len(q) and np.array_equal(a["sid"], sid) and np.array_equal(a["q"], q), (name, i)


MEASURED = {}


@pytest.mark.parametrize("name", sorted(VR.GENERIC) + sorted(VR.IDEAL))
def test_the_serial_driver_gives_the_restatements_nodes(probe, name):
    cell, pos = VR.fixture(name)
    ref = VR.stored(name)
    got = probe.nodes(cell, pos, VR.TAU)
    assert np.array_equal(got["status"], ref["status"]) and np.all(got["status"] == VR.OK), name
    assert got["rounds"] == ref["rounds"] and np.array_equal(got["nbr_count"], ref["nbr_count"]), name
    assert got["merge_status"] == VR.OK and got["records"] == ref["records"]
    assert got["vertices"] == ref["vertices"], name                  # the same nodes in the same order
    dc = synth_mic(got["centers"] - ref["exact_centers"], cell)
    dr = np.abs(got["radii"] - ref["exact_radii"]).max()
    print("%s: %d nodes; largest |centre - exact| %.3g, |radius - exact| %.3g" % (name, len(got["vertices"]), dc, dr))
    if name in VR.GENERIC:
        MEASURED[name] = max(dc, dr)
        assert max(dc, dr) <= VR.CENTER_MEASURED, "a larger error than the recorded measurement: %g" % max(dc, dr)
    else:
        assert dc <= VR.MU_FACTOR * VR.TAU


def synth_mic(d, cell):
    from sitator_amd import synth
    if not len(d):
        return 0.0
    return float(np.linalg.norm(synth.mic_displacement(d, cell), axis=1).max())
