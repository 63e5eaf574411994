"""CPU-only: the decisions of the device convex hull (sitator_amd/csrc/hull_predicates.h) and its bookkeeping
(sitator_amd/csrc/hull_plan.h) compiled with the host compiler under ASan / UBSan, the way test_pathway_graph.py builds its
probe.  The probe answers orientation tests and drives the wrap serially - one edge after the other, every pivot a chain of
hp_pick in index order - over every site and step of the TRUE reference's recentred point clouds
(tests/golden/site_groups_known_answers.npz) and the designed shapes of tests/hull_ref.py that tests/test_gpu_hull.py runs on
the device.  Both compilers are told -ffp-contract=off, so the signs certified here are the ones the kernel certifies.

Volume bounds.  Against the exact volume of the probe's own facet list: ``hull_ref.volume_bound`` (derived from the inputs).
Against qhull: ``hull_ref.QHULL_REL_TOL``, 64 times the largest relative difference between ``ConvexHull.volume`` and the
exact volume measured over these inputs (``test_qhull_against_the_exact_volume`` prints the measurement and fails if it ever
exceeds the recorded one)."""
import os
import subprocess

import numpy as np
import pytest

from tests import hull_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode.
#   mode 0: int64 n; float64 quad[n, 4, 3] -> int32 sign[n]; float64 det[n], bound[n]
#   mode 1: int64 K, N; int64 offsets[K + 1]; float64 pts[N, 3]
#           -> int32 status[K], n_facets[K], n_vertices[K]; float64 volume[K]; uint8 mask[N]; int32 facets[sum n_facets, 3]
#   mode 2: -> int64 HP_FACET_CAP, HP_OPEN_CAP, HP_BLOCK, HP_LDS_BYTES
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include <vector>
#include "hull_predicates.h"
#include "hull_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

// the pivot about (a, b), one point after the other
static HpCand pivot(const double *pts, int64_t len, const double a[3], const double b[3], bool b_real)
{
    HpCand c = hp_none();
    for (int64_t j = 0; j < len; j++) {
        const double *q = pts + 3 * j;
        if (hp_same(q, a) || (b_real && hp_same(q, b))) continue;
        c = hp_pick(a, b, c, hp_point((uint32_t)j, q));
    }
    return c;
}

static int wrap_site(const double *pts, int64_t len, unsigned char *mask, std::vector<int32_t> &facets, int *n_facets, int *n_vertices, double *volume)
{
    std::vector<HullEdge> open((size_t)HP_OPEN_CAP);
    HullWrap w;
    hw_init(w, open.data());
    *n_facets = 0; *n_vertices = 0; *volume = NAN;
    if (len < 4) return HS_FEW;
    if (len > HP_MAX_POINTS) return HS_CAPACITY;
    HpCand a = hp_none();
    for (int64_t j = 0; j < len; j++) a = hp_pick_least(a, hp_point((uint32_t)j, pts + 3 * j));
    double v[3];
    hp_virtual_second(a.p, v);
    const HpCand b = pivot(pts, len, a.p, v, false);
    if (b.i == HP_NONE || b.uncertain) return HS_UNCERTAIN;
    const HpCand c = pivot(pts, len, a.p, b.p, true);
    if (c.i == HP_NONE || c.uncertain) return HS_UNCERTAIN;
    hw_first(w, a.i, b.i, c.i);
    mask[a.i] = mask[b.i] = mask[c.i] = 1;
    w.n_vertices = 3;
    const int32_t f0[3] = {(int32_t)a.i, (int32_t)b.i, (int32_t)c.i};
    facets.insert(facets.end(), f0, f0 + 3);
    double permanent, vol = hp_det(a.p, b.p, c.p, a.p, &permanent);
    int state = -1;
    for (int step = 0; step < HP_FACET_CAP && state < 0; step++) {
        if (w.overflow) state = HS_CAPACITY;
        else if (w.n_open == 0) state = hw_closed_status(w);
        else if (w.n_facets >= HP_FACET_CAP) state = HS_CAPACITY;
        else {
            const HullEdge e = hw_take(w);
            const double *pu = pts + 3 * (int64_t)e.from, *pv = pts + 3 * (int64_t)e.to;
            const HpCand win = pivot(pts, len, pu, pv, true);
            if (win.i == HP_NONE || win.uncertain) { state = HS_UNCERTAIN; break; }
            const int p1 = hw_find(w.open, 0, w.n_open, e.to, win.i), p2 = hw_find(w.open, 0, w.n_open, win.i, e.from);
            hw_join(w, e, win.i, p1, p2);
            if (!mask[win.i]) { mask[win.i] = 1; w.n_vertices++; }
            const int32_t f[3] = {(int32_t)e.from, (int32_t)e.to, (int32_t)win.i};
            facets.insert(facets.end(), f, f + 3);
            vol += hp_det(pu, pv, win.p, a.p, &permanent);
        }
    }
    if (state < 0) state = HS_CAPACITY;
    *n_facets = w.n_facets; *n_vertices = w.n_vertices;
    if (state == HS_CLOSED) *volume = vol / 6.0;
    return state;
}

int main()
{
    int64_t mode;
    if (fread(&mode, 8, 1, stdin) != 1) return 2;
    if (mode == 0) {
        int64_t n;
        if (fread(&n, 8, 1, stdin) != 1 || n < 0) return 2;
        std::vector<double> quad((size_t)(12 * n)), det((size_t)n), bound((size_t)n);
        std::vector<int32_t> sign((size_t)n);
        if (!rd(quad.data(), 8, (size_t)(12 * n))) return 2;
        for (int64_t k = 0; k < n; k++) {
            const double *p = &quad[(size_t)(12 * k)];
            double permanent;
            sign[(size_t)k] = hp_orient3d(p, p + 3, p + 6, p + 9);
            det[(size_t)k] = hp_det(p, p + 3, p + 6, p + 9, &permanent);
            bound[(size_t)k] = HP_BOUND_A * permanent;
        }
        wr(sign.data(), 4, (size_t)n); wr(det.data(), 8, (size_t)n); wr(bound.data(), 8, (size_t)n);
        return 0;
    }
    if (mode == 2) {
        const int64_t plan[4] = {HP_FACET_CAP, HP_OPEN_CAP, HP_BLOCK, HP_LDS_BYTES};
        wr(plan, 8, 4);
        return 0;
    }
    int64_t h[2];
    if (mode != 1 || fread(h, 8, 2, stdin) != 2 || h[0] < 0 || h[1] < 0) return 2;
    const int64_t K = h[0], N = h[1];
    std::vector<int64_t> off((size_t)K + 1);
    std::vector<double> pts((size_t)(3 * N)), volume((size_t)K);
    if (!rd(off.data(), 8, (size_t)K + 1) || !rd(pts.data(), 8, (size_t)(3 * N))) return 2;
    for (int64_t s = 0; s < K; s++) if (off[(size_t)s] < 0 || off[(size_t)s] > off[(size_t)s + 1] || off[(size_t)s + 1] > N) return 3;
    std::vector<int32_t> status((size_t)K), nf((size_t)K), nv((size_t)K), facets;
    std::vector<unsigned char> mask((size_t)N, 0);
    for (int64_t s = 0; s < K; s++) {
        const int64_t o = off[(size_t)s];
        int f = 0, v = 0;
        const size_t before = facets.size();
        status[(size_t)s] = wrap_site(pts.data() + 3 * o, off[(size_t)s + 1] - o, mask.data() + o, facets, &f, &v, &volume[(size_t)s]);
        nf[(size_t)s] = f; nv[(size_t)s] = v;
        if (facets.size() - before != (size_t)(3 * f)) return 4;
    }
    wr(status.data(), 4, (size_t)K); wr(nf.data(), 4, (size_t)K); wr(nv.data(), 4, (size_t)K); wr(volume.data(), 8, (size_t)K);
    wr(mask.data(), 1, (size_t)N); wr(facets.data(), 4, facets.size());
    return 0;
}
"""


class Probe(object):
    def __init__(self, exe):
        self.exe = exe

    def _run(self, data):
        return subprocess.run([self.exe], input=data, stdout=subprocess.PIPE, check=True).stdout

    def plan(self):
        return tuple(int(v) for v in np.frombuffer(self._run(np.array([2], dtype=np.int64).tobytes()), dtype=np.int64))

    def orient(self, quads):
        quads = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 4, 3)
        n = len(quads)
        raw = self._run(np.array([0, n], dtype=np.int64).tobytes() + quads.tobytes())
        assert len(raw) == 20 * n
        return (np.frombuffer(raw[:4 * n], dtype=np.int32), np.frombuffer(raw[4 * n:12 * n], dtype=np.float64),
                np.frombuffer(raw[12 * n:], dtype=np.float64))

    def wrap(self, offsets, pts):
        """Per site a dict like ``hull_ref.wrap``'s (facets and vertices site-local)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        K, N = len(offsets) - 1, len(pts)
        raw = self._run(np.array([1, K, N], dtype=np.int64).tobytes() + offsets.tobytes() + pts.tobytes())
        status, nf, nv = (np.frombuffer(raw[4 * K * i:4 * K * (i + 1)], dtype=np.int32) for i in range(3))
        vol = np.frombuffer(raw[12 * K:20 * K], dtype=np.float64)
        mask = np.frombuffer(raw[20 * K:20 * K + N], dtype=np.uint8)
        facets = np.frombuffer(raw[20 * K + N:], dtype=np.int32).reshape(-1, 3)
        assert len(facets) == nf.sum()
        cuts = np.concatenate([[0], np.cumsum(nf)])
        return [{"status": int(status[s]), "facets": facets[cuts[s]:cuts[s + 1]].astype(np.int64), "n_vertices": int(nv[s]),
                 "vertices": np.nonzero(mask[offsets[s]:offsets[s + 1]])[0], "volume": float(vol[s])} for s in range(K)]

    def wrap_one(self, pts):
        return self.wrap([0, len(pts)], pts)[0]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("hull_predicates")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])
    return Probe(exe)


# ---- the predicate ------------------------------------------------------------------------------------------------------------

def quadruples():
    """[n, 4, 3]: random ones, ones whose fourth point is moved 0, 1, 2, ... ulps off the plane of the other three, exactly
    coplanar ones (small dyadic coordinates) and ones with a repeated point."""
    rng = np.random.default_rng(11)
    out = [rng.normal(size=(300, 4, 3)) * 10.0 ** rng.integers(-2, 3, size=(300, 1, 1))]
    near = []
    for _ in range(120):
        a, b, c = rng.uniform(-30.0, 30.0, size=(3, 3))
        s, t = rng.uniform(-1.0, 2.0, size=2)
        q = a + s * (b - a) + t * (c - a)                            # on the plane, to rounding
        d = int(rng.integers(0, 3))
        for ulps in range(0, 9):
            p = q.copy()
            for _ in range(ulps):
                p[d] = np.nextafter(p[d], np.inf)
            near.append([a, b, c, p])
            p = q.copy()
            for _ in range(ulps * 16):
                p[d] = np.nextafter(p[d], -np.inf)
            near.append([a, b, c, p])
    out.append(np.array(near))
    flat = rng.integers(-64, 64, size=(150, 4, 3)) / 8.0
    flat[:75, :, 2] = flat[:75, :, 0] + flat[:75, :, 1]               # all four in the plane z = x + y, exactly
    flat[75:, 3] = flat[75:, 0] + 2.0 * (flat[75:, 1] - flat[75:, 0]) - 3.0 * (flat[75:, 2] - flat[75:, 0])
    out.append(flat)
    dup = rng.normal(size=(40, 4, 3))
    for k in range(40):
        dup[k, 3] = dup[k, k % 3]
    out.append(dup)
    return np.concatenate(out)


def test_a_certified_sign_is_the_exact_sign_and_clear_cases_are_certified(probe):
    quads = quadruples()
    sign, det, bound = probe.orient(quads)
    r_det, r_perm = HR.det_permanent(quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3])
    assert np.array_equal(det, r_det) and np.array_equal(bound, HR.BOUND_A * r_perm)       # the restatement's arithmetic is the header's
    assert np.array_equal(sign, HR.orient(quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3]))
    certified = uncertain = 0
    for k, q in enumerate(quads):
        exact = HR.exact_det(*q)
        if sign[k] != HR.UNCERTAIN:
            certified += 1
            assert sign[k] == (HR.POS if exact < 0 else HR.NEG) and exact != 0, (k, q)
        else:
            uncertain += 1
            assert abs(exact) <= 2 * HR.Fraction(float(bound[k])), (k, q)
        assert abs(HR.Fraction(float(det[k])) - exact) <= HR.Fraction(float(bound[k])), (k, q)   # the bound itself
    print("%d certified, %d uncertain of %d" % (certified, uncertain, len(quads)))
    assert certified > 400 and uncertain > 200
    # exactly coplanar and repeated points are never certified
    assert np.all(sign[-190:] == HR.UNCERTAIN)


def test_plan_constants(probe):
    cap, open_cap, block, lds = probe.plan()
    assert cap == HR.FACET_CAP >= 1024 and open_cap == cap + 2 and block == 256
    assert lds <= 64 * 1024


# ---- the wrap -----------------------------------------------------------------------------------------------------------------

def check_site(got, pts, what):
    """A closed site against the restatement, qhull and the exact volume of its own facets."""
    ref = HR.wrap(pts)
    assert got["status"] == HR.CLOSED == ref["status"], what
    assert np.array_equal(got["facets"], ref["facets"]), what                          # the same facets in the same order
    assert got["volume"] == ref["volume"], what
    assert got["n_vertices"] == len(got["vertices"]) and len(got["facets"]) == 2 * got["n_vertices"] - 4, what
    qv, qvol = HR.qhull(pts)
    assert np.array_equal(got["vertices"], qv), what
    exact = HR.exact_volume(pts, got["facets"])
    assert exact > 0
    err = abs(HR.Fraction(got["volume"]) - exact)
    assert err <= HR.Fraction(HR.volume_bound(pts, got["facets"])), what
    rel_q = float(abs(HR.Fraction(qvol) - exact) / exact)
    assert abs(got["volume"] - qvol) <= HR.QHULL_REL_TOL * qvol, what
    return float(err / exact), rel_q


def test_every_site_and_step_of_the_goldens_closes(probe):
    worst, worst_q, n = 0.0, 0.0, 0
    for name, nr, i, s, pts in HR.golden_sites():
        rel, rel_q = check_site(probe.wrap_one(pts), pts, (name, nr, i, s))
        worst, worst_q, n = max(worst, rel), max(worst_q, rel_q), n + 1
    print("%d hulls: largest relative error against the exact volume %.3g, qhull's %.3g" % (n, worst, worst_q))
    assert n == 9 * (4 + 5)
    assert worst_q <= HR.QHULL_MEASURED_REL


@pytest.mark.parametrize("name", sorted(HR.GROUPINGS))
def test_designed_shapes_close(probe, name):
    sites = HR.GROUPINGS[name]
    _, _, off, work = HR.grouping(sites)
    got = probe.wrap(off, work)
    worst_q = 0.0
    for s, site in enumerate(sites):
        pts = work[off[s]:off[s + 1]]
        if site[0] == "doubled":
            # of equal points the first is the vertex: compare coordinates, and the vertices are first copies
            g = got[s]
            assert g["status"] == HR.CLOSED
            qv, qvol = HR.qhull(pts)
            assert {tuple(p) for p in pts[g["vertices"]]} == {tuple(p) for p in pts[qv]}
            first = {tuple(p): k for k, p in reversed(list(enumerate(pts)))}
            assert all(first[tuple(pts[k])] == k for k in g["vertices"])
            assert abs(g["volume"] - qvol) <= HR.QHULL_REL_TOL * qvol
            assert abs(HR.Fraction(g["volume"]) - HR.exact_volume(pts, g["facets"])) <= HR.Fraction(HR.volume_bound(pts, g["facets"]))
        else:
            worst_q = max(worst_q, check_site(got[s], pts, (name, s))[1])
    print("%s: largest relative difference of qhull's volume to the exact one %.3g; most facets %d"
          % (name, worst_q, max(len(g["facets"]) for g in got)))
    assert worst_q <= HR.QHULL_MEASURED_REL
    if name == "shell":
        assert len(got[0]["facets"]) == 1196 and len(got[0]["vertices"]) == 600


def test_flagged_shapes(probe):
    """The cube's corners, fewer than 4 points, a coplanar site, more facets than the capacity: statuses 2, 1, 2, 3."""
    _, _, off, work = HR.grouping(HR.FLAGGED_SITES)
    assert np.array_equal(work[off[0]:off[1]] - work[off[0]], HR.CUBE)                   # the recentring kept the cube exact
    got = probe.wrap(off, work)
    for s, site in enumerate(HR.FLAGGED_SITES):
        assert got[s]["status"] == site[3], site
        assert np.isnan(got[s]["volume"])
        ref = HR.wrap(work[off[s]:off[s + 1]])
        assert ref["status"] == site[3], site
    assert len(got[3]["facets"]) == HR.FACET_CAP
    assert [HR.FLAGGED, HR.FEW, HR.FLAGGED, HR.CAPACITY] == [s[3] for s in HR.FLAGGED_SITES]
