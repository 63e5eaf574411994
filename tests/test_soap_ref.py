"""CPU-only: the two yardsticks of tests/soap_ref.py against each other, and the decisions of the SOAP kernel
(sitator_amd/csrc/soap_plan.h) compiled with the host compiler under ASan / UBSan into a stand-alone probe, the way
test_barrier_plan.py builds its own, and driven over stdin / stdout.

The probe's mode 1 evaluates a centre the way the kernel does - the plan's translation ranges, the solid harmonics by recurrence, the
primitive, the switch, the contraction over the feature table - in one thread; tests/soap_ref.py finds the images by brute force
and takes its harmonics from scipy.  Mode 2 runs the integer bucket plan of SOAPDescriptorAverages, which must reproduce the
weight matrix the TRUE reference gave (tests/golden/soap_averages_known_answers.npz, tools/make_soap_goldens.py) exactly."""
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.special import eval_legendre

from tests import clamp_ref as CR
from tests import soap_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "soap_averages_known_answers.npz")

# stdin: int64 h[8] = mode, ...
#   mode 0: h = {0, l_max, count}; float64 p[count, 3]                      -> float64 R[count, (l_max + 1)^2]
#   mode 1: h = {1, S, n_species, n_max, l_max, crossover, P}; float64 cm[9], ci[9], cutoff, width, sigma, alpha[L n], beta[L n n],
#           pos[S, 3], species[S] (as float64), centres[P, 3]               -> int64 n_dim; P x (int64 terms; float64 p[n_dim])
#   mode 2: h = {2, F, M, K, stepsize, averaging, avg_per_site}; int64 labels[F, M]
#                                                                           -> int64 R, N, averaging used, counts[K], nr[K], averagings[K],
#                                                                              first_row[K], entry[N], row[N], site[N]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "soap_plan.h"

struct Cell { double cm[9], ci[9]; };

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

int main()
{
    int64_t h[8];
    if (fread(h, 8, 8, stdin) != 8) return 2;
    if (h[0] == 0) {
        const int l_max = (int)h[1];
        const int64_t count = h[2];
        if (l_max < 0 || l_max > SP_MAX_L || count < 0 || count > 100000) return 3;
        const int L2 = (l_max + 1) * (l_max + 1);
        std::vector<double> norm((size_t)L2), p((size_t)(3 * count)), out((size_t)(L2 * count));
        if (!rd(p.data(), 8, p.size())) return 2;
        sp_harmonic_norms(l_max, norm.data());
        for (int64_t k = 0; k < count; k++) sp_solid_harmonics(p[3 * k], p[3 * k + 1], p[3 * k + 2], l_max, norm.data(), &out[(size_t)(k * L2)]);
        wr(out.data(), 8, out.size());
        return 0;
    }
    if (h[0] == 1) {
        const int64_t S = h[1], P = h[6];
        const int crossover = (int)h[5];
        SoapShape sh;
        int what;
        if (S < 0 || S > 100000 || P < 0 || P > 10000) return 3;
        if (!sp_shape((int)h[2], (int)h[3], (int)h[4], sh, &what)) return 10 + what;
        Cell c;
        double par[3];
        const int tab = (sh.l_max + 1) * sh.n_max;
        std::vector<double> alpha((size_t)tab), beta((size_t)(tab * sh.n_max)), pos((size_t)(3 * S)), spec((size_t)S), cen((size_t)(3 * P));
        if (!rd(c.cm, 8, 9) || !rd(c.ci, 8, 9) || !rd(par, 8, 3) || !rd(alpha.data(), 8, alpha.size()) || !rd(beta.data(), 8, beta.size()) ||
            !rd(pos.data(), 8, pos.size()) || !rd(spec.data(), 8, spec.size()) || !rd(cen.data(), 8, cen.size()))
            return 2;
        BarrierPlan pl;
        if (!bp_plan(c, par[0], pl)) return 4;
        const double a = 1.0 / (2.0 * par[2] * par[2]);
        std::vector<double> K((size_t)tab), gam((size_t)tab), norm((size_t)sh.L2), harm((size_t)sh.L2);
        for (int l = 0; l <= sh.l_max; l++)
            for (int n = 0; n < sh.n_max; n++) sp_prim_consts(a, alpha[(size_t)(l * sh.n_max + n)], l, &K[(size_t)(l * sh.n_max + n)], &gam[(size_t)(l * sh.n_max + n)]);
        sp_harmonic_norms(sh.l_max, norm.data());
        const int64_t n_dim = sp_n_dim(sh.n_species, sh.n_max, sh.l_max, crossover);
        std::vector<int32_t> feat((size_t)(3 * n_dim));
        if (sp_feature_table(sh.n_species, sh.n_max, sh.l_max, crossover, feat.data()) != n_dim) return 5;
        wr(&n_dim, 8, 1);
        for (int64_t q = 0; q < P; q++) {
            const double *x = &cen[(size_t)(3 * q)];
            double fx[3];
            cp_to_cell(c, x, fx);
            std::vector<double> coef((size_t)sh.n_coef, 0.0), out((size_t)n_dim);
            int64_t terms = 0;
            for (int64_t s = 0; s < S; s++) {
                const int z = (int)spec[(size_t)s];
                if (z < 0) continue;
                if (z >= sh.n_species) return 6;
                double fs[3];
                int lo[3], hi[3];
                cp_to_cell(c, &pos[(size_t)(3 * s)], fs);
                for (int k = 0; k < 3; k++) bp_axis_range(fx[k] - fs[k], pl.q[k], pl.n[k], &lo[k], &hi[k]);
                for (int m0 = lo[0]; m0 <= hi[0]; m0++)
                    for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                        for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                            double p[3];
                            for (int k = 0; k < 3; k++)
                                p[k] = (pos[(size_t)(3 * s + k)] - x[k]) + (((double)m0 * c.cm[3 * k] + (double)m1 * c.cm[3 * k + 1]) + (double)m2 * c.cm[3 * k + 2]);
                            const double d2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
                            if (!(d2 <= pl.rc2)) continue;
                            terms++;
                            const double w = sp_switch(sqrt(d2), par[0], par[1]);
                            sp_solid_harmonics(p[0], p[1], p[2], sh.l_max, norm.data(), harm.data());
                            for (int l = 0; l <= sh.l_max; l++)
                                for (int n = 0; n < sh.n_max; n++) {
                                    double g = 0.0;
                                    for (int k = 0; k < sh.n_max; k++)
                                        g += beta[(size_t)((l * sh.n_max + n) * sh.n_max + k)] * sp_primitive(K[(size_t)(l * sh.n_max + k)], gam[(size_t)(l * sh.n_max + k)], d2);
                                    for (int lm = l * l; lm <= l * l + 2 * l; lm++) coef[(size_t)((z * sh.n_max + n) * sh.L2 + lm)] += (w * g) * harm[(size_t)lm];
                                }
                        }
            }
            for (int64_t f = 0; f < n_dim; f++)
                out[(size_t)f] = sp_contract(&coef[(size_t)(feat[(size_t)(3 * f)] * sh.L2)], &coef[(size_t)(feat[(size_t)(3 * f + 1)] * sh.L2)], feat[(size_t)(3 * f + 2)]);
            wr(&terms, 8, 1);
            wr(out.data(), 8, out.size());
        }
        return 0;
    }
    if (h[0] == 2) {
        const int64_t F = h[1], M = h[2], K = h[3], stepsize = h[4];
        if (F < 0 || M < 0 || K < 1 || F * M > 1000000 || K > 100000 || stepsize < 1) return 3;
        std::vector<int64_t> labels((size_t)(F * M)), counts((size_t)K), nr((size_t)K), avgs((size_t)K), first((size_t)K), w0((size_t)K), w1((size_t)K), w2((size_t)K);
        if (!rd(labels.data(), 8, labels.size())) return 2;
        for (int64_t v : labels)
            if (v < -1 || v >= K) return 6;
        sp_bucket_counts(labels.data(), F, M, K, stepsize, counts.data(), w0.data());
        int zero = 0;
        const int64_t avg = sp_bucket_averaging(counts.data(), K, h[5], h[6], &zero);
        const int64_t R = sp_bucket_rows(counts.data(), K, avg, nr.data(), avgs.data(), first.data());
        const int64_t N = sp_bucket_contributors(labels.data(), F, M, K, stepsize, nr.data(), avgs.data(), first.data(), w0.data(), w1.data(), w2.data(),
                                                 nullptr, nullptr, nullptr);
        std::vector<int64_t> entry((size_t)N), row((size_t)N), site((size_t)N);
        if (sp_bucket_contributors(labels.data(), F, M, K, stepsize, nr.data(), avgs.data(), first.data(), w0.data(), w1.data(), w2.data(),
                                   entry.data(), row.data(), site.data()) != N) return 5;
        const int64_t head[3] = {R, N, zero ? 0 : avg};
        wr(head, 8, 3);
        wr(counts.data(), 8, (size_t)K); wr(nr.data(), 8, (size_t)K); wr(avgs.data(), 8, (size_t)K); wr(first.data(), 8, (size_t)K);
        wr(entry.data(), 8, (size_t)N); wr(row.data(), 8, (size_t)N); wr(site.data(), 8, (size_t)N);
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("soap_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(header, *arrays):
        head = np.zeros(8, dtype=np.int64)
        head[:len(header)] = header
        data = head.tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
        return subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout
    return run


def f64(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]


def probe_vectors(probe, cell, static_pos, species_idx, centers, n_species, par):
    """(p [P, n_dim], terms [P]) from the host build of soap_plan.h."""
    cm, ci = CR.cell_matrices(np.asarray(cell, dtype=np.float64))
    alpha, beta = SR.radial_tables(par["cutoff"], par["n_max"], par["l_max"])
    static_pos = np.asarray(static_pos, dtype=np.float64).reshape(-1, 3)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    raw = probe([1, len(static_pos), n_species, par["n_max"], par["l_max"], int(par["crossover"]), len(centers)],
                *f64(cm, ci, [par["cutoff"], par["cutoff_transition_width"], par["atom_sigma"]], alpha, beta, static_pos, species_idx,
                     centers))
    n_dim = int(np.frombuffer(raw[:8], dtype=np.int64)[0])
    rec = np.frombuffer(raw[8:], dtype=np.dtype([("terms", "<i8"), ("p", "<f8", (n_dim,))]))
    assert len(rec) == len(centers)
    return rec["p"].reshape(len(centers), n_dim), rec["terms"]


def harmonics(probe, l_max, points):
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    raw = probe([0, l_max, len(points)], *f64(points))
    return np.frombuffer(raw, dtype=np.float64).reshape(len(points), (l_max + 1) ** 2)


TRICLINIC = np.array([[6.1, 0.0, 0.0], [1.3, 5.4, 0.0], [-0.9, 1.7, 5.8]])
SMALL_TRICLINIC = np.array([[2.1, 0.0, 0.0], [0.6, 1.9, 0.0], [-0.3, 0.5, 2.4]])


def crystal(cell, S, n_species, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.5, 1.5, (S, 3)) @ cell                  # some atoms given outside the cell
    species = rng.integers(0, n_species, S)
    species[:n_species] = np.arange(n_species)[:S]
    return pos, species


# ---- the two yardsticks against each other --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["one atom", "three atoms, two species", "crossover, switch"])
def test_restate_against_quadrature(case):
    par = SR.params(cutoff=2.0, atom_sigma=0.5, l_max=2, n_max=2, crossover=case.startswith("crossover"),
                    cutoff_transition_width=0.5 if case.startswith("crossover") else 0.0)
    cell = np.eye(3) * 7.0
    center = np.array([3.4, 3.6, 3.5])
    if case == "one atom":
        pos, species, Z = center + [[0.5, -0.8, 0.7]], [0], 1
    else:
        pos, species, Z = center + [[0.5, -0.8, 0.7], [-1.1, 0.3, 0.4], [0.2, 1.3, -1.4]], [0, 1, 0], 2
    p, B, terms = SR.restate(cell, pos, species, [center], Z, par)
    assert terms[0] == len(pos)
    q1, _ = SR.quadrature(cell, pos, species, center, Z, par, nr=60, nt=24, nphi=48)
    q2, _ = SR.quadrature(cell, pos, species, center, Z, par, nr=120, nt=48, nphi=96)
    own = float(np.max(np.abs(q1 - q2)))                         # the quadrature's own error, measured by doubling the rule
    print("quadrature's own error %.3e, restate - quadrature %.3e, largest feature %.3e" % (own, np.max(np.abs(p[0] - q2)), np.max(np.abs(q2))))
    assert own < 1e-6 * np.max(np.abs(q2))
    assert np.max(np.abs(p[0] - q2)) <= 10.0 * own


# ---- the solid harmonics ---------------------------------------------------------------------------------------------------------

def test_solid_harmonics_against_scipy(probe):
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.normal(size=(40, 3)) * 1.7, [[0.0, 0.0, 2.0], [0.0, 0.0, -1.5], [1.0, 0.0, 0.0], [0.0, -2.0, 0.0]]])
    got = harmonics(probe, 8, pts)
    d = np.linalg.norm(pts, axis=1)
    theta, phi = np.arccos(pts[:, 2] / d), np.arctan2(pts[:, 1], pts[:, 0])
    for l in range(9):
        for m in range(-l, l + 1):
            exp = d ** l * SR.y_real(l, m, theta, phi)
            assert np.all(np.abs(got[:, l * l + l + m] - exp) <= 1e-13 * d ** l * math.sqrt((2 * l + 1) / (2 * math.pi))), (l, m)


def test_an_atom_on_the_z_axis_has_only_m_zero(probe):
    got = harmonics(probe, 8, [[0.0, 0.0, 1.3], [0.0, 0.0, -2.2]])
    for l in range(9):
        for m in range(-l, l + 1):
            if m:
                assert np.all(got[:, l * l + l + m] == 0.0)
            else:
                assert np.all(got[:, l * l + l] != 0.0)


def test_a_centre_on_an_atom_is_finite_and_only_l_zero(probe):
    got = harmonics(probe, 8, [[0.0, 0.0, 0.0]])[0]
    assert np.isfinite(got).all() and got[0] == math.sqrt(1.0 / (4.0 * math.pi)) and np.all(got[1:] == 0.0)
    par = SR.params(l_max=4, n_max=3)
    cell = np.eye(3) * 9.0
    for fn in (lambda: SR.restate(cell, [[1.0, 2.0, 3.0]], [0], [[1.0, 2.0, 3.0]], 1, par)[0],
               lambda: probe_vectors(probe, cell, [[1.0, 2.0, 3.0]], [0], [[1.0, 2.0, 3.0]], 1, par)[0]):
        p = fn()[0]
        ls = np.array([f[4] for f in SR.feature_table(1, 3, 4, False)])
        assert np.isfinite(p).all() and np.all(p[ls > 0] == 0.0) and np.all(p[ls == 0] != 0.0)


def test_two_atom_power_spectrum_is_the_addition_theorem(probe):
    par = SR.params(l_max=6, n_max=1, cutoff=3.0)
    cell = np.eye(3) * 12.0
    x = np.array([5.0, 6.0, 5.5])
    p1, p2 = np.array([1.2, -0.7, 0.9]), np.array([-0.4, 1.6, 1.1])
    d1, d2 = np.linalg.norm(p1), np.linalg.norm(p2)
    cosg = float(p1 @ p2) / (d1 * d2)
    alpha, beta = SR.radial_tables(3.0, 1, 6)
    a = 1.0 / (2.0 * 0.4 ** 2)
    exp = []
    for l in range(7):
        K, gam = math.pi ** 1.5 * a ** l * (alpha[l, 0] + a) ** -(l + 1.5), alpha[l, 0] * a / (alpha[l, 0] + a)
        g1, g2 = (beta[l, 0, 0] * K * math.exp(-gam * d * d) * d ** l for d in (d1, d2))
        exp.append(math.pi * math.sqrt(8.0 / (2 * l + 1)) * (2 * l + 1) / (4.0 * math.pi) * (g1 * g1 + g2 * g2 + 2.0 * g1 * g2 * eval_legendre(l, cosg)))
    exp = np.array(exp)
    got_r, B, _ = SR.restate(cell, [x + p1, x + p2], [0, 0], [x], 1, par)
    got_p, terms = probe_vectors(probe, cell, [x + p1, x + p2], [0, 0], [x], 1, par)
    assert terms[0] == 2
    assert np.all(np.abs(got_r[0] - exp) <= 1e-12 * B[0]) and np.all(np.abs(got_p[0] - exp) <= 1e-12 * B[0])


# ---- the host build of the plan against restate, and the invariances ------------------------------------------------------------

@pytest.mark.parametrize("cell_name,cutoff,par", [
    ("cubic", 3.0, dict()), ("triclinic", 3.0, dict(crossover=True)), ("triclinic", 3.0, dict(cutoff_transition_width=1.0)),
    ("small", None, dict(l_max=3, n_max=2, crossover=True)), ("small", None, dict(l_max=1, n_max=2, cutoff_transition_width=1.0))])
def test_host_plan_against_restate(probe, cell_name, cutoff, par):
    cell = {"cubic": np.eye(3) * 6.0, "triclinic": TRICLINIC, "small": SMALL_TRICLINIC}[cell_name]
    if cutoff is None:
        cutoff = 2.6 * SR.heights(cell).min()
    par = SR.params(cutoff=cutoff, **par)
    Z = 3
    pos, species = crystal(cell, 3 if cell_name == "small" else 12, Z, 5)
    species[-1] = -1                                              # an atom of a species outside the environment
    centers = np.concatenate([np.random.default_rng(6).uniform(-1.0, 2.0, (3, 3)) @ cell, pos[:1]])
    exp, B, terms = SR.restate(cell, pos, species, centers, Z, par)
    got, got_terms = probe_vectors(probe, cell, pos, species, centers, Z, par)
    assert np.array_equal(got_terms, terms) and terms.max() > (60 if cell_name == "small" else 3)
    assert np.all(np.abs(got - exp) <= 1e-12 * B)
    assert np.max(np.abs(exp)) > 0


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


@pytest.mark.parametrize("which", ["restate", "probe"])
def test_invariances(probe, which):
    par = SR.params(l_max=4, n_max=3, crossover=True)
    cell, Z = TRICLINIC, 2
    pos, species = crystal(cell, 7, Z, 8)
    centers = np.random.default_rng(9).uniform(0, 1, (2, 3)) @ cell

    def vectors(cell, pos, species, centers):
        if which == "restate":
            out = SR.restate(cell, pos, species, centers, Z, par)
            return out[0], out[1]
        return probe_vectors(probe, cell, pos, species, centers, Z, par)[0], None
    base, B = vectors(cell, pos, species, centers)
    B = SR.restate(cell, pos, species, centers, Z, par)[1] if B is None else B
    Q = rotation(10)
    rot, _ = vectors(cell @ Q.T, pos @ Q.T, species, centers @ Q.T)
    assert np.all(np.abs(rot - base) <= 1e-11 * B)               # a rotation mixes the m of every l: rounding of order l_max^2 terms
    perm = np.random.default_rng(11).permutation(len(pos))
    per, _ = vectors(cell, pos[perm], species[perm], centers)
    assert np.all(np.abs(per - base) <= 1e-12 * B)
    sup, _ = vectors(cell * np.array([[2.0], [1.0], [1.0]]), np.concatenate([pos, pos + cell[0]]), np.concatenate([species, species]), centers)
    assert np.all(np.abs(sup - base) <= 1e-12 * B)


@pytest.mark.parametrize("which", ["restate", "probe"])
def test_an_empty_environment_is_exactly_zero(probe, which):
    par = SR.params(l_max=3, n_max=2)
    cell = np.eye(3) * 20.0
    pos, centers = [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], [[10.0, 10.0, 10.0], [1.5, 1.5, 1.5]]
    species = [0, -1]
    got = SR.restate(cell, pos, species, centers[:1], 1, par)[0] if which == "restate" else probe_vectors(probe, cell, pos, species, centers[:1], 1, par)[0]
    assert np.all(got == 0.0)
    masked = SR.restate(cell, pos, [-1, -1], centers, 1, par)[0] if which == "restate" else probe_vectors(probe, cell, pos, [-1, -1], centers, 1, par)[0]
    assert np.all(masked == 0.0)


def test_feature_count_and_capacity(probe):
    for Z, n, l, cross in [(1, 1, 0, False), (2, 2, 1, True), (3, 6, 6, True), (3, 6, 6, False), (4, 8, 8, True)]:
        par = SR.params(n_max=n, l_max=l, crossover=cross)
        got, _ = probe_vectors(probe, np.eye(3) * 9.0, np.zeros((0, 3)), [], np.zeros((1, 3)), Z, par)
        assert got.shape[1] == len(SR.feature_table(Z, n, l, cross))
    for Z, n, l, code in [(5, 6, 6, 13), (1, 9, 6, 12), (1, 6, 9, 11), (1, 0, 6, 12)]:
        with pytest.raises(subprocess.CalledProcessError) as e:
            probe([1, 0, Z, n, l, 0, 0])
        assert e.value.returncode == code


# ---- the bucket plan against the true reference ----------------------------------------------------------------------------------

def bucket_probe(probe, labels, K, stepsize, averaging, per_site):
    F, M = labels.shape
    raw = np.frombuffer(probe([2, F, M, K, stepsize, averaging, per_site], np.ascontiguousarray(labels, dtype=np.int64)), dtype=np.int64)
    R, N, avg = (int(v) for v in raw[:3])
    parts = np.split(raw[3:], np.cumsum([K, K, K, K, N, N]))
    return dict(zip(["counts", "nr", "averagings", "first_row", "entry", "row", "site"], parts), R=R, N=N, averaging=avg)


def golden_cases():
    g = np.load(GOLDEN)
    return [str(n) for n in g["cases"]]


@pytest.mark.parametrize("name", golden_cases())
def test_bucket_plan_reproduces_the_reference(probe, name):
    g = np.load(GOLDEN)
    labels, K = g[name + "/labels"], int(g[name + "/n_sites"])
    W, d2s = g[name + "/W"], g[name + "/desc_to_site"]
    plan = bucket_probe(probe, labels, K, int(g[name + "/stepsize"]), int(g[name + "/averaging"]), int(g[name + "/avg_descriptors_per_site"]))
    assert plan["R"] == len(W) and np.array_equal(np.repeat(np.arange(K), plan["nr"]), d2s)
    mine = np.zeros_like(W)
    assert len(set(plan["entry"].tolist())) == plan["N"]
    mine[plan["row"], plan["entry"]] = 1.0 / plan["averagings"][plan["site"]]
    assert mine.tobytes() == W.tobytes()
    # the order the rows are added up in: ascending frames
    assert np.all(np.diff(plan["entry"] // labels.shape[1]) >= 0)
    # and the line-by-line numpy restatement of tests/soap_ref.py gives the same
    W2, d2 = SR.bucket_plan(labels, K, int(g[name + "/stepsize"]), int(g[name + "/averaging"]) or None, int(g[name + "/avg_descriptors_per_site"]) or None)
    assert W2.tobytes() == W.tobytes() and np.array_equal(d2, d2s)


def test_golden_cases_cover_the_quirks():
    g = np.load(GOLDEN)
    names = golden_cases()
    assert {int(g[n + "/stepsize"]) for n in names} == {1, 3}
    assert {1, 4} <= {int(g[n + "/averaging"]) for n in names} and any(int(g[n + "/avg_descriptors_per_site"]) for n in names)
    for n in names:
        labels, K = g[n + "/labels"], int(g[n + "/n_sites"])
        assert (labels == -1).any() and not (labels == K - 1).any()
        assert any(len(set(r[r >= 0])) < np.sum(r >= 0) for r in labels[::int(g[n + "/stepsize"])])
    assert any(int(g[n + "/averaging"]) > g[n + "/labels"].shape[0] for n in names)
