"""CPU-only: the decisions of the barrier kernel (sitator_amd/csrc/barrier_plan.h) compiled with the host compiler under ASan /
UBSan into a stand-alone probe, the way test_pathway_graph.py builds its own, and driven over stdin / stdout.  Both compilers
are told -ffp-contract=off, so the pair term, the driven point and the cutoff test pinned here are the ones the kernel evaluates.

The translations.  For every (cell, rc, point, atom) the probe walks the triples the header admits and reports how many pass the
cutoff, a signature of which ones, and their sum; tests/barrier_ref.py finds them by brute force over ranges wider by 2.  The
count and the signature must agree exactly - no term within the cutoff may be missed, none counted twice - and the sum within
the bound of a reordered float64 sum."""
import os
import subprocess

import numpy as np
import pytest

from tests import barrier_ref as BR
from tests import clamp_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, count, n.
#   mode 0: float64 cm[9], ci[9], rc, eps, sigma; count x (x[3], s[3])    -> int64 plan n[3]; count x (int64 terms, signature; float64 e, abs_sum)
#   mode 1: float64 threshold; count x float64 row[n]                     -> count x uint8[3]
#   mode 2: float64 eps, sigma, rc; float64 d2[count]                     -> float64 eps4, sig2, e0; float64 phi[count]
#   mode 3: float64 from[3], vector[3]; float64 coeff[count]              -> float64 x[count, 3]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "barrier_plan.h"

struct Cell { double cm[9], ci[9]; };

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

int main()
{
    int64_t h[3];
    if (fread(h, 8, 3, stdin) != 3) return 2;
    const int64_t mode = h[0], count = h[1], n = h[2];
    if (count < 0 || count > 1000000 || n < 0 || n > 100000) return 3;
    if (mode == 0) {
        Cell c;
        double par[3];
        if (!rd(c.cm, 8, 9) || !rd(c.ci, 8, 9) || !rd(par, 8, 3)) return 2;
        std::vector<double> pts((size_t)(6 * count));
        if (!rd(pts.data(), 8, (size_t)(6 * count))) return 2;
        BarrierPlan pl;
        if (!bp_plan(c, par[0], pl)) return 4;
        const int64_t plan[3] = {pl.n[0], pl.n[1], pl.n[2]};
        wr(plan, 8, 3);
        for (int64_t k = 0; k < count; k++) {
            const double *x = &pts[(size_t)(6 * k)], *s = x + 3;
            double rec[BP_REC], fx[3];
            bp_atom(c, s, par[1], par[2], par[0], rec);
            cp_to_cell(c, x, fx);
            const double e = bp_atom_energy(c, pl, rec, x, fx);
            // which triples: a walk of the admitted ranges, every triple within the cutoff adds a mark of its own
            int lo[3], hi[3];
            for (int a = 0; a < 3; a++) bp_axis_range(fx[a] - rec[3 + a], pl.q[a], pl.n[a], &lo[a], &hi[a]);
            int64_t sig = 0, seen = 0;
            double abs_sum = 0.0;
            for (int m0 = lo[0]; m0 <= hi[0]; m0++)
                for (int m1 = lo[1]; m1 <= hi[1]; m1++)
                    for (int m2 = lo[2]; m2 <= hi[2]; m2++) {
                        double d[3];
                        for (int q = 0; q < 3; q++)
                            d[q] = (x[q] - s[q]) - (((double)m0 * c.cm[3 * q] + (double)m1 * c.cm[3 * q + 1]) + (double)m2 * c.cm[3 * q + 2]);
                        const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                        if (dd <= pl.rc2) {
                            seen++;
                            abs_sum += fabs(bp_phi(dd, rec[7], rec[6], rec[8]));
                            sig += ((int64_t)m0 * 1000003 + (int64_t)m1 * 10007 + (int64_t)m2 * 101) * ((int64_t)m0 + 7 * (int64_t)m1 + 49 * (int64_t)m2 + 1);
                        }
                        if (hi[0] - lo[0] > 2 * pl.n[0] || hi[1] - lo[1] > 2 * pl.n[1] || hi[2] - lo[2] > 2 * pl.n[2]) return 5;
                    }
            const int64_t ints[2] = {seen, sig};
            const double reals[2] = {e, abs_sum};
            wr(ints, 8, 2);
            wr(reals, 8, 2);
        }
        return 0;
    }
    if (mode == 1) {
        double thr;
        if (!rd(&thr, 8, 1) || n < 3) return 2;
        std::vector<double> rows((size_t)(count * n));
        if (!rd(rows.data(), 8, (size_t)(count * n))) return 2;
        for (int64_t k = 0; k < count; k++) {
            uint8_t v[3];
            bp_verdict(&rows[(size_t)(k * n)], (int)n, thr, v);
            wr(v, 1, 3);
        }
        return 0;
    }
    if (mode == 2) {
        double par[3];
        if (!rd(par, 8, 3)) return 2;
        std::vector<double> d2((size_t)count), out((size_t)count);
        if (!rd(d2.data(), 8, (size_t)count)) return 2;
        Cell c = Cell();
        const double zero[3] = {0.0, 0.0, 0.0};
        double rec[BP_REC];
        bp_atom(c, zero, par[0], par[1], par[2], rec);
        for (int64_t k = 0; k < count; k++) out[(size_t)k] = bp_phi(d2[(size_t)k], rec[7], rec[6], rec[8]);
        wr(rec + 6, 8, 3);
        wr(out.data(), 8, (size_t)count);
        return 0;
    }
    if (mode == 3) {
        double path[6];
        if (!rd(path, 8, 6)) return 2;
        std::vector<double> coeff((size_t)count), out((size_t)(3 * count));
        if (!rd(coeff.data(), 8, (size_t)count)) return 2;
        for (int64_t k = 0; k < count; k++) bp_driven(path, path + 3, coeff[(size_t)k], &out[(size_t)(3 * k)]);
        wr(out.data(), 8, (size_t)(3 * count));
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("barrier_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(mode, count, n, *arrays):
        data = np.array([mode, count, n], dtype=np.int64).tobytes() + b"".join(
            np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)
        return subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout
    return run


def signature(m):
    m = np.asarray(m, dtype=np.int64).reshape(-1, 3)
    return int(np.sum((m[:, 0] * 1000003 + m[:, 1] * 10007 + m[:, 2] * 101) * (m[:, 0] + 7 * m[:, 1] + 49 * m[:, 2] + 1)))


CELLS = {
    "cubic": np.eye(3) * 5.0,
    "skewed": np.array([[5.0, 0.0, 0.0], [4.2, 2.6, 0.0], [-3.9, 3.1, 2.2]]),        # heights 1.1, 1.5, 2.2 under vectors of about 5
    "needle": np.array([[2.5, 0.0, 0.0], [0.4, 2.4, 0.0], [0.3, -0.5, 13.0]]),
}


def points_for(cell, seed):
    """(x, s) pairs: both up to three cells outside the cell, atoms given far away, differences on and next to whole cells."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.0, 4.0, (10, 3)) @ cell
    s = rng.uniform(-3.0, 4.0, (10, 3)) @ cell
    s[7] += np.array([40.0, -25.0, 13.0]) @ cell                 # an atom given many cells away
    x[8] = s[8] + np.array([2.0, -1.0, 1.0]) @ cell + 1e-3       # the difference next to a whole number of cells
    x[9] = s[9] + np.array([1e-13, 0.5, -1e-13]) @ cell          # crystal coordinates of the difference at 0 from both sides
    return x, s


@pytest.mark.parametrize("name", sorted(CELLS))
@pytest.mark.parametrize("factor", ["0.3 h_min", "0.5 h_min", "1.0 h_min", "h_max", "1.7 h_max", "3.5 h_max"])
def test_translation_ranges_miss_nothing(probe, name, factor):
    cell = CELLS[name]
    h = BR.heights(cell)
    scale, which = factor.split() if " " in factor else ("1.0", factor)
    rc = float(scale) * (h.min() if which == "h_min" else h.max())
    cm, ci = CR.cell_matrices(cell)
    x, s = points_for(cell, 11)
    eps, sigma = 0.7, rc / 3.0
    raw = probe(0, len(x), 0, cm, ci, [rc, eps, sigma], np.concatenate([x, s], axis=1))
    assert len(raw) == 24 + 32 * len(x)
    plan = np.frombuffer(raw[:24], dtype=np.int64)
    floor_plan = BR.plan_translations(cell, rc)
    assert (plan >= floor_plan).all() and (plan <= floor_plan + 1).all()
    rest = np.frombuffer(raw[24:], dtype=np.dtype([("terms", "<i8"), ("sig", "<i8"), ("e", "<f8"), ("abs", "<f8")]))
    total = 0
    for k in range(len(x)):
        phi, _, _, m = BR.terms(cell, s[k:k + 1], [eps], [sigma], rc, x[k])
        assert rest["terms"][k] == len(phi), "terms within the cutoff: %d found, %d exist" % (rest["terms"][k], len(phi))
        assert rest["sig"][k] == signature(m)
        e, abs_sum, n_terms = BR.mobile_energy(cell, s[k:k + 1], [eps], [sigma], rc, x[k])
        assert n_terms <= 100000
        assert abs(rest["e"][k] - e) <= 1e-10 * abs_sum and abs(rest["abs"][k] - abs_sum) <= 1e-10 * abs_sum
        total += n_terms
    assert total > 0


def test_plan_is_the_floor_formula_away_from_its_ties(probe):
    cell = CELLS["skewed"]
    cm, ci = CR.cell_matrices(cell)
    for rc in (0.2, 1.0, 2.5, 7.3, 19.9):
        raw = probe(0, 0, 0, cm, ci, [rc, 1.0, 1.0], np.zeros((0, 6)))
        assert np.array_equal(np.frombuffer(raw, dtype=np.int64), BR.plan_translations(cell, rc))


INF = np.inf
# (row, what np.argmax's first maximum makes of it)
VERDICT_ROWS = [
    ([5.0, 1.0, 2.0, 3.0, 4.0], "maximum at 0"),
    ([1.0, 2.0, 3.0, 4.0, 5.0], "maximum at n - 1"),
    ([1.0, 2.0, 6.0, 4.0, 3.0], "interior"),
    ([5.0, 1.0, 2.0, 3.0, 5.0], "tie of 0 and n - 1: 0"),
    ([1.0, 6.0, 2.0, 6.0, 3.0], "tie of two interior images: the first"),
    ([6.0, 1.0, 6.0, 2.0, 3.0], "tie of the first end and an interior image: the end"),
    ([1.0, 2.0, 6.0, 3.0, 6.0], "tie of an interior image and the last end: the interior image"),
    ([1.0, INF, 2.0, 3.0, 4.0], "+inf inside"),
    ([INF, 1.0, INF, 2.0, 3.0], "+inf at 0 and inside: inf - inf compares false"),
    ([1.0, 2.0, 3.0, 4.0, INF], "+inf at n - 1"),
    ([1.0, 1.5, 2.0, 1.5, 1.25], "both barriers at the threshold or below"),
    ([1.0, 1.5, 2.0, 1.5, 0.5], "forward only"),
    ([-3.0, -3.0, -3.0, -3.0, -3.0], "flat"),
]


@pytest.mark.parametrize("threshold", [1.0, 0.75, 100.0, -1.0])
def test_verdict_follows_argmax(probe, threshold):
    rows = np.array([r for r, _ in VERDICT_ROWS])
    raw = probe(1, len(rows), rows.shape[1], [threshold], rows)
    got = np.frombuffer(raw, dtype=np.uint8).reshape(len(rows), 3)
    for (row, what), v in zip(VERDICT_ROWS, got):
        assert tuple(bool(b) for b in v) == BR.verdict(row, threshold), what


def test_verdict_with_three_images(probe):
    rows = np.array([[1.0, 2.0, 1.5], [2.0, 1.0, 1.5], [1.0, 1.5, 2.0], [2.0, 2.0, 2.0], [1.0, INF, 1.0]])
    got = np.frombuffer(probe(1, len(rows), 3, [0.6], rows), dtype=np.uint8).reshape(len(rows), 3)
    assert [tuple(bool(b) for b in v) for v in got] == [BR.verdict(r, 0.6) for r in rows]
    assert tuple(got[0]) == (1, 0, 1) and tuple(got[1]) == (0, 1, 1) and tuple(got[4]) == (1, 0, 0)


@pytest.mark.parametrize("eps,sigma,rc", [(1.0, 1.0, 3.0), (0.37, 1.83, 4.9), (2.5e-3, 3.4, 8.5)])
def test_pair_term_is_bit_equal(probe, eps, sigma, rc):
    rng = np.random.default_rng(5)
    d2 = np.concatenate([[0.0, rc * rc, 1e-300, 1e300], rng.uniform(0.01, 1.2, 2000) * rc * rc, 10.0 ** rng.uniform(-8, 3, 500)])
    raw = probe(2, len(d2), 0, [eps, sigma, rc], d2)
    out = np.frombuffer(raw, dtype=np.float64)
    eps4, sig2, e0 = BR.atom_constants(eps, sigma, rc)
    assert out[0].tobytes() == np.float64(eps4).tobytes() and out[1].tobytes() == np.float64(sig2).tobytes()
    assert out[2].tobytes() == np.float64(e0).tobytes()
    exp = BR.phi(d2, sig2, eps4, e0)
    assert out[3:].tobytes() == exp.tobytes()
    assert out[3] == np.inf and not np.isnan(out[3:]).any()      # d = 0: +inf, and never NaN
    assert out[4] == 0.0                                         # shifted: zero at the cutoff


def test_driven_points_are_bit_equal(probe):
    rng = np.random.default_rng(9)
    for n in (3, 4, 20, 67):
        a, b = rng.uniform(0, 10, 3), rng.uniform(0, 10, 3)
        coeffs = np.linspace(0, 1, n)
        out = np.frombuffer(probe(3, n, 0, a, b - a, coeffs), dtype=np.float64).reshape(n, 3)
        exp = ((b - a)[None, :] * coeffs[:, None]) + a[None, :]
        assert out.tobytes() == exp.tobytes()
