"""GPU: ``sit_coordination_environments`` and ``SiteCoordinationEnvironment.run`` against the numpy / scipy restatement
(tests/coordenv_ref.py: qhull for the site's cell, itertools and SVD for the shape measure).  There is no pymatgen golden: that
package cannot be run here, and agreement with it is not claimed.

Statuses, flags, coordination numbers, the coordinating atoms and their order, the shapes and the rounds of the search radius
are compared exactly (every fixture keeps its decisions 1e-3 from the cutoffs and 1e-6 from the runner-up shape,
tests/test_coordenv_ref.py); shape measures, confidences and the normalised distances and angles within ``coordenv_ref.TOL``
(64 times the largest deviation measured on these fixtures, which must stay below 1e-9).  The shapes are the smallest at which
the kernels can go wrong: coordination numbers 1 to 8 and beyond, both shapes of 8 vertices over all 40 320 assignments,
degenerate spheres of the ideal lattices, a tiny triclinic cell with atoms given several cells outside, a void that makes the
driver grow the search radius, more coordinating atoms than the plan holds."""
import logging

import numpy as np
import pytest

from tests import coordenv_ref as CR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    from sitator_amd import _lib
    made = []

    def get(cell):
        made.append(_lib.HipContext(cell))
        return made[-1]
    yield get
    for ctx in made:
        ctx.close()


def symbol_of(got, k):
    if got["n"][k] == 0:
        return "BAD:0"
    return CR.SYMBOLS[got["shape"][k]] if got["shape"][k] >= 0 else "UN:%d" % got["n"][k]


def deviation(got, ref):
    worst = 0.0
    for k, r in enumerate(ref):
        pairs = [(got["norm_distance"][k], r["norm_distance"]), (got["norm_angle"][k], r["norm_angle"]), (got["csm_all"][k], r["csm_all"]),
                 (got["confidence"][k], r["confidence"])]
        if not np.isnan(r["csm_best"]):
            pairs.append((got["csm_best"][k], r["csm_best"]))
        for a, b in pairs:
            a, b = np.atleast_1d(a), np.atleast_1d(b)
            assert np.array_equal(np.isnan(a), np.isnan(b))
            if np.any(~np.isnan(b)):
                worst = max(worst, float(np.nanmax(np.abs(a - b))))
    return worst


@pytest.mark.parametrize("name", sorted(CR.FIXTURES))
def test_environments_are_the_restatements(contexts, name):
    cell, pos, sites = CR.fixture(name)
    assert len(pos) < 120 and len(sites) < 20
    ref = CR.answer(name)
    got = contexts(cell).coordination_environments(pos, sites, CR.TAU)
    info = got["info"]
    print(name, info)
    assert np.all(got["status"] == CR.OK) and np.all(got["flags"] == 0)
    assert got["n"].tolist() == [r["n"] for r in ref]
    assert [v.tolist() for v in got["vertices"]] == [r["vertices"] for r in ref]          # the same atoms in the same order
    assert [symbol_of(got, k) for k in range(len(sites))] == [r["symbol"] for r in ref]
    assert info["rounds"] == max(r["rounds"] for r in ref) and info["max_neighbours"] == max(r["nbr_count"] for r in ref)
    assert abs(info["final_radius"] - max(r["final_radius"] for r in ref)) <= 1e-12 * info["final_radius"]
    assert info["max_n"] == max(r["n"] for r in ref)
    worst = deviation(got, ref)
    print("%s: largest deviation from the restatement %.3g" % (name, worst))
    assert CR.TOL <= 1e-9 and worst <= CR.TOL
    if name in CR.EXPECTED:
        assert [(int(n), symbol_of(got, k)) for k, n in enumerate(got["n"])] == CR.EXPECTED[name]
    if name == "sc_jitter":                                           # both shapes of 8 vertices, all 40 320 assignments each
        assert np.all(got["n"] == 8) and np.all(~np.isnan(got["csm_all"][:, :2])) and np.all(np.isnan(got["csm_all"][:, 2]))
    if name == "sc_void":
        assert info["rounds"] == 2                                    # the first search radius does not close these cells
    if name == "cluster_1.1":
        assert symbol_of(got, 0) == "UN:7" and got["confidence"][0] == 0.0 and got["csm_best"][0] > CR.MAX_CSM
    if name == "bcc":
        assert abs(got["csm_all"][0, 0] - 2.2876383367) <= 1e-9 and abs(got["csm_all"][0, 1] - 20.0) <= 1e-9
        assert got["confidence"].tolist() == [1.0, 1.0, 1.0]


def test_two_calls_return_the_same_bytes_and_the_fill_call_computes_nothing(contexts):
    cell, pos, sites = CR.fixture("fcc_jitter")
    a = contexts(cell).coordination_environments(pos, sites, CR.TAU)
    b = contexts(cell).coordination_environments(pos, sites, CR.TAU)      # another context: a context keeps its last result
    assert a["info"]["size_computed"] == 1 and a["info"]["fill_computed"] == 0
    for key in ("status", "flags", "n", "shape", "csm_best", "csm_all", "confidence"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for key in ("vertices", "norm_distance", "norm_angle"):
        assert [v.tobytes() for v in a[key]] == [v.tobytes() for v in b[key]], key
    ctx = contexts(cell)
    ctx.coordination_environments(pos, sites, CR.TAU)
    again = ctx.coordination_environments(pos, sites, CR.TAU)             # the same input: nothing is computed at all
    assert again["info"]["size_computed"] == 0 and again["info"]["fill_computed"] == 0
    other = ctx.coordination_environments(pos, sites, CR.TAU, angle_cutoff=0.31)
    assert other["info"]["size_computed"] == 1
    assert other["csm_all"].tobytes() == a["csm_all"].tobytes()


def test_cutoffs_change_the_neighbours(contexts):
    cell, pos, sites = CR.fixture("bcc")
    wide = contexts(cell).coordination_environments(pos, sites[1:2], CR.TAU, distance_cutoff=1.5)
    assert wide["n"].tolist() == [6]                                  # the four atoms at sqrt 2 join the two at 1
    ref = CR.site(cell, pos, sites[1], distance_cutoff=1.5)
    assert wide["vertices"][0].tolist() == ref["vertices"] and symbol_of(wide, 0) == ref["symbol"]
    cell, pos, sites = CR.fixture("cluster_1.2")
    loose = contexts(cell).coordination_environments(pos, sites, CR.TAU, angle_cutoff=0.2)
    assert loose["n"].tolist() == [7]                                 # the 7th atom's face has 0.214 of the largest solid angle


def test_capacity_is_reported_not_truncated(contexts):
    from sitator_amd import CoordinationEnvironmentError, SiteCoordinationEnvironment, SiteNetwork, Structure, _lib
    cap = _lib.coordenv_plan()["coordination_cap"]
    cell, pos = CR.shell(119, 4)
    assert cap < 119
    got = contexts(cell).coordination_environments(pos, np.array([[15.0, 15.0, 15.0]]), CR.TAU)
    assert got["status"].tolist() == [CR.CAPACITY] and got["n"].tolist() == [0] and len(got["vertices"][0]) == 0
    assert got["shape"].tolist() == [-1] and np.all(np.isnan(got["csm_all"]))
    sn = SiteNetwork(Structure(pos, cell), np.ones(len(pos), dtype=bool), np.zeros(len(pos), dtype=bool))
    sn.centers = np.array([[15.0, 15.0, 15.0]])
    with pytest.raises(CoordinationEnvironmentError) as err:
        SiteCoordinationEnvironment().run(sn)
    assert err.value.sites == [0] and err.value.statuses == [CR.CAPACITY]
    assert sn.site_types is None                                      # a partly typed network is never returned


def test_invalid_arguments(contexts):
    cell, pos, sites = CR.fixture("fcc")
    ctx = contexts(cell)
    for kw in (dict(tau=0.0), dict(distance_cutoff=0.9), dict(angle_cutoff=0.0), dict(angle_cutoff=1.5), dict(max_csm=0.0),
               dict(max_csm=np.inf), dict(distance_cutoff=np.nan)):
        with pytest.raises(ValueError):
            ctx.coordination_environments(pos, sites, **kw)
    with pytest.raises(ValueError):
        ctx.coordination_environments(pos, np.zeros((0, 3)))
    bad = sites.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        ctx.coordination_environments(pos, bad)


def small_fcc_network():
    """The conventional FCC cell (a = 4, 4 atoms) with two mobile atoms: 4 octahedral and 8 tetrahedral holes."""
    from sitator_amd import SiteNetwork, Structure
    basis = np.array([(0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0)]) * 4.0 + 0.3
    pos = np.concatenate([basis, [[2.3, 2.3, 2.3], [1.3, 1.3, 1.3]]])
    static = np.array([True] * 4 + [False] * 2)
    return SiteNetwork(Structure(pos, np.eye(3) * 4.0), static, ~static)


def test_operator_after_the_voronoi_generator():
    from sitator_amd import SiteCoordinationEnvironment, VoronoiSiteGenerator
    sn = VoronoiSiteGenerator().run(small_fcc_network())
    assert sn.n_sites == 12
    op = SiteCoordinationEnvironment()
    out = op.run(sn)
    assert out is sn and op.last_info["rounds"] >= 1
    envs = list(sn.coordination_environments)
    assert sorted(set(envs)) == ["O:6", "T:4"] and envs.count("O:6") == 4 and envs.count("T:4") == 8
    assert sn.coordination_numbers.tolist() == [len(v) for v in sn.vertices]
    assert sn.types.tolist() == [0, 1]                                # ordered by coordination number: 4 before 6
    assert np.all((sn.site_types == 0) == (sn.coordination_numbers == 4))
    assert np.all(sn.site_type_confidences == 1.0) and np.all(sn.coordination_csm <= CR.TOL)
    assert all(0 <= i < 4 for v in sn.vertices for i in v)            # statics-only numbering


def test_operator_surface(caplog):
    from sitator_amd import SiteCoordinationEnvironment, SiteNetwork, Structure
    with pytest.raises(NotImplementedError):
        SiteCoordinationEnvironment(guess_ionic_bonds=True)
    with pytest.raises(ValueError):
        SiteCoordinationEnvironment(tolerance=0.0)
    cell, pos, sites = CR.fixture("bcc_jitter")
    ref = CR.answer("bcc_jitter")
    both = np.concatenate([pos, sites[:1]])
    static = np.array([True] * len(pos) + [False])
    sn = SiteNetwork(Structure(both, cell), static, ~static)
    with caplog.at_level(logging.WARNING):
        assert SiteCoordinationEnvironment().run(sn) is sn and sn.site_types is None       # no sites: a warning, as it came
    assert "no sites" in caplog.text
    cell2, pos2, sites2 = CR.fixture("bcc")
    sn.centers = np.concatenate([sites, sites2[1:2]])                 # two T:4 sites and, on the ideal lattice's spot, whatever it is
    ref = ref + [CR.site(cell, pos, sites2[1])]
    SiteCoordinationEnvironment(full_chemenv_site_types=True).run(sn)
    symbols = [r["symbol"] for r in ref]
    assert list(sn.coordination_environments) == symbols
    order = sorted(set(symbols))
    assert sn.site_types.tolist() == [order.index(s) for s in symbols]
    assert sn.coordination_numbers.tolist() == [r["n"] for r in ref] == [len(v) for v in sn.vertices]
    assert np.abs(sn.site_type_confidences - [r["confidence"] for r in ref]).max() <= CR.TOL
    SiteCoordinationEnvironment().run(sn)                             # again, by coordination number: the attributes are replaced
    numbers = sorted(set(r["n"] for r in ref))
    assert sn.site_types.tolist() == [numbers.index(r["n"]) for r in ref]


def test_by_type_entropy_after_the_coordination_environments():
    from sitator_amd import ConfigurationalEntropy, SiteCoordinationEnvironment, SiteTrajectory, VoronoiSiteGenerator
    from tests import entropy_ref as ER
    sn = SiteCoordinationEnvironment().run(VoronoiSiteGenerator().run(small_fcc_network()))
    rng = np.random.default_rng(21)
    labels = rng.integers(-1, 12, size=(48, 2)).astype(np.int64)
    labels[:, 1] = np.where(labels[:, 1] == labels[:, 0], -1, labels[:, 1])
    st = SiteTrajectory(sn, labels)
    got = ConfigurationalEntropy().compute(st)
    residences = ER.residences(labels, 12)
    assert np.array_equal(np.asarray(sn.total_corrected_residences), residences)
    ref = ER.entropy(residences, len(labels), np.asarray(sn.site_types))
    assert abs(got - ref) <= 1e-12 * abs(ref) and got > 0.0
