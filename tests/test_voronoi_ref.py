"""CPU-only: the numpy restatement of the Voronoi-node contract (tests/voronoi_ref.py) against its yardsticks, and the conditions
every fixture has to meet so that no test can pass by luck or hide behind a status.

There is no golden from the true reference: Zeo++ cannot be run here.  Generic fixtures: qhull's answer in
tests/golden/voronoi_known_answers.npz (same count, same vertex sets).  Ideal SC, BCC and FCC: the closed-form interstitial
positions and vertex lists of sitator_amd/synth.py.  The restatement's answers stored in the golden file (what the GPU tests read)
are recomputed here.

Conditions, checked with the exact evaluation (Fractions on the float inputs): every shell distance of every node is within
tau / 100 of r or at least 100 tau beyond r + tau; no candidate sphere within the search radius has its deepest neighbour between
tau / 100 and 100 tau inside; every recorded quadruple has |det| / permanent >= 100 VP_SHAPE_MIN; distinct nodes are at least
100 mu apart."""
import numpy as np
import pytest

from sitator_amd import synth
from tests import voronoi_ref as VR

MU = VR.MU_FACTOR * VR.TAU
ALL = sorted(VR.GENERIC) + sorted(VR.IDEAL)


def mic_norm(d, cell):
    return np.linalg.norm(synth.mic_displacement(d, cell), axis=1)


@pytest.mark.parametrize("name", sorted(VR.GENERIC))
def test_generic_fixtures_have_qhulls_nodes(name):
    a, g, k = VR.answer(name), VR.golden(), name + "/"
    cell, pos = VR.fixture(name)
    assert np.array_equal(g[k + "cell"], cell) and np.array_equal(g[k + "pos"], pos)
    off = g[k + "offsets"]
    qhull = [tuple(g[k + "indices"][off[j]:off[j + 1]].tolist()) for j in range(len(off) - 1)]
    assert np.all(a["status"] == VR.OK) and a["merge_status"] == VR.OK
    assert len(a["vertices"]) == len(qhull) and sorted(map(tuple, a["vertices"])) == sorted(qhull)
    by_set = {}
    for j, v in enumerate(qhull):
        by_set.setdefault(v, []).append(g[k + "centers"][j])
    for v, c in zip(a["vertices"], a["centers"]):                        # and where qhull has them (qhull's own error: 1e-8)
        assert min(mic_norm(np.array(by_set[tuple(v)]) - c, cell)) < 1e-8


@pytest.mark.parametrize("name", ["sc1", "sc2", "bcc1", "bcc2", "fcc2"])
def test_ideal_lattices_have_their_closed_form_nodes(name):
    a = VR.answer(name)
    cell, pos = VR.fixture(name)
    want = VR.closed_form(name)
    assert np.all(a["status"] == VR.OK) and len(a["centers"]) == len(want)
    assert sorted(mic_norm(want - c, cell).argmin() for c in a["centers"]) == list(range(len(want)))
    assert all(mic_norm(want - c, cell).min() <= MU for c in a["centers"])
    expect = {"sc1": [1], "sc2": [8] * 8, "bcc1": [2] * 12, "bcc2": [4] * 96, "fcc2": [4] * 64 + [6] * 32}[name]
    assert sorted(len(v) for v in a["vertices"]) == expect


@pytest.mark.parametrize("which", ["sc_grid", "bcc_tet", "fcc_mixed"])
def test_synth_hosts_are_the_restatements_nodes(which):
    """Centres and vertex lists match those of synth.py's hosts as sets."""
    host = {"sc_grid": lambda: synth.sc_grid((3, 3, 3)), "bcc_tet": lambda: synth.bcc_tet(2), "fcc_mixed": lambda: synth.fcc_mixed(2)}[which]()
    a = VR.nodes(host.cell, host.static_pos)
    assert np.all(a["status"] == VR.OK) and len(a["centers"]) == len(host.centers)
    order = [int(mic_norm(a["centers"] - c, host.cell).argmin()) for c in host.centers]
    assert sorted(order) == list(range(len(order)))
    assert all(mic_norm(a["centers"][[k]] - c, host.cell)[0] <= MU for k, c in zip(order, host.centers))
    assert [a["vertices"][k] for k in order] == [sorted(v) for v in host.vertices]


def test_the_void_makes_the_radius_grow():
    a = VR.stored("sc_void")
    assert a["rounds"] == 3 and np.all(a["status"] == VR.OK) and max(len(v) for v in a["vertices"]) == 24
    assert a["nbr_count"].max() < VR.NBR_CAP


@pytest.mark.parametrize("name", ALL)
def test_stored_answers_are_the_restatements_and_fixtures_are_far_from_every_threshold(name):
    a, s = VR.answer(name), VR.stored(name)
    cell, pos = VR.fixture(name)
    assert a["vertices"] == s["vertices"] and np.array_equal(a["status"], s["status"]) and a["rounds"] == s["rounds"]
    assert np.array_equal(a["nbr_count"], s["nbr_count"]) and a["records"] == s["records"]
    assert np.array_equal(a["centers"], s["centers"]) and a["final_radius"] == s["final_radius"]
    tau = VR.Decimal(VR.TAU)
    assert a["margins"]["inside_band"] == 0                             # no candidate's deepest neighbour near the inside threshold
    assert a["margins"]["R_shell"] > 1e-9 and a["margins"]["half_R"] > 1e-9
    worst_on, least_out, least_ratio = VR.Decimal(0), VR.Decimal(10) ** 6, 1.0
    for atom, quad, q, rec in a["all_quads"]:
        gaps = VR.exact_gaps(VR.exact_center(*quad), q)
        for gap in gaps:
            assert gap > -tau / 100, (name, atom, gap)
            if abs(gap) <= tau / 100:
                worst_on = max(worst_on, abs(gap))
            else:
                assert gap >= 101 * tau, (name, atom, gap)
                least_out = min(least_out, gap)
        least_ratio = min(least_ratio, VR.exact_ratio(*quad))
    assert least_ratio >= 100 * VR.SHAPE_MIN, (name, least_ratio)
    c = a["centers"]
    apart = min((mic_norm(c[k + 1:] - c[k], cell).min() for k in range(len(c) - 1)), default=np.inf)
    assert apart >= 100 * MU, (name, apart)
    print("%s: on-shell |d - r| <= %.3g, nearest outsider %.3g beyond r, flattest quadruple %.3g, nearest nodes %.3g apart"
          % (name, float(worst_on), float(least_out), least_ratio, apart))
