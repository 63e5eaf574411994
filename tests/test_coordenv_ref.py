"""CPU-only: the numpy / scipy restatement of SiteCoordinationEnvironment (tests/coordenv_ref.py) against closed forms, and the
margins that make the exact comparisons of tests/test_gpu_coordenv.py and tests/test_coordenv_plan.py meaningful."""
import numpy as np
import pytest

from tests import coordenv_ref as CR


def test_closed_form_shape_measures():
    sh = CR.shapes()
    assert abs(CR.csm(sh["S:4"], sh["T:4"]) - 100.0 / 3.0) <= 1e-11
    assert abs(CR.csm(sh["O:6"], sh["T:6"]) - 16.7367553608) <= 1e-9
    assert abs(CR.csm(sh["T:5"], sh["S:5"]) - 10.4307806183) <= 1e-9
    for sym in CR.SYMBOLS:
        assert np.allclose(np.linalg.norm(sh[sym], axis=1), 1.0, rtol=0, atol=1e-15)
        assert CR.csm(sh[sym], sh[sym]) <= 1e-12, sym
    # the trigonal prism and the square antiprism have all edges equal
    for sym, edges in (("T:6", 9), ("SA:8", 16)):
        p = sh[sym]
        d = np.sort(np.linalg.norm(p[:, None] - p[None], axis=2)[np.triu_indices(len(p), 1)])
        assert np.ptp(d[:edges]) <= 1e-14 and d[edges] > d[0] * 1.2, sym


def test_solid_angles_and_weights():
    square = np.array([[1, 1, 1.0], [-1, 1, 1], [-1, -1, 1], [1, -1, 1]])
    assert abs(CR.polygon_angle(square, np.array([0, 0, 2.0])) - 4 * np.pi / 6) <= 1e-15
    assert CR.polygon_angle(square[:2], np.array([0, 0, 2.0])) == 0.0
    assert CR.weight(0.0) == 1.0 and CR.weight(8.0) == 0.0 and CR.weight(4.0) == 0.25


def test_ideal_lattices_have_the_stated_environments():
    for name, expected in CR.EXPECTED.items():
        ref = CR.answer(name)
        assert [(r["n"], r["symbol"]) for r in ref] == expected, name
    fcc, bcc = CR.answer("fcc"), CR.answer("bcc")
    assert fcc[0]["csm_best"] <= 1e-12 and fcc[1]["csm_best"] <= 1e-12
    assert abs(bcc[0]["csm_all"][0] - 2.2876383367) <= 1e-9 and abs(bcc[0]["csm_all"][1] - 20.0) <= 1e-11 and bcc[0]["confidence"] == 1.0
    assert bcc[1]["symbol"] == "L:2" and abs(bcc[1]["select_margin"] - (np.sqrt(2.0) - 1.4) / 1.4) <= 1e-12     # distance decides
    assert CR.answer("cluster_1.2")[0]["n"] == 6 and CR.answer("cluster_1.1")[0]["n"] == 7
    assert CR.answer("cluster_1.1")[0]["symbol"] == "UN:7" and abs(CR.answer("cluster_1.1")[0]["norm_angle"][-1] - 0.332) <= 1e-3
    assert max(r["rounds"] for r in CR.answer("sc_void")) == 2
    # the second shells of the holes: 1.73 and 1.915 for FCC, 1.612 for the BCC tetrahedral site
    cell, pos, sites = CR.fixture("fcc")
    for c, second in ((sites[0], np.sqrt(3.0)), (sites[1], np.sqrt(11.0 / 3.0))):
        q, _ = CR.site_neighbours(cell, pos, c, 6.0)
        d = np.unique(np.round(np.linalg.norm(q, axis=1), 9))
        assert abs(d[1] / d[0] - second) <= 1e-8


@pytest.mark.parametrize("name", sorted(CR.FIXTURES))
def test_margins(name):
    """Every coordinating decision at least 1e-3 (relative) from its cutoff, every best shape at least 1e-6 in S from the
    runner-up and from max_csm: then neighbour sets, counts and symbols can be compared exactly."""
    for r in CR.answer(name):
        assert r["select_margin"] >= CR.SELECT_MARGIN and r["shape_gap"] >= CR.SHAPE_MARGIN
    if name.endswith("_jitter"):
        for r in CR.answer(name):
            assert r["norm_distance"].max() <= 1.16
